"""Tear-off building on the GPU (cg_build_filtered / cg_build_partial_trees, build_filtered.hip) against
oracle.corda: every output table field by field and byte by byte (tests/build_filtered_ref.py), the round
trip through cg_verify_filtered, the device form with exact and short capacities, the statuses, the bare
form, and the Python layer over a Kryo-encoded WireTransaction."""
import hashlib

import numpy as np
import pytest

import build_filtered_ref as R
from build_filtered_ref import bare_cases, notary_filter, wire_transaction
from corda_amd import batch as B
from corda_amd import merkle as M
from oracle import corda as O

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 6, 8, 9, 12, 17, 33)  # components per transaction, the salt leaf included


def _masks(n, rng):
    """Masks over the n - 1 non-salt components."""
    m = n - 1
    one = lambda i: [int(j == i) for j in range(m)]  # noqa: E731
    out = [[0] * m, [1] * m, one(0), one(m - 1), [j & 1 for j in range(m)]]
    if n <= 9:
        out += [one(i) for i in range(m)]
    out += [[int(x) for x in rng.random(m) < d] for d in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.8, 0.9)]
    return out


@pytest.fixture(scope="module")
def inputs():
    """One batch: every size, every mask. (txs, masks, packed tables, visible, the oracle's tables)."""
    rng = np.random.default_rng(41)
    txs, masks = [], []
    for n in SIZES:
        for mask in _masks(n, rng):
            blobs = [rng.integers(0, 256, int(rng.integers(1, 701)), dtype=np.uint8).tobytes() for _ in range(n - 1)]
            txs.append((blobs, rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                        rng.integers(0, 256, int(rng.integers(40, 120)), dtype=np.uint8).tobytes()))
            masks.append(mask)
    t, c, arena = M.pack_transactions(txs)
    vis = M.pack_visible(txs, masks)
    return txs, masks, (t, c, arena), vis, R.filtered_tables(t, c, arena, vis)


@pytest.fixture(scope="module")
def built(engine, inputs):
    _, _, (t, c, arena), vis, _ = inputs
    return engine.build_filtered(t, c, arena, vis)


# 1 ---------------------------------------------------------------- parity
def test_parity_with_the_oracle(inputs, built):
    txs, masks, (t, c, arena), vis, want = inputs
    assert len(txs) == sum(5 + 8 + (n - 1 if n <= 9 else 0) for n in SIZES)
    assert not built[4].any()
    R.assert_same(built, want)
    ftxs, nodes, leaves, out, _, totals = built
    assert int(totals["over"]) == 0
    # what the tables say, spelled out: dense ranges, the root is the id, the nonces, the stream
    node0 = leaf0 = slot0 = 0
    for (blobs, salt, salt_blob), mask, f in zip(txs, masks, ftxs):
        assert (int(f["first_node"]), int(f["first_leaf"]), int(f["root_off"])) == (node0, leaf0, 32 * slot0)
        assert int(f["flags"]) == B.FTX_FILTERED and int(f["n_leaves"]) == sum(mask)
        assert out[32 * slot0:32 * slot0 + 32].tobytes() == O.tx_id(blobs, salt, salt_blob)
        rows = leaves[leaf0:leaf0 + sum(mask)]
        assert [out[int(r["nonce_off"]):int(r["nonce_off"]) + 32].tobytes() for r in rows] == \
            [O.compute_nonce(salt, i) for i, v in enumerate(mask) if v]
        assert [arena[int(r["off"]):int(r["off"]) + int(r["len"])].tobytes() for r in rows] == \
            [b for b, v in zip(blobs, mask) if v]
        n_hash = int(np.count_nonzero(nodes["kind"][node0:node0 + int(f["n_nodes"])] != B.PMT_NODE))
        p = 1
        while p < len(blobs) + 1:
            p <<= 1
        assert int(f["n_nodes"]) <= 2 * p - 1 < 4 * (len(blobs) + 1) and n_hash <= p < 2 * (len(blobs) + 1)
        node0, leaf0, slot0 = node0 + int(f["n_nodes"]), leaf0 + sum(mask), slot0 + 1 + sum(mask) + n_hash
    assert (node0, leaf0, 32 * slot0) == (len(nodes), len(leaves), out.size) == \
        (int(totals["n_nodes"]), int(totals["n_leaves"]), int(totals["out_bytes"]))


# 2 ---------------------------------------------------------------- round trip through cg_verify_filtered
def test_round_trip_through_verify_filtered(engine, inputs):
    _, masks, (t, c, arena), vis, _ = inputs
    out_base = (arena.size + 15) & ~15
    ftxs, nodes, leaves, out, st, _ = engine.build_filtered(t, c, arena, vis, out_base=out_base)
    assert not st.any()
    whole = np.concatenate([arena, np.zeros(out_base - arena.size, np.uint8), out, np.zeros(8, np.uint8)])
    want = np.array([0 if any(m) else 2 for m in masks], np.uint8)
    assert set(want) == {0, 2}
    assert np.array_equal(engine.verify_filtered(ftxs, nodes, leaves, whole), want)
    victim = next(k for k, m in enumerate(masks) if sum(m) >= 2 and k > 20)
    row = leaves[int(ftxs[victim]["first_leaf"]) + 1]
    whole[int(row["nonce_off"]) + 7] ^= 0x20
    want[victim] = 1
    assert np.array_equal(engine.verify_filtered(ftxs, nodes, leaves, whole), want)


# 3 ---------------------------------------------------------------- the device form
def _device_build(engine, t, c, arena, vis, caps, guard_rows=2):
    """cg_build_filtered_device on a side stream; every output buffer poisoned, `guard_rows` rows behind the
    node capacity. Returns the tables as numpy arrays (the whole buffers) and the totals record."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    poison = lambda nbytes: torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device=dev)  # noqa: E731
    node_cap, leaf_cap, out_cap = caps
    d_t, d_c, d_v = up(t), up(c), up(vis)
    d_a = up(np.concatenate([arena, np.zeros(-arena.size % 4, np.uint8)]))
    d_f, d_n = poison(40 * len(t)), poison(16 * (node_cap + guard_rows))
    d_l, d_o, d_s, d_tot = poison(24 * leaf_cap), poison(out_cap), poison(len(t)), poison(32)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        engine.build_filtered_device(d_t.data_ptr(), len(t), d_c.data_ptr(), len(c), d_a.data_ptr(), arena.size,
                                     d_v.data_ptr(), 0, d_f.data_ptr(), d_n.data_ptr(), node_cap, d_l.data_ptr(),
                                     leaf_cap, d_o.data_ptr(), out_cap, d_s.data_ptr(), d_tot.data_ptr(),
                                     stream=s.cuda_stream)
    torch.cuda.synchronize()
    g = lambda d, dt, n: d.cpu().numpy()[:n * np.dtype(dt).itemsize].view(dt)  # noqa: E731
    return (g(d_f, B.FTX_DTYPE, len(t)), g(d_n, B.PMT_NODE_DTYPE, node_cap + guard_rows), g(d_l, B.FLEAF_DTYPE, leaf_cap),
            g(d_o, np.uint8, out_cap), g(d_s, np.uint8, len(t)), g(d_tot, B.BUILD_TOTALS_DTYPE, 1)[0])


@pytest.fixture(scope="module")
def subset(inputs):
    """Every fifth transaction of the batch, packed anew, with the oracle's tables."""
    txs, masks, _, _, _ = inputs
    txs, masks = txs[::5], masks[::5]
    t, c, arena = M.pack_transactions(txs)
    vis = M.pack_visible(txs, masks)
    return (t, c, arena), vis, R.filtered_tables(t, c, arena, vis)


def test_device_form_with_exact_capacities(engine, subset):
    (t, c, arena), vis, want = subset
    caps = (len(want[1]), len(want[2]), want[3].size)
    ftxs, nodes, leaves, out, st, totals = _device_build(engine, t, c, arena, vis, caps)
    assert int(totals["over"]) == 0 and int(totals["reserved"]) == 0
    poison = np.frombuffer(b"\xa5" * 16, B.PMT_NODE_DTYPE)[0]
    assert all(r == poison for r in nodes[caps[0]:])
    R.assert_same((ftxs, nodes[:caps[0]], leaves, out, st, totals), want, "device form")
    R.assert_same(engine.build_filtered(t, c, arena, vis), want, "host form")


def test_device_form_one_node_row_short(engine, subset):
    (t, c, arena), vis, want = subset
    cap = len(want[1]) - 1
    ftxs, nodes, leaves, out, st, totals = _device_build(engine, t, c, arena, vis, (cap, len(want[2]), want[3].size))
    assert int(totals["over"]) == 1
    assert (int(totals["n_nodes"]), int(totals["n_leaves"]), int(totals["out_bytes"])) == \
        (len(want[1]), len(want[2]), want[3].size)  # what the call needs
    poison = np.frombuffer(b"\xa5" * 16, B.PMT_NODE_DTYPE)[0]
    assert all(r == poison for r in nodes[cap:])  # the guard rows
    assert np.array_equal(nodes[:cap], want[1][:cap])
    # the host form refuses the same capacity and names the totals
    from corda_amd import _lib
    import ctypes
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    f, n_, l_ = np.zeros(len(t), B.FTX_DTYPE), np.zeros(cap + 1, B.PMT_NODE_DTYPE), np.zeros(len(want[2]) + 1, B.FLEAF_DTYPE)
    o, s_, tot = np.zeros(want[3].size, np.uint8), np.zeros(len(t), np.uint8), np.zeros(1, B.BUILD_TOTALS_DTYPE)
    rc = _lib.lib().cg_build_filtered(engine._h, p(t), len(t), p(c), len(c), p(arena), arena.size, p(vis), 0, p(f),
                                      p(n_), cap, p(l_), len(want[2]), p(o), o.size, p(s_), p(tot))
    assert rc == -1 and int(tot[0]["over"]) == 1 and int(tot[0]["n_nodes"]) == cap + 1
    assert "%d node rows" % (cap + 1) in _lib.last_error() and not n_.view(np.uint8).any()


# 4 ---------------------------------------------------------------- statuses
def test_statuses_leave_the_neighbours_alone(engine):
    rng = np.random.default_rng(43)
    txs = [([rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes() for _ in range(k % 5 + 1)],
            bytes([k + 1]) * 32, b"salt blob %d" % k) for k in range(14)]
    masks = [[(i + k) & 1 for i in range(len(b))] for k, (b, _, _) in enumerate(txs)]
    t, c, arena = M.pack_transactions(txs)
    vis = M.pack_visible(txs, masks)
    first = lambda k: int(t[k]["first"])  # noqa: E731
    malformed = {}
    t[1]["n"] = 0                                     # no leaves
    t[3]["first"] = len(c) - 1                        # the range runs past the component table
    t[3]["n"] = 5
    t[5]["salt_off"] = arena.size - 31                # the salt runs past the arena
    malformed.update({1: 1, 3: 1, 5: 1})
    c[first(7) + 1]["off"] = arena.size + 1           # a component outside the arena
    malformed[7] = 2
    t[10]["first"] = first(9) + 1                     # claims two components of transaction 9
    malformed.update({9: 3, 10: 3})
    vis[first(11) + int(t[11]["n"]) - 1] = 1          # a visible privacy salt
    vis[first(12)] = 2                                # a visible byte that is neither 0 nor 1
    got = engine.build_filtered(t, c, arena, vis)
    want_st = np.zeros(len(t), np.uint8)
    for k, v in malformed.items():
        want_st[k] = v
    want_st[[11, 12]] = B.BUILD_BAD_VISIBLE
    assert got[4].tolist() == want_st.tolist()
    assert sorted(set(want_st)) == [0, 1, 2, 3, 6] and np.count_nonzero(want_st == 0) == 6
    ids, id_st = engine.tx_ids(t, c, arena)
    assert [int(s) for s in id_st] == [int(s) if s != 6 else 0 for s in want_st]  # 1 / 2 / 3 as cg_tx_ids
    R.assert_same(got, R.filtered_tables(t, c, arena, vis, 0, malformed), "statuses")
    for k in np.flatnonzero(want_st):
        f = got[0][k]
        assert (int(f["n_nodes"]), int(f["n_leaves"])) == (0, 0)
        assert not got[3][int(f["root_off"]):int(f["root_off"]) + 32].any()


# 5 ---------------------------------------------------------------- bare PartialMerkleTree.build
def test_partial_trees_bare_form(engine):
    cases = bare_cases()
    leaf_lists, include = [c[0] for c in cases], [c[1] for c in cases]
    assert {len(x) for x in leaf_lists} >= set(range(0, 10)) | {17}
    want = R.partial_tree_tables(leaf_lists, include)
    got = engine.build_partial_trees(leaf_lists, include)
    assert sorted(set(want[4])) == [0, 1, 4, 5]
    R.assert_same(got, want, "bare form")
    # the tables are the input of bare PartialMerkleTree.verify: out[] is the arena
    ftxs, nodes, leaves, out, st, _ = got
    arena = np.concatenate([out, np.zeros(8, np.uint8)])
    assert engine.verify_filtered(ftxs, nodes, leaves, arena).tolist() == [0 if s == 0 else 3 for s in st]
    # and through the object layer
    res = M.PartialMerkleTree.build_batch(leaf_lists, include, engine)
    tuples = []
    for (lv, inc), r, s in zip(cases, res, st):
        if s == 0:
            root, pmt = r
            assert root == O.merkle_root(lv)
            tuples.append((root, inc, None, pmt))
        else:
            assert type(r) is type(M.build_status_exception(s)) and str(r) == str(M.build_status_exception(s))
    assert not M.verify_filtered_batch(tuples, engine, filtered=False).any()
    # one tree, several include lists: the leaf lists may share leaves
    hs = [hashlib.sha256(bytes([k])).digest() for k in range(9)]
    shared = engine.build_partial_trees([hs, hs, hs], [[hs[0]], [hs[8], hs[3]], []])
    R.assert_same(shared, R.partial_tree_tables([hs, hs, hs], [[hs[0]], [hs[8], hs[3]], []]), "shared leaves")


def test_partial_trees_device_form(engine):
    """cg_build_partial_trees_device on a side stream: lists that share leaves, exact capacities and
    leaf_total = the sum of the counts; then a list outside its table and a leaf_total that the last tree
    passes (status 1 for those, the neighbours built); a misaligned hash table is refused."""
    import torch
    from corda_amd import _lib
    hs = [hashlib.sha256(b"dev %d" % k).digest() for k in range(12)]
    lists = [hs[:9], hs[:9], hs[2:7], hs[11:12], hs[:12]]
    include = [[hs[0], hs[8]], [], [hs[4]], [hs[11]], [hs[5], hs[6], hs[10]]]
    want = R.partial_tree_tables(lists, include)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    poison = lambda nbytes: torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device=dev)  # noqa: E731
    first = np.array([0, 0, 2, 11, 0], np.uint64)
    count = np.array([len(x) for x in lists], np.uint32)
    inc_flat = [h for x in include for h in x]
    inc_count = np.array([len(x) for x in include], np.uint32)
    inc_first = (np.cumsum(inc_count) - inc_count).astype(np.uint64)
    d_lv = up(np.frombuffer(b"".join(hs) + bytes(4), np.uint8).copy())
    d_inc = up(np.frombuffer(b"".join(inc_flat), np.uint8).copy())
    d_first, d_count, d_if, d_ic = up(first), up(count), up(inc_first), up(inc_count)
    n, caps = len(lists), (len(want[1]), len(want[2]), want[3].size)

    def run(n_leaf_hashes, leaf_total, lv_ptr=None):
        d_f, d_n, d_l = poison(40 * n), poison(16 * (caps[0] + 1)), poison(24 * caps[1])
        d_o, d_s, d_tot = poison(caps[2]), poison(n), poison(32)
        s = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            engine.build_partial_trees_device(lv_ptr or d_lv.data_ptr(), n_leaf_hashes, d_first.data_ptr(),
                                              d_count.data_ptr(), n, leaf_total, d_inc.data_ptr(), len(inc_flat),
                                              d_if.data_ptr(), d_ic.data_ptr(), 0, d_f.data_ptr(), d_n.data_ptr(),
                                              caps[0], d_l.data_ptr(), caps[1], d_o.data_ptr(), caps[2],
                                              d_s.data_ptr(), d_tot.data_ptr(), stream=s.cuda_stream)
        torch.cuda.synchronize()
        g = lambda d, dt, k: d.cpu().numpy()[:k * np.dtype(dt).itemsize].view(dt)  # noqa: E731
        return (g(d_f, B.FTX_DTYPE, n), g(d_n, B.PMT_NODE_DTYPE, caps[0] + 1), g(d_l, B.FLEAF_DTYPE, caps[1]),
                g(d_o, np.uint8, caps[2]), g(d_s, np.uint8, n), g(d_tot, B.BUILD_TOTALS_DTYPE, 1)[0])

    got = run(12, int(count.sum()))
    assert int(got[5]["over"]) == 0 and got[1][caps[0]] == np.frombuffer(b"\xa5" * 16, B.PMT_NODE_DTYPE)[0]
    R.assert_same((got[0], got[1][:caps[0]], *got[2:]), want, "device form")
    # a table of 11 hashes: the lists that reach hash 11 lie outside it
    assert run(11, int(count.sum()))[4].tolist() == [0, 0, 0, 1, 1]
    # leaf_total is the scratch the trees share, in order: 9 + 9 + 5 + 1 fit into 24, the last tree does not
    got = run(12, 24)
    assert got[4].tolist() == [0, 0, 0, 0, 1] and int(got[5]["over"]) == 0
    short = R.partial_tree_tables(lists[:4], include[:4])
    assert np.array_equal(got[1][:len(short[1])], short[1]) and np.array_equal(got[0][:4], short[0])
    with pytest.raises(_lib.EngineUnavailable, match=r"\(-1\).*not 4-byte aligned"):
        run(11, int(count.sum()), d_lv.data_ptr() + 1)


# 6 ---------------------------------------------------------------- the Python layer
def test_wire_transaction_build_filtered_transaction(engine):
    wtx = wire_transaction()
    d = wtx.data()
    f = wtx.build_filtered_transaction(notary_filter, engine)
    # the host path: merkle_tree, then PartialMerkleTree.build
    hashes = [O.component_hash(b, d.salt, i) for i, b in enumerate(d.components)] + [O.sha256(d.salt_blob)]
    tree = M.merkle_tree(hashes, engine)
    vis = [i for i, c in enumerate(wtx.available_components()) if notary_filter(c)]
    host = M.FilteredTransaction(tree.hash, [d.components[i] for i in vis], [O.compute_nonce(d.salt, i) for i in vis],
                                 M.PartialMerkleTree.build(tree, [hashes[i] for i in vis]))
    assert vis == [0, 1, 6]
    assert (f.root_hash, f.component_blobs, f.nonces) == (host.root_hash, host.component_blobs, host.nonces)
    assert f.partial_merkle_tree.postorder() == host.partial_merkle_tree.postorder()
    assert f.root_hash == O.tx_id(d.components, d.salt, d.salt_blob)
    assert f.verify(engine) is True
    with pytest.raises(M.MerkleTreeException, match="without included leaves"):
        wtx.build_filtered_transaction(lambda c: False, engine).verify(engine)
