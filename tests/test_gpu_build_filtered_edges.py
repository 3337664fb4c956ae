"""Tear-off building on the GPU, the paths tests/test_gpu_build_filtered.py does not reach. Everything is
byte-exact against oracle.corda (tests/build_filtered_ref.py); every precondition a case rests on is asserted
on the CPU next to it.

1. k_bf_scan over more than one 1024-counter tile, transaction form: 3 x 1024 + 1 transactions whose three
   counts differ from one to the next, failed transactions on both sides of the tile boundaries, prefixes
   that end one short of, on and one past a boundary (the carry, the wsum reuse, the `i < n` tail, the totals
   from the carry), and the round trip through cg_verify_filtered.
2. The same for the bare form, whose extra scan (k_pt_widen + k_bf_scan without totals) places every tree's
   scratch bytes: 2049 trees over one shared table of 64 hashes, host form and device form.
3. Deep trees: bare lists of 31 .. 4097 leaves (levels 5 .. 13) and transactions of 64 .. 257 components, with
   masks that make the largest hidden blocks and, at P / 2 + 1 leaves, padding blocks of every size; deep and
   one-leaf trees alternate, so lanes 0, 63 and 64 of the 64-lane kernels walk trees of different depth.
4. Every capacity guard of the device forms, both forms: leaf rows one short, out bytes 32 and 1 short (the
   latter no multiple of 32: the last slot stays unwritten), all three capacities 0; 0xA5 behind every capacity.
5. k_bf_leaves' own nonce code with salts at every byte phase and a salt ending the arena.
6. The context's buffers reused by a smaller call and by cg_tx_ids between two large calls.

Not covered: trees above 2^30 leaves (status 1: such a list cannot be built in a test), totals above 2^32, and
NULL tables in a device-form call (the host's argument checks are tests/test_gpu_api_args.py's)."""
import hashlib

import numpy as np
import pytest

import build_filtered_ref as R
import layout_util as LU
from corda_amd import batch as B
from corda_amd import merkle as M
from oracle import corda as O
from test_gpu_build_filtered import inputs, subset  # noqa: F401  (fixtures: that file's batch, every fifth of it)

pytestmark = pytest.mark.gpu

TILE = 1024                                 # counters per tile of k_bf_scan
FAILED = (1023, 1024, 2047, 3072)           # (0, 0, 1) counts on both sides of the boundaries
GUARD_ROWS, GUARD_BYTES = 2, 64


def _rb(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _counts_of(want):
    return [int(want[5][f]) for f in ("n_nodes", "n_leaves", "out_bytes")]


def _verify_arena(out):
    return np.concatenate([out, np.zeros(8, np.uint8)])


# ---------------------------------------------------------------- device forms, every table guarded
class _Device:
    """Uploads, poisoned result buffers with guard rows / bytes behind every capacity, and the call on a side
    stream. run() returns the whole buffers (capacity + guard) as numpy arrays and the totals record."""

    def __init__(self, n, caps):
        import torch
        self.torch, self.dev, self.n, self.caps = torch, torch.device("cuda", 0), n, caps
        node_cap, leaf_cap, out_cap = caps
        self.sizes = (40 * n, 16 * (node_cap + GUARD_ROWS), 24 * (leaf_cap + GUARD_ROWS),
                      (out_cap + 31) // 32 * 32 + GUARD_BYTES, n, 32)
        self.bufs = [torch.full((max(s, 16),), 0xA5, dtype=torch.uint8, device=self.dev) for s in self.sizes]

    def up(self, x):
        return self.torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(self.dev)

    def run(self, call):
        torch = self.torch
        s = torch.cuda.Stream(device=self.dev)
        torch.cuda.synchronize()
        f, nd, lf, o, st, tot = (b.data_ptr() for b in self.bufs)
        with torch.cuda.stream(s):
            call((f, nd, self.caps[0], lf, self.caps[1], o, self.caps[2], st, tot), s.cuda_stream)
        torch.cuda.synchronize()
        dts = (B.FTX_DTYPE, B.PMT_NODE_DTYPE, B.FLEAF_DTYPE, np.uint8, np.uint8, B.BUILD_TOTALS_DTYPE)
        got = [b.cpu().numpy()[:size].view(dt) for b, size, dt in zip(self.bufs, self.sizes, dts)]
        return got[:5] + [got[5][0]]


def _device_tx(engine, t, c, arena, vis, caps):
    d = _Device(len(t), caps)
    d_t, d_c, d_v = d.up(t), d.up(c), d.up(vis)
    d_a = d.up(np.concatenate([arena, np.zeros(-arena.size % 4, np.uint8)]))
    return d.run(lambda o, stream: engine.build_filtered_device(
        d_t.data_ptr(), len(t), d_c.data_ptr(), len(c), d_a.data_ptr(), arena.size, d_v.data_ptr(), 0, *o,
        stream=stream))


def _device_bare(engine, table, first, count, include, caps, leaf_total=None):
    """table: the leaf hashes the lists share; list j is table[first[j] : first[j] + count[j]]."""
    d = _Device(len(count), caps)
    inc_flat = [h for x in include for h in x]
    inc_count = np.array([len(x) for x in include], np.uint32)
    inc_first = (np.cumsum(inc_count) - inc_count).astype(np.uint64)
    d_lv = d.up(np.frombuffer(b"".join(table) + bytes(4), np.uint8))
    d_inc = d.up(np.frombuffer(b"".join(inc_flat) + bytes(4), np.uint8))
    d_first, d_count = d.up(np.asarray(first, np.uint64)), d.up(np.asarray(count, np.uint32))
    d_if, d_ic = d.up(inc_first), d.up(inc_count)
    leaf_total = int(np.sum(count)) if leaf_total is None else leaf_total
    return d.run(lambda o, stream: engine.build_partial_trees_device(
        d_lv.data_ptr(), len(table), d_first.data_ptr(), d_count.data_ptr(), len(count), leaf_total, d_inc.data_ptr(),
        len(inc_flat), d_if.data_ptr(), d_ic.data_ptr(), 0, *o, stream=stream))


def _assert_guarded(got, want, caps, what):
    """A device-form result against the oracle under capacities `caps`: ftxs, status and totals complete, every
    row and slot below its capacity the oracle's, every byte at or past a capacity still 0xA5."""
    ftxs, nodes, leaves, out, st, totals = got
    node_cap, leaf_cap, out_cap = caps
    assert _counts_of(got) == _counts_of(want), what
    need = (len(want[1]), len(want[2]), want[3].size)
    assert int(totals["over"]) == int(any(n > c for n, c in zip(need, caps))) and int(totals["reserved"]) == 0, what
    k = (min(node_cap, need[0]), min(leaf_cap, need[1]), min(out_cap // 32 * 32, need[2]))
    R.assert_same((ftxs, nodes[:k[0]], leaves[:k[1]], out[:k[2]], st, want[5]),
                  (want[0], want[1][:k[0]], want[2][:k[1]], want[3][:k[2]], want[4], want[5]), what)
    for name, table, kept in (("nodes", nodes, k[0]), ("leaves", leaves, k[1]), ("out", out, k[2])):
        tail = table[kept:].view(np.uint8)
        assert tail.size >= (GUARD_BYTES if name == "out" else GUARD_ROWS * table.itemsize), (what, name)
        assert np.all(tail == 0xA5), (what, name, "written at or past the capacity", np.flatnonzero(tail != 0xA5)[:5])


# ---------------------------------------------------------------- 1. multi-tile scans, transaction form
@pytest.fixture(scope="module")
def big():
    """3 x 1024 + 1 small transactions, four of them failed: (packed tables, visible, the oracle's tables,
    the expected cg_verify_filtered statuses)."""
    rng = np.random.default_rng(51)
    txs, masks = [], []
    for _ in range(3 * TILE + 1):
        n = int(rng.integers(1, 5))                       # components, the salt leaf included
        txs.append(([_rb(rng, rng.integers(1, 41)) for _ in range(n - 1)], _rb(rng, 32), _rb(rng, rng.integers(1, 41))))
        masks.append([0] * (n - 1) if rng.random() < 0.2 else [int(x) for x in rng.random(n - 1) < 0.5])
    t, c, arena = M.pack_transactions(txs)
    vis = M.pack_visible(txs, masks)
    malformed = {}
    for j, k in enumerate(FAILED):
        if j % 2 == 0:
            t[k]["n"] = 0                                 # status 1
            malformed[k] = 1
        else:
            vis[int(t[k]["first"])] = 2                   # status 6
    want = R.filtered_tables(t, c, arena, vis, malformed=malformed)
    verdicts = np.array([0 if any(m) else 2 for m in masks], np.uint8)
    verdicts[list(FAILED)] = 3                            # no node rows: malformed for cg_verify_filtered
    return (t, c, arena), vis, want, verdicts


def test_big_batch_preconditions(big):
    (t, c, arena), vis, want, verdicts = big
    assert len(t) == 3 * TILE + 1 and set(verdicts) == {0, 2, 3}
    assert np.flatnonzero(want[4]).tolist() == list(FAILED)
    assert want[4][list(FAILED)].tolist() == [1, B.BUILD_BAD_VISIBLE, 1, B.BUILD_BAD_VISIBLE]
    counts = R.row_counts(want)
    for k in FAILED:
        assert [int(x[k]) for x in counts] == [0, 0, 1]
    carries = []
    for b in (TILE, 2 * TILE, 3 * TILE):
        # around every tile boundary each count takes several values, so an offset that lost or doubled a
        # carry, or took a neighbour's count, cannot land on the right row by accident
        for x in counts:
            assert len(set(x[b - 8:b + 8].tolist())) >= 3
        carries.append(tuple(int(x[:b].sum()) for x in counts))
    assert all(min(cr) > 0 for cr in carries) and len(set(carries)) == 3
    assert len({tuple(int(x[b:b + TILE].sum()) for x in counts) for b in (0, TILE, 2 * TILE)}) == 3  # no two tiles alike


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 2049, 3073])
def test_scan_across_tiles(engine, big, n):
    (t, c, arena), vis, want, _ = big
    if n in (1025, 2049, 3073):
        assert (n - 1) % TILE == 0                        # the last transaction alone occupies the last tile
    got = engine.build_filtered(t[:n].copy(), c, arena, vis)  # the components behind the prefix: unclaimed
    assert int(got[5]["over"]) == 0
    R.assert_same(got, R.prefix_tables(want, n), "%d transactions" % n)


def test_big_batch_round_trip_through_verify_filtered(engine, big):
    (t, c, arena), vis, want, verdicts = big
    out_base = (arena.size + 15) & ~15
    ftxs, nodes, leaves, out, st, _ = engine.build_filtered(t, c, arena, vis, out_base=out_base)
    assert np.array_equal(st, want[4])
    whole = np.concatenate([arena, np.zeros(out_base - arena.size, np.uint8), out, np.zeros(8, np.uint8)])
    assert np.array_equal(engine.verify_filtered(ftxs, nodes, leaves, whole), verdicts)


# ---------------------------------------------------------------- 2. multi-tile scans, bare form
BARE_FAILED = {1022: 5, 1023: 1, 1024: 4, 1025: 5, 2046: 4, 2047: 1}
BARE_NEIGHBOURS = {1021: 0, 1026: 2, 2045: 0, 2048: 2}   # the built trees next to the boundaries: 3 leaves, this one included


@pytest.fixture(scope="module")
def bare_big():
    """2049 trees over one table of 64 hashes: (table, first, count, lists, include lists, the oracle's tables)."""
    rng = np.random.default_rng(52)
    table = R.leaf_hashes(64, 52)
    n = 2 * TILE + 1
    count = rng.integers(1, 7, n)
    count[list(BARE_NEIGHBOURS)] = 3
    first = np.array([int(rng.integers(0, 65 - k)) for k in count])
    include = []
    for j in range(n):
        own = table[first[j]:first[j] + count[j]]
        pick = [] if rng.random() < 0.15 else [own[i] for i in np.flatnonzero(rng.random(len(own)) < 0.5)]
        rng.shuffle(pick)
        include.append([bytes(x) for x in pick] if j not in BARE_NEIGHBOURS else [own[BARE_NEIGHBOURS[j]]])
    for j, s in BARE_FAILED.items():
        if s == 1:
            count[j] = 0
        elif s == 4:
            include[j] = include[j] + [bytes(32)]
        else:
            include[j] = include[j] + [hashlib.sha256(b"not in the table").digest()]
    lists = [table[f:f + k] for f, k in zip(first, count)]
    return table, first, count, lists, include, R.partial_tree_tables(lists, include)


def _bare_mask(lists, include, j):
    return bytes(int(h in include[j]) for h in lists[j])


def test_bare_big_preconditions(bare_big):
    table, first, count, lists, include, want = bare_big
    assert len(lists) == 2 * TILE + 1 and len(set(table)) == 64
    assert {j: int(s) for j, s in enumerate(want[4]) if s} == BARE_FAILED
    assert set(count.tolist()) == set(range(7)) and any(not x for x in include)
    built = np.flatnonzero(want[4] == 0)
    for b in (TILE, 2 * TILE):
        # the nearest built trees on either side of the boundary mark different bytes: were their scratch
        # ranges to overlap (a lost carry in the scan of the leaf counts), one of them would come out wrong
        lo, hi = int(built[built < b][-1]), int(built[built >= b][0])
        assert lo in BARE_NEIGHBOURS and hi in BARE_NEIGHBOURS
        assert hi - lo <= 5 and _bare_mask(lists, include, lo) != _bare_mask(lists, include, hi)
        assert any(_bare_mask(lists, include, lo)) and any(_bare_mask(lists, include, hi))
        for x in R.row_counts(want):
            assert len(set(x[b - 8:b + 8].tolist())) >= 3
        assert int(count[:b].sum()) > 0


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_bare_scan_across_tiles(engine, bare_big, n):
    _, _, _, lists, include, want = bare_big
    assert n != 1025 and n != 2049 or (n - 1) % TILE == 0
    got = engine.build_partial_trees(lists[:n], include[:n])
    assert int(got[5]["over"]) == 0
    R.assert_same(got, R.prefix_tables(want, n), "%d trees" % n)


def test_bare_scan_across_tiles_device_form(engine, bare_big):
    table, first, count, _, include, want = bare_big
    caps = (len(want[1]), len(want[2]), want[3].size)
    _assert_guarded(_device_bare(engine, table, first, count, include, caps), want, caps, "bare device form")


# ---------------------------------------------------------------- 3. deep trees
# cg_verify_filtered's multiset comparison reads every node row and every leaf hash once per included leaf, on
# one lane. A tree is sent through it if that is at most this many reads (1025 leaves all included: 3.2 M);
# 4097 leaves with half or all of them included would be 21 M and 67 M, seconds of one lane. Those three trees
# are compared with the oracle byte for byte like the rest, and 4097 leaves go through verify with the five
# sparse masks.
VERIFY_READS = 4 << 20


@pytest.fixture(scope="module")
def deep_bare():
    """(leaf lists, include lists, tree depth per list): deep trees count-major, a one-leaf tree behind each."""
    lists, include, depth = [], [], []
    for n in R.DEEP_COUNTS:
        hs = R.leaf_hashes(n, 300 + n)
        for k, mask in enumerate(R.deep_masks(n).values()):
            lists += [hs, hs[k:k + 1]]
            include += [[h for h, v in zip(hs, mask) if v], hs[k:k + 1] if k & 1 else []]
            depth += [(n - 1).bit_length(), 0]
    return lists, include, depth


def test_deep_bare_trees(engine, deep_bare):
    lists, include, depth = deep_bare
    assert len(lists) == 2 * len(R.DEEP_COUNTS) * len(R.DEEP_MASKS) > 65
    assert len({depth[0], depth[63], depth[64]}) == 3 and max(depth) == 13      # lanes 0, 63, 64 of the 64-lane kernels
    assert all((a == 0) != (b == 0) for a, b in zip(depth, depth[1:]))           # deep and one-leaf trees alternate
    for n in (33, 257, 1025, 4097):                                              # P / 2 + 1: one leaf right of the split
        assert n in R.DEEP_COUNTS and (n - 1) & (n - 2) == 0
    want = R.partial_tree_tables(lists, include)
    assert not want[4].any()
    got = engine.build_partial_trees(lists, include)
    assert int(got[5]["over"]) == 0
    R.assert_same(got, want, "deep bare trees")
    ftxs, nodes, leaves, out, _, _ = got
    reads = ftxs["n_leaves"].astype(np.int64) * (ftxs["n_nodes"].astype(np.int64) + ftxs["n_leaves"])
    keep = reads <= VERIFY_READS
    names = [(n, name) for n in R.DEEP_COUNTS for name in R.DEEP_MASKS]      # of the deep tree at row 2 k
    assert {names[j // 2] for j in np.flatnonzero(~keep)} == {(4097, "alternate"), (4097, "p50"), (4097, "all")}
    assert not engine.verify_filtered(ftxs[keep], nodes, leaves, _verify_arena(out)).any()


def test_deep_transactions(engine):
    rng = np.random.default_rng(53)
    txs, masks = [], []
    for n in (64, 65, 129, 257):                          # components, the salt leaf included
        for mask in R.deep_masks(n, n - 1).values():      # the salt leaf is never visible
            assert len(mask) == n and mask[-1] == 0
            txs.append(([_rb(rng, 1) for _ in range(n - 1)], _rb(rng, 32), _rb(rng, 1)))
            masks.append(mask)
    assert [sum(m) for m in masks[-8:-5]] + [sum(masks[-1])] == [0, 1, 1, 256] and masks[-6][255] == 1
    t, c, arena = M.pack_transactions(txs)
    vis = M.pack_visible(txs, masks)
    want = R.filtered_tables(t, c, arena, vis)
    assert not want[4].any()
    out_base = (arena.size + 15) & ~15
    got = engine.build_filtered(t, c, arena, vis)
    assert int(got[5]["over"]) == 0
    R.assert_same(got, want, "deep transactions")
    ftxs, nodes, leaves, out, _, _ = engine.build_filtered(t, c, arena, vis, out_base=out_base)
    whole = np.concatenate([arena, np.zeros(out_base - arena.size, np.uint8), out, np.zeros(8, np.uint8)])
    verdicts = [0 if any(m) else 2 for m in masks]
    assert set(verdicts) == {0, 2}
    assert engine.verify_filtered(ftxs, nodes, leaves, whole).tolist() == verdicts


# ---------------------------------------------------------------- 4. every capacity guard, both forms
SHORT = {"leaf rows - 1": lambda nd, lf, o: (nd, lf - 1, o),
         "out bytes - 32": lambda nd, lf, o: (nd, lf, o - 32),
         "out bytes - 1": lambda nd, lf, o: (nd, lf, o - 1),
         "all zero": lambda nd, lf, o: (0, 0, 0)}


@pytest.mark.parametrize("short", list(SHORT))
def test_device_form_short_capacity(engine, subset, short):
    (t, c, arena), vis, want = subset
    need = (len(want[1]), len(want[2]), want[3].size)
    caps = SHORT[short](*need)
    assert min(need) > 2 and need[2] % 32 == 0 and (short != "out bytes - 1" or caps[2] % 32 == 31)
    got = _device_tx(engine, t, c, arena, vis, caps)
    assert int(got[5]["over"]) == 1
    _assert_guarded(got, want, caps, short)
    if short == "all zero":
        assert all(np.all(x.view(np.uint8) == 0xA5) for x in got[1:4])


@pytest.mark.parametrize("short", list(SHORT))
def test_bare_device_form_short_capacity(engine, short):
    """The lists of test_partial_trees_device_form."""
    hs = [hashlib.sha256(b"dev %d" % k).digest() for k in range(12)]
    first, count = [0, 0, 2, 11, 0], [9, 9, 5, 1, 12]
    lists = [hs[f:f + k] for f, k in zip(first, count)]
    include = [[hs[0], hs[8]], [], [hs[4]], [hs[11]], [hs[5], hs[6], hs[10]]]
    want = R.partial_tree_tables(lists, include)
    need = (len(want[1]), len(want[2]), want[3].size)
    caps = SHORT[short](*need)
    assert not want[4].any() and need[1] == 7 and (short != "out bytes - 1" or caps[2] % 32 == 31)
    assert int(want[0][-1]["n_leaves"]) == 3              # the last tree's include loop crosses the leaf capacity
    got = _device_bare(engine, hs, first, count, include, caps)
    assert int(got[5]["over"]) == 1
    _assert_guarded(got, want, caps, short)
    if short == "all zero":
        assert all(np.all(x.view(np.uint8) == 0xA5) for x in got[1:4])


# ---------------------------------------------------------------- 5. the builder's nonce path at odd layouts
@pytest.fixture(scope="module")
def relaid():
    cases, cph, sph = LU.tx_case()
    rng = np.random.default_rng(55)
    masks = [[int(x) for x in rng.random(len(blobs)) < rng.choice([0.0, 0.3, 0.7, 1.0])] for blobs, _, _ in cases]
    masks[-1][0] = 1                                      # the transaction whose salt will end the arena
    t, c, arena = M.pack_transactions(cases)
    vis = M.pack_visible(cases, masks)
    want = R.filtered_tables(t, c, arena, vis)
    assert not want[4].any() and np.array_equal(want[2]["off"], c["off"][vis == 1])
    assert any(not any(m) for m in masks) and any(all(m) for m in masks) and len(want[2]) > 1000
    return (t, c, arena), cph, sph, vis, want


def _relaid_case(relaid, rem):
    (t, c, arena), cph, sph, vis, want = relaid
    t2, c2, a2 = LU.relayout_tx(t, c, arena, 37, lead=5, rem=rem, last="salt", comp_phase=cph, salt_phase=sph)
    st = LU.layout_stats(LU.tx_fields(t2, c2), a2.size, mod=64)
    assert a2.size % 4 == rem and st["salt"]["ends"] and not st["comp"]["ends"]
    assert {p % 4 for p in st["salt"]["phases"]} == {0, 1, 2, 3} and st["comp"]["phases"] == set(range(64))
    # a visible component of the transaction whose salt ends the arena: its nonce reads the arena's last bytes
    last = int(np.flatnonzero(t2["salt_off"] + 32 == a2.size)[0])
    assert vis[int(t2[last]["first"]):int(t2[last]["first"]) + int(t2[last]["n"])].any()
    leaves = want[2].copy()
    leaves["off"] = c2["off"][vis == 1]
    assert not np.array_equal(leaves["off"], want[2]["off"])
    return t2, c2, a2, (want[0], want[1], leaves, want[3], want[4], want[5])


@pytest.mark.parametrize("rem", LU.REMS)
def test_build_filtered_relaid_out(engine, relaid, rem):
    t2, c2, a2, want = _relaid_case(relaid, rem)
    got = engine.build_filtered(t2, c2, a2, relaid[3])
    assert int(got[5]["over"]) == 0
    R.assert_same(got, want, "rem %d" % rem)


def test_build_filtered_relaid_out_device_form(engine, relaid):
    t2, c2, a2, want = _relaid_case(relaid, 3)
    caps = (len(want[1]), len(want[2]), want[3].size)
    _assert_guarded(_device_tx(engine, t2, c2, a2, relaid[3], caps), want, caps, "relaid out, device form")


# ---------------------------------------------------------------- 6. reuse of the context's buffers
def test_buffers_reused_by_a_smaller_call(engine, big):
    (t, c, arena), vis, want, _ = big
    rng = np.random.default_rng(56)
    small = [([_rb(rng, 90), _rb(rng, 7), _rb(rng, 300)], _rb(rng, 32), _rb(rng, 50)) for _ in range(3)]
    small_masks = [[1, 0, 1], [0, 0, 0], [1, 1, 1]]
    ts, cs, as_ = M.pack_transactions(small)
    vs = M.pack_visible(small, small_masks)
    other = [([_rb(rng, rng.integers(1, 200)) for _ in range(k % 7 + 1)], _rb(rng, 32), _rb(rng, 33)) for k in range(500)]
    to, co, ao = M.pack_transactions(other)
    r1 = engine.build_filtered(t, c, arena, vis)
    r2 = engine.build_filtered(ts, cs, as_, vs)
    ids, id_st = engine.tx_ids(to, co, ao)
    r4 = engine.build_filtered(t, c, arena, vis)
    R.assert_same(r1, want, "first large call")
    R.assert_same(r2, R.filtered_tables(ts, cs, as_, vs), "small call after a large one")
    assert not id_st.any() and [bytes(x) for x in ids] == [O.tx_id(*x) for x in other]
    R.assert_same(r4, r1, "second large call")
    assert int(r1[5]["over"]) == int(r2[5]["over"]) == int(r4[5]["over"]) == 0
