"""Test helper for tear-off building (cg_build_filtered / cg_build_partial_trees): the expected output tables,
byte for byte, from oracle.corda (tx_id, compute_nonce, component_hash, merkle_tree, partial_tree_build,
partial_tree_postorder), in the layout include/cordagpu.h documents, computed once per input and shared; and the
cases more than one test file uses (the bare form's rules, the Kryo-encoded WireTransaction)."""
import hashlib

import numpy as np

from corda_amd import batch as B
from corda_amd import kryo as K
from oracle import corda as O


class Tables:
    """The rows as Python lists while they grow, numpy tables at the end."""

    def __init__(self, out_base):
        self.out_base, self.ftxs, self.nodes, self.leaves, self.slots, self.status = out_base, [], [], [], [], []

    def slot(self, h):
        self.slots.append(bytes(h))
        return self.out_base + 32 * (len(self.slots) - 1)

    def failed(self, status, flags):
        self.ftxs.append((len(self.nodes), len(self.leaves), self.slot(bytes(32)), 0, 0, flags, 0))
        self.status.append(status)

    def stream(self, stream):
        for kind, h in stream:
            self.nodes.append((0 if h is None else self.slot(h), kind, 0))

    def done(self):
        arr = lambda rows, dt: np.array(rows, dt) if rows else np.zeros(0, dt)  # noqa: E731
        out = np.frombuffer(b"".join(self.slots), np.uint8).copy()
        totals = np.zeros(1, B.BUILD_TOTALS_DTYPE)[0]
        totals["n_nodes"], totals["n_leaves"], totals["out_bytes"] = len(self.nodes), len(self.leaves), out.size
        return (arr(self.ftxs, B.FTX_DTYPE), arr(self.nodes, B.PMT_NODE_DTYPE), arr(self.leaves, B.FLEAF_DTYPE), out,
                np.array(self.status, np.uint8), totals)


def filtered_tables(txs, comps, arena, visible, out_base=0, malformed=None):
    """What cg_build_filtered writes for well-formed cg_tx / cg_component tables (the statuses of ``malformed``,
    {tx index: status}, are taken as given: those transactions' tables are not read)."""
    T = Tables(out_base)
    a = arena.tobytes()
    for t, tx in enumerate(txs):
        if malformed and t in malformed:
            T.failed(malformed[t], B.FTX_FILTERED)
            continue
        first, n = int(tx["first"]), int(tx["n"])
        rows, vis = comps[first:first + n], [int(v) for v in visible[first:first + n]]
        if any(v > 1 for v in vis) or any(v and (int(r["flags"]) & 1) for v, r in zip(vis, rows)):
            T.failed(B.BUILD_BAD_VISIBLE, B.FTX_FILTERED)
            continue
        salt = a[int(tx["salt_off"]):int(tx["salt_off"]) + 32]
        blobs = [a[int(r["off"]):int(r["off"]) + int(r["len"])] for r in rows]
        hashes = [O.component_hash(b, salt, i, is_salt=bool(int(r["flags"]) & 1)) for i, (b, r) in enumerate(zip(blobs, rows))]
        root = O.merkle_root(hashes)
        if int(rows[-1]["flags"]) & 1 and not any(int(r["flags"]) & 1 for r in rows[:-1]):
            assert root == O.tx_id(blobs[:-1], salt, blobs[-1])
        pt = O.partial_tree_build(O.merkle_tree(hashes), [h for h, v in zip(hashes, vis) if v])
        node0, leaf0 = len(T.nodes), len(T.leaves)
        root_off = T.slot(root)
        for i, (r, v) in enumerate(zip(rows, vis)):
            if v:
                T.leaves.append((int(r["off"]), T.slot(O.compute_nonce(salt, i)), int(r["len"]), 0))
        T.stream(O.partial_tree_postorder(pt))
        T.ftxs.append((node0, leaf0, root_off, len(T.nodes) - node0, sum(vis), B.FTX_FILTERED, 0))
        T.status.append(0)
    return T.done()


def partial_tree_tables(leaf_lists, include_lists, out_base=0):
    """What cg_build_partial_trees writes."""
    T = Tables(out_base)
    for leaves, include in zip(leaf_lists, include_lists):
        if not leaves:
            T.failed(1, 0)
            continue
        try:
            pt = O.partial_tree_build(O.merkle_tree(leaves), include)
        except O.MerkleTreeException:
            T.failed(B.BUILD_NOT_IN_TREE, 0)
            continue
        except ValueError:
            T.failed(B.BUILD_ZERO_HASH, 0)
            continue
        node0, leaf0 = len(T.nodes), len(T.leaves)
        root_off = T.slot(O.merkle_root(leaves))
        for h in include:
            T.leaves.append((T.slot(h), 0, 32, B.FLEAF_HASH))
        T.stream(O.partial_tree_postorder(pt))
        T.ftxs.append((node0, leaf0, root_off, len(T.nodes) - node0, len(include), 0, 0))
        T.status.append(0)
    return T.done()


def assert_same(got, want, what=""):
    """Field by field and byte by byte; the totals' three counts (``over`` is the caller's to check)."""
    names = ("ftxs", "nodes", "leaves", "out", "status")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.dtype.names:
            for f in g.dtype.names:
                bad = np.flatnonzero(g[f] != w[f])
                assert bad.size == 0, (what, name, f, bad[:5], g[f][bad[:5]], w[f][bad[:5]])
        else:
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (what, name, bad[:5])
    for f in ("n_nodes", "n_leaves", "out_bytes"):
        assert int(got[5][f]) == int(want[5][f]), (what, f)


class OracleEngine:
    """A stand-in for Engine.build_filtered / build_partial_trees on the CPU: the oracle's tables."""

    def __init__(self):
        self.calls = []

    def build_filtered(self, txs, comps, arena, visible, out_base=0):
        self.calls.append((txs.copy(), comps.copy(), arena.copy(), np.array(visible, np.uint8)))
        malformed = {t: 1 for t, tx in enumerate(txs) if int(tx["n"]) == 0}
        return filtered_tables(txs, comps, arena, visible, out_base, malformed)

    def build_partial_trees(self, leaf_lists, include_lists, out_base=0):
        return partial_tree_tables(leaf_lists, include_lists, out_base)


# ---------------------------------------------------------------- shared cases
def leaf_hashes(n, tag=0):
    return [hashlib.sha256(b"leaf %d %d" % (tag, i)).digest() for i in range(n)]


def bare_cases():
    """(leaves, include list): the rules of PartialMerkleTree.build by value."""
    a, b, c, d = leaf_hashes(4, 77)
    out = [([a, b, c], [a, a]),             # a duplicate in the include list
           ([a, b, c], [d]),                # a hash the tree lacks
           ([a, b, c], [b, d]),
           ([a, a, a], [a]),                # an included hash that also sits at other leaves
           ([a, b, a], [a]),
           ([a, b, c], [bytes(32)]),        # zeroHash: IllegalArgumentException
           ([a, b, c], [a, bytes(32)]),
           ([a, a, b], [a, a]),             # both copies of a duplicated leaf: builds
           ([a, b, c], []),                 # nothing included: one Leaf(root)
           ([a], [a]), ([a], []),
           ([], [a]), ([], [])]             # no leaves
    rng = np.random.default_rng(21)
    for n in list(range(1, 10)) + [17]:
        hs = leaf_hashes(n, 100 + n)
        for _ in range(4):
            pick = [hs[i] for i in np.flatnonzero(rng.random(n) < 0.4)]
            rng.shuffle(pick)               # the include list's order does not matter
            out.append((hs, [bytes(x) for x in pick]))
    return out


def prefix_tables(want, n):
    """The oracle's tables for the first n transactions (or trees) of a batch: the tables are dense and in
    order, so this is a cut at transaction n's first_node / first_leaf / root_off (out_base 0)."""
    ftxs, nodes, leaves, out, st, totals = want
    if n == len(ftxs):
        return want
    f = ftxs[n]
    cut = (int(f["first_node"]), int(f["first_leaf"]), int(f["root_off"]))
    t = np.zeros(1, B.BUILD_TOTALS_DTYPE)[0]
    t["n_nodes"], t["n_leaves"], t["out_bytes"] = cut
    return ftxs[:n], nodes[:cut[0]], leaves[:cut[1]], out[:cut[2]], st[:n], t


def row_counts(want):
    """Per transaction (or tree) the three counts k_bf_scan scans: node rows, leaf rows, 32-byte slots."""
    ftxs, _, _, out, _, _ = want
    ends = np.append(ftxs["root_off"][1:], out.size).astype(np.int64)
    return (ftxs["n_nodes"].astype(np.int64), ftxs["n_leaves"].astype(np.int64),
            (ends - ftxs["root_off"].astype(np.int64)) // 32)


DEEP_COUNTS = (31, 32, 33, 255, 256, 257, 1025, 4097)   # 33, 257, 1025, 4097: P / 2 + 1
DEEP_MASKS = ("none", "first", "last", "split", "alternate", "p01", "p50", "all")


def deep_masks(n, m=None):
    """{name: mask over n leaves} of which only the first m (default: all) may be included: nothing, the first
    leaf, the last includable leaf, both sides of the top split (leaves P/2 - 1 and P/2), every other leaf,
    seeded random at density 0.01 and 0.5, all."""
    m = n if m is None else m
    p = 1
    while p < n:
        p <<= 1
    rng = np.random.default_rng(1000 + n)
    sets = {"none": [], "first": [0], "last": [m - 1], "split": [p // 2 - 1, p // 2], "alternate": range(0, n, 2),
            "p01": np.flatnonzero(rng.random(n) < 0.01), "p50": np.flatnonzero(rng.random(n) < 0.5),
            "all": range(n)}
    assert tuple(sets) == DEEP_MASKS
    out = {}
    for name, idx in sets.items():
        mask = [0] * n
        for i in idx:
            if i < m:
                mask[int(i)] = 1
        out[name] = mask
    return out


def wire_transaction():
    """The WireTransaction of tests/test_kryo.py (test_wire_transaction_id_from_encoded_components)."""
    h = K.SecureHash(hashlib.sha256(b"prev").digest())
    notary = K.Party(K.x500_der("CN=Notary,O=R3,L=London,C=GB"), K.PublicKeyRef(4, bytes(range(32))))
    iou = K.CordaObject("com.example.state.IOUState", (("iou", "object", K.CordaObject("com.example.state.IOU", (
        ("value", "int", 7),))), ("sender", "party", notary)))
    return K.WireTransaction(inputs=[K.StateRef(h, 0), K.StateRef(h, 1)], attachments=[h],
                             outputs=[K.TransactionState(iou, notary)],
                             commands=[K.Command(K.CordaObject("com.example.Cmd$Create"), (notary.owning_key,))],
                             notary=notary, time_window=K.TimeWindow((1_700_000_000, 5), None),
                             privacy_salt=K.PrivacySalt(bytes(range(1, 33))))


def notary_filter(c):
    """NotaryFlow.Client: Predicate { it is StateRef || it is TimeWindow }."""
    return isinstance(c, (K.StateRef, K.TimeWindow))
