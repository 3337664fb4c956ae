"""Test helper: content-preserving repackers of the engine's packed inputs.

include/cordagpu.h puts no alignment requirement on any arena offset. Each ``relayout_*`` takes the
packed tables the engine takes and returns the same tables over a new arena in which

  * every referenced byte range keeps its contents and moves to a byte phase drawn from a seeded
    RNG (mod 4; mod 64 for transaction components, whose kernel indexes 64-byte sectors),
  * every gap and the ``lead`` bytes in front hold ``poison``, and at least one poison byte
    directly follows every field,
  * the arena ends exactly at the last byte of the last field (no slack) with
    ``arena.size % 4 == rem``,
  * the fields are emitted so that a field of kind ``last`` is the one that touches the end.

The ``*_fields`` functions list the byte ranges a set of tables references (kind -> offsets,
lengths); ``same_content`` / ``layout_stats`` turn the rules above into checks a test can state
as preconditions. Plain numpy, no GPU.
"""
import numpy as np

from corda_amd import batch as B


class _Spec:
    """One kind of field: rows of ``tab`` whose ``off`` column points at ``lens[row]`` arena bytes."""

    def __init__(self, kind, tab, off, lens, mod=4, mask=None):
        self.kind, self.tab, self.off, self.mod = kind, tab, off, mod
        self.lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), (len(tab),))
        self.mask = np.ones(len(tab), bool) if mask is None else np.asarray(mask, bool)

    def ranges(self):
        rows = np.flatnonzero(self.mask)
        return self.tab[self.off][rows].astype(np.int64), self.lens[rows]


def _fields(groups):
    out = {}
    for g in groups:
        for s in g:
            out[s.kind] = s.ranges()
    return out


def _relayout(src, groups, last, seed, lead, poison, rem, phases=None):
    """Moves every field of ``groups`` (lists of _Spec over one table each, emitted row by row) out
    of ``src`` into a new arena and rewrites the offset columns in place. Returns the arena."""
    assert 0 <= rem < 4 and 0 <= poison < 256
    phases = phases or {}
    rng = np.random.default_rng(seed)
    kinds = [s.kind for g in groups for s in g]
    assert last in kinds, f"last={last!r} is not one of {kinds}"
    groups = sorted(groups, key=lambda g: any(s.kind == last for s in g))   # stable: last's group at the end
    groups[-1] = sorted(groups[-1], key=lambda s: s.kind == last)
    seq = []
    for g in groups:
        for row in range(len(g[0].tab)):
            seq.extend((s, row) for s in g if s.mask[row])
    ends = [j for j, (s, row) in enumerate(seq) if s.kind == last and s.lens[row] > 0]
    assert ends, f"no non-empty field of kind {last!r} to end the arena on"
    seq.append(seq.pop(ends[-1]))
    placed, pos = [], int(lead)
    for j, (s, row) in enumerate(seq):
        ln = int(s.lens[row])
        want = phases.get(s.kind)
        ph = int(want[row]) if want is not None and want[row] >= 0 else int(rng.integers(0, s.mod))
        if j == len(seq) - 1:     # the arena ends at this field's last byte, arena.size % 4 == rem
            low = (rem - ln) % 4
            if ph % 4 != low:
                assert want is None or want[row] < 0, "the requested phase contradicts arena.size % 4"
                ph = (ph & ~3) | low
        off = pos + (ph - pos) % s.mod
        placed.append((s, row, off, ln))
        pos = off + ln + 1        # one poison byte at least behind every field
    s, row, off, ln = placed[-1]
    arena = np.full(off + ln, poison, np.uint8)
    for s, row, off, ln in placed:
        o = int(s.tab[s.off][row])
        assert o + ln <= src.size, f"{s.kind} {row} lies outside the source arena"
        arena[off:off + ln] = src[o:o + ln]
        s.tab[s.off][row] = off
    assert arena.size % 4 == rem
    return arena


# ----------------------------------------------------------------------------- signatures
def _batch_groups(keys, items):
    return [[_Spec("key", keys, "off", keys["len"])],
            [_Spec("sig", items, "sig_off", items["sig_len"]), _Spec("msg", items, "msg_off", items["msg_len"])]]


def batch_fields(b):
    return _fields(_batch_groups(b.keys, b.items))


def relayout_batch(batch, seed, lead=0, poison=0xFF, rem=1, last="msg"):
    """``Batch`` with keys, signatures and messages moved (``last``: "msg", "sig" or "key"; with
    "key" the keys sit behind the items). Items stay in table order, (sig, msg) adjacent per item."""
    keys, items = batch.keys.copy(), batch.items.copy()
    arena = _relayout(batch.arena, _batch_groups(keys, items), last, seed, lead, poison, rem)
    return B.Batch(keys, items, arena)


# ----------------------------------------------------------------------------- hashing spans
def spans_fields(spans):
    return _fields([[_Spec("span", spans, "off", spans["len"])]])


def relayout_spans(msgs, seed, lead=0, poison=0xFF, rem=1, phases=None):
    """(SPAN_DTYPE table, arena) for cg_sha256_batch / cg_sha512_batch over ``msgs``; ``phases``:
    the byte phase (0..3) of each message, or -1 / None for a random one."""
    spans = np.zeros(len(msgs), B.SPAN_DTYPE)
    src, off = [], 0
    for i, m in enumerate(msgs):
        spans[i] = (off, len(m))
        src.append(bytes(m))
        off += len(m)
    src = np.frombuffer(b"".join(src), np.uint8)
    ph = None if phases is None else {"span": np.asarray(phases, np.int64)}
    arena = _relayout(src, [[_Spec("span", spans, "off", spans["len"])]], "span", seed, lead, poison, rem, ph)
    return spans, arena


# ----------------------------------------------------------------------------- transaction ids
def _tx_groups(txs, comps):
    return [[_Spec("salt", txs, "salt_off", 32)], [_Spec("comp", comps, "off", comps["len"], mod=64)]]


def tx_fields(txs, comps):
    return _fields(_tx_groups(txs, comps))


def relayout_tx(txs, comps, arena, seed, lead=0, poison=0xFF, rem=1, last="comp", comp_phase=None, salt_phase=None):
    """(txs, comps, arena) with every component (the salt blob among them) at a phase mod 64 and every
    32-byte salt at a phase mod 4; ``last``: "comp" or "salt". ``comp_phase`` / ``salt_phase``: a
    phase per row (-1: random)."""
    txs, comps = txs.copy(), comps.copy()
    ph = {}
    if comp_phase is not None:
        ph["comp"] = np.asarray(comp_phase, np.int64)
    if salt_phase is not None:
        ph["salt"] = np.asarray(salt_phase, np.int64)
    return txs, comps, _relayout(arena, _tx_groups(txs, comps), last, seed, lead, poison, rem, ph)


# ----------------------------------------------------------------------------- tear-offs
def _filtered_groups(ftxs, nodes, leaves):
    plain = (leaves["flags"] & (B.FLEAF_SALT | B.FLEAF_HASH)) == 0   # only these carry a nonce
    return [[_Spec("root", ftxs, "root_off", 32)],
            [_Spec("node", nodes, "hash_off", 32, mask=nodes["kind"] != B.PMT_NODE)],
            [_Spec("leaf", leaves, "off", leaves["len"]), _Spec("nonce", leaves, "nonce_off", 32, mask=plain)]]


def filtered_fields(ftxs, nodes, leaves):
    return _fields(_filtered_groups(ftxs, nodes, leaves))


def relayout_filtered(ftxs, nodes, leaves, arena, seed, lead=0, poison=0xFF, rem=1, last="nonce"):
    """(ftxs, nodes, leaves, arena) with leaf blobs, nonces, node hashes and roots moved; ``last``:
    "leaf", "nonce", "node" or "root"."""
    ftxs, nodes, leaves = ftxs.copy(), nodes.copy(), leaves.copy()
    arena = _relayout(arena, _filtered_groups(ftxs, nodes, leaves), last, seed, lead, poison, rem)
    return ftxs, nodes, leaves, arena


# ----------------------------------------------------------------------------- tx signatures
def _txsig_groups(keys, sigs, tmpls):
    return [[_Spec("key", keys, "off", keys["len"])],
            [_Spec("prefix", tmpls, "prefix_off", tmpls["prefix_len"]),
             _Spec("suffix", tmpls, "suffix_off", tmpls["suffix_len"])],
            [_Spec("sig", sigs, "sig_off", sigs["sig_len"])]]


def txsig_fields(tb):
    return _fields(_txsig_groups(tb.keys, tb.sigs, tb.tmpls))


def relayout_txsig(tb, seed, lead=0, poison=0xFF, rem=1, last="sig"):
    """``TxSigBatch`` with key, signature and template prefix / suffix bytes moved; ``last``: "sig",
    "key", "prefix" or "suffix". The ids are a table of their own and stay."""
    keys, sigs, tmpls = tb.keys.copy(), tb.sigs.copy(), tb.tmpls.copy()
    arena = _relayout(tb.arena, _txsig_groups(keys, sigs, tmpls), last, seed, lead, poison, rem)
    return B.TxSigBatch(keys, tb.ids, sigs, tmpls, arena)


# ----------------------------------------------------------------------------- checks
def same_content(old_fields, old_arena, new_fields, new_arena, poison=0xFF):
    """Every field read through the new tables is byte-equal to the original, and the byte behind it
    is ``poison`` or the arena's end. Raises AssertionError naming the first field that is not."""
    assert old_fields.keys() == new_fields.keys()
    for kind in old_fields:
        (oo, ol), (no, nl) = old_fields[kind], new_fields[kind]
        assert np.array_equal(ol, nl), f"{kind}: lengths changed"
        for a, b, ln in zip(oo.tolist(), no.tolist(), ol.tolist()):
            assert b + ln <= new_arena.size, f"{kind} at {b}+{ln} runs past the arena"
            assert np.array_equal(old_arena[a:a + ln], new_arena[b:b + ln]), f"{kind} at {a} -> {b}: bytes differ"
            assert b + ln == new_arena.size or new_arena[b + ln] == poison, f"{kind} at {b}+{ln}: no poison behind"


def layout_stats(fields, arena_size, mod=4):
    """Per kind: ``unaligned`` (share of fields whose offset is no multiple of 4), ``phases`` (the set
    of offsets mod ``mod``), ``ends`` (a non-empty field of the kind ends exactly at the arena's end)."""
    out = {}
    for kind, (off, ln) in fields.items():
        out[kind] = {"unaligned": float(np.mean(off % 4 != 0)) if off.size else 0.0,
                     "phases": set(np.unique(off % mod).tolist()),
                     "ends": bool(np.any((off + ln == arena_size) & (ln > 0)))}
    return out


# ----------------------------------------------------------------------------- inputs of the layout tests
# Shared by tests/test_layout_util.py (CPU: the repack alone satisfies every precondition) and
# tests/test_gpu_layout.py (GPU: the engine's answers do not depend on the layout).
REMS = (1, 2, 3)                 # arena.size % 4
SEEDS = (101, 202)
VERIFY_LASTS = ("msg", "sig", "key")
# small; SHA-512 padding edge behind the 64-byte R || A prefix (Ed25519); SHA-256 padding edge
# (ECDSA); SHA block edges; either side of ITEM_LONG_MIN (keyws.h); long
VERIFY_LENS = (1, 2, 3, 47, 48, 175, 176, 55, 56, 119, 120, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 5000)
WIDE_ED_USES, WIDE_EC_USES = 2400, 900   # the wide-table thresholds test_wide_tables_vs_c_oracle asserts
GOLDEN_SETS = ("ed25519.json", "ecdsa.json", "spki.json", "ref_certs.json")
_cache = {}


def verify_case():
    """The verify batch of test_gpu_layout (its section a): every length of VERIFY_LENS for each of the three schemes,
    the golden sets (SPKI, compressed, hybrid and malformed keys among them), and one key per scheme
    above the wide-table threshold; shuffled. Built once per process."""
    if "verify" not in _cache:
        import golden_io
        from tools.workload import wl
        parts = []
        for j, ln in enumerate(VERIFY_LENS):
            parts.append(wl.ed25519_batch(40, n_keys=5, msg_len=ln, corrupt_permille=200, seed=300 + j, nthreads=4)[0])
            for curve in (0, 1):
                parts.append(wl.ecdsa_batch(curve, 24, n_keys=3, msg_len=ln, corrupt_permille=200,
                                            seed=400 + 2 * j + curve, nthreads=4)[0])
        parts += [golden_io.sig_batch(golden_io.load(name))[0] for name in GOLDEN_SETS]
        parts.append(wl.ed25519_batch(WIDE_ED_USES, n_keys=1, msg_len=47, corrupt_permille=200, seed=501, nthreads=4)[0])
        for curve in (0, 1):
            parts.append(wl.ecdsa_batch(curve, WIDE_EC_USES, n_keys=1, msg_len=55, corrupt_permille=200,
                                        seed=502 + curve, nthreads=4)[0])
        _cache["verify"] = wl.concat(parts, shuffle_seed=599)[0]
    return _cache["verify"]


# SignableData template lengths (prefix, suffix): the 32-byte id across the SHA-512 block ends at
# M[64) and M[192) and across the SHA-256 block ends, both sides of the precomputed-schedule
# condition (a prefix covering M[64, 192)), the padding byte at each edge
TMPL_LENS = ((0, 0), (15, 0), (16, 1), (31, 3), (32, 2), (47, 0), (48, 0), (63, 9), (64, 0), (79, 1), (80, 0),
             (111, 0), (112, 5), (143, 0), (144, 0), (159, 7), (160, 0), (175, 0), (176, 1), (191, 3), (192, 0),
             (193, 2), (255, 0), (256, 4), (287, 0), (288, 1))


def txsig_case():
    """The tx-signature batch of test_gpu_layout (its section e): for every template of TMPL_LENS 60 Ed25519 and 30 + 30 ECDSA signatures over
    SignableData(id) = prefix || id || suffix, as a 4-aligned TxSigBatch (templates behind the
    generator's arena) for relayout_txsig to move. Returns (TxSigBatch, template index per item)."""
    if "txsig" not in _cache:
        from tools.workload import wl
        rng = np.random.default_rng(31)
        parts, tm = [], []
        for j, (pl, sl) in enumerate(TMPL_LENS):
            pre = rng.integers(0, 256, pl, dtype=np.uint8).tobytes()
            suf = rng.integers(0, 256, sl, dtype=np.uint8).tobytes()
            with wl.signable_mode(pre, suf, group=3, id_seed=j + 1):
                bs = [wl.ed25519_batch(60, n_keys=6, msg_len=pl + 32 + sl, corrupt_permille=150, seed=700 + j,
                                       nthreads=4)[0]]
                bs += [wl.ecdsa_batch(curve, 30, n_keys=3, msg_len=pl + 32 + sl, corrupt_permille=150,
                                      seed=800 + 2 * j + curve, nthreads=4)[0] for curve in (0, 1)]
            parts += bs
            tm += [j] * sum(b.n for b in bs)
        big, _ = wl.concat(parts)
        tm = np.array(tm)
        arena, off = [big.arena], big.arena.size
        tmpls = np.zeros(len(TMPL_LENS), B.TMPL_DTYPE)
        src = np.random.default_rng(31)   # the same template bytes, drawn in the same order
        for j, (pl, sl) in enumerate(TMPL_LENS):
            tmpls[j] = (off, off + pl, pl, sl)
            arena.append(src.integers(0, 256, pl, dtype=np.uint8))
            arena.append(src.integers(0, 256, sl, dtype=np.uint8))
            off += pl + sl
        arena = np.concatenate(arena)
        pl = np.array([TMPL_LENS[t][0] for t in tm])
        ids = arena[big.items["msg_off"].astype(np.int64)[:, None] + pl[:, None] + np.arange(32)]
        sigs = np.zeros(big.n, B.TXSIG_DTYPE)
        for f in ("sig_off", "sig_len", "key_idx"):
            sigs[f] = big.items[f]
        sigs["tx_idx"] = np.arange(big.n)
        sigs["tmpl"] = tm
        _cache["txsig"] = (B.TxSigBatch(big.keys, ids.reshape(-1), sigs, tmpls, arena), tm)
    return _cache["txsig"]


# component lengths of the transaction-id phase sweep: the one-block and two-block SHA-256 padding
# edges with (len + 32) and without (the salt leaf) the 32-byte nonce suffix
TX_SWEEP_LENS = (0, 1, 3, 4, 23, 24, 31, 32, 55, 56, 63, 64, 65, 87, 88, 119, 120)
# at or above 16 SHA-256 blocks: the capped class of k_tx_leaves holds lanes of different block counts
TX_CAPPED_LENS = (920, 951, 952, 960, 983, 984, 1016, 1024, 1500, 4097)
TX_LEAF_COUNTS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 130)


def tx_case():
    """The transactions of test_gpu_layout's section c as (list of (blobs, salt, salt_blob), component phase per component row of
    merkle.pack_transactions, salt phase per transaction): the phase sweep (a 3-leaf transaction per
    offset mod 64 and length of TX_SWEEP_LENS, the salt leaf's blob of that length too), 200
    transactions of TX_CAPPED_LENS components, and one transaction per leaf count."""
    if "tx" not in _cache:
        rng = np.random.default_rng(41)
        rb = lambda n: rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()  # noqa: E731
        txs, cph = [], []
        for ph in range(64):
            for ln in TX_SWEEP_LENS:
                txs.append(([rb(ln), rb(ln)], rb(32), rb(ln)))
                cph += [ph, 63 - ph, ph]
        for _ in range(200):
            n = int(rng.integers(3, 9))
            txs.append(([rb(rng.choice(TX_CAPPED_LENS)) for _ in range(n)], rb(32), rb(rng.choice(TX_CAPPED_LENS))))
            cph += [-1] * (n + 1)
        for n in TX_LEAF_COUNTS:
            salt = rb(32)
            txs.append(([rb(rng.integers(0, 200)) for _ in range(n - 1)], salt, b"\x01" + salt))
            cph += [-1] * n
        sph = np.arange(len(txs)) % 4
        sph[-1] = -1   # free to end the arena (last="salt")
        _cache["tx"] = (txs, np.array(cph), sph)
    return _cache["tx"]
