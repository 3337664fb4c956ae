"""The host tx-signature path's policy (corda_amd/csrc/txsig_plan.h) on the CPU, through
tests/native/txsig_plan_test.cpp: chunk bounds, key-use counts (exact, block-sampled, the estimate),
byte extents, the resident-interval set and the packed form's fix-up. Each rule is restated here in
numpy, from the text cg_verify_tx_signatures had before the policy moved to the header, and whole
output arrays are compared. The policy decides which keys get which table mode and which bytes reach
the device when; on the GPU it is reachable only through calls of 2^16 signatures and more."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "libtxsigplantest.so")
U64 = ctypes.c_uint64
U32 = ctypes.c_uint32
VP = ctypes.c_void_p
U64_MAX = 2**64 - 1

TXSIG = np.dtype([("sig_off", "<u8"), ("tx_idx", "<u4"), ("key_idx", "<u4"), ("sig_len", "<u2"), ("tmpl", "<u2"),
                  ("reserved", "<u4")])
TXSIG12 = np.dtype([("tx_idx", "<u4"), ("key_idx", "<u4"), ("sig_len", "<u2"), ("tmpl", "<u2")])
KEY = np.dtype([("off", "<u8"), ("len", "<u2"), ("scheme", "u1"), ("fmt", "u1"), ("reserved", "<u4")])
TMPL = np.dtype([("prefix_off", "<u8"), ("suffix_off", "<u8"), ("prefix_len", "<u4"), ("suffix_len", "<u4")])
ED25519, SECP256K1, SECP256R1 = 4, 2, 3  # include/cordagpu.h scheme ids


def _lib():
    csrc = os.path.join(HERE, "..", "corda_amd", "csrc")
    deps = [os.path.join(HERE, "native", "txsig_plan_test.cpp"), os.path.join(csrc, "txsig_plan.h"),
            os.path.join(csrc, "host_pool.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", SO, deps[0]])
    L = ctypes.CDLL(SO)
    L.tp_bounds.argtypes = [U64, U64, ctypes.c_int, U64, VP, U64, VP]
    L.tp_bounds.restype = U64
    L.tp_equal_bounds.argtypes = [U64, U64, VP, U64]
    L.tp_equal_bounds.restype = U64
    for f, n in ((L.tp_sample_override, 1), (L.tp_sample_block, 1)):
        f.argtypes = [U32] * n
        f.restype = U32
    L.tp_sample_rate.argtypes = [U32, U64, U32]
    L.tp_sample_rate.restype = U32
    L.tp_estimate.argtypes = [U64, U32, U64, U64]
    L.tp_estimate.restype = U32
    L.tp_hot_floor.argtypes = [U32, U32, U32]
    L.tp_hot_floor.restype = U64
    L.tp_count_exact.argtypes = [ctypes.c_int, VP, U64, U32, U64, VP]
    L.tp_count_sampled.argtypes = [ctypes.c_int, VP, U64, U32, U64, U32, U32, VP]
    L.tp_key_use_counts.argtypes = [ctypes.c_int, VP, U64, VP, U32, U64, U32, U32, U32, U32, VP]
    L.tp_extent_add.argtypes = [VP, U64, U64, U64]
    L.tp_extent_empty.argtypes = [U64, U64]
    L.tp_resident_new.restype = VP
    L.tp_resident_free.argtypes = [VP]
    L.tp_resident_missing.argtypes = [VP, U64, U64, VP, U64]
    L.tp_resident_missing.restype = U64
    L.tp_resident_have.argtypes = [VP, VP, U64]
    L.tp_resident_have.restype = U64
    L.tp_scan_chunk.argtypes = [ctypes.c_int, VP, U64, U64, U64, U64, U64, VP]
    L.tp_head_extent.argtypes = [VP, U32, VP, U32, U64, VP]
    L.tp_fixup.argtypes = [VP, U32, VP, U32, U64, VP, VP]
    return L


def _table(dtype, key_idx, tx_idx=None, sig_off=None, sig_len=None):
    t = np.zeros(len(key_idx), dtype=dtype)
    t["key_idx"] = key_idx
    if tx_idx is not None:
        t["tx_idx"] = tx_idx
    if sig_len is not None:
        t["sig_len"] = sig_len
    if sig_off is not None and dtype is TXSIG:
        t["sig_off"] = sig_off
    return t


# ---------------------------------------------------------------- chunk bounds
def _equal_chunk(chunk, n):
    if n <= chunk:
        return n or 1
    k = -(-n // chunk)
    return -(-n // k)


def _bounds_model(n, chunk, chunk_set, first_div):
    per = _equal_chunk(chunk, n)
    if not chunk_set and n >= 3 * 2**20:
        per = min(per, -(-n // 3))
    k0 = -(-n // per)
    if first_div > 1 and k0 > 1:
        f0 = n // first_div
        return [0, f0] + [f0 + (n - f0) * k // k0 for k in range(1, k0 + 1)]
    return [n if k == k0 else k * per for k in range(k0 + 1)]


def _bounds(n, chunk, chunk_set, first_div):
    out = np.zeros(64, dtype=np.uint64)
    largest = U64(0)
    m = _lib().tp_bounds(n, chunk, int(chunk_set), first_div, out.ctypes.data, len(out), ctypes.byref(largest))
    b = [int(x) for x in out[:m]]
    assert largest.value == max(b[k + 1] - b[k] for k in range(len(b) - 1))
    return b


DEFAULT_CHUNK = 8 << 20


@pytest.mark.parametrize("n, chunk, chunk_set, first_div, want", [
    (1, DEFAULT_CHUNK, False, 6, [0, 1]),
    (100_000, DEFAULT_CHUNK, False, 6, [0, 100_000]),                       # below the chunk size: one chunk
    (150_000, 40_001, True, 6, [0, 25_000, 56_250, 87_500, 118_750, 150_000]),  # 1/6, then as many as the equal split
    (150_000, 40_001, True, 0, [0, 37_500, 75_000, 112_500, 150_000]),      # equal chunks
    (150_000, 40_001, True, 1, [0, 37_500, 75_000, 112_500, 150_000]),
    # fewer signatures than the divisor in more than one chunk: the first chunk is EMPTY (n // 6 = 0).
    # That is what the library has always done; kept as it is, and written down here as what it is.
    (3, 1, True, 6, [0, 0, 1, 2, 3]),
    # from 3 * 2^20 signatures a caller that did not set chunk_items gets at least 3 chunks + the first
    (3 << 20, DEFAULT_CHUNK, False, 6, [0, 524_288, 1_398_101, 2_271_914, 3_145_728]),
    (3 << 20, DEFAULT_CHUNK, True, 6, [0, 3 << 20]),
    ((3 << 20) - 1, DEFAULT_CHUNK, False, 6, [0, (3 << 20) - 1]),
])
def test_chunk_bounds(n, chunk, chunk_set, first_div, want):
    b = _bounds(n, chunk, chunk_set, first_div)
    assert b == want == _bounds_model(n, chunk, chunk_set, first_div)
    assert b[0] == 0 and b[-1] == n
    assert all(b[k] <= b[k + 1] for k in range(len(b) - 1))
    if len(b) > 2 and first_div > 1:
        assert b[1] == n // first_div


def test_chunk_bounds_match_the_model_over_a_sweep():
    rng = np.random.default_rng(7)
    for _ in range(300):
        n = int(rng.integers(1, 5 << 20))
        chunk = int(rng.choice([1 << 10, 40_001, 1 << 20, DEFAULT_CHUNK]))
        if n // chunk > 60:
            chunk = DEFAULT_CHUNK
        for chunk_set in (False, True):
            for fd in (0, 1, 2, 6, 8):
                assert _bounds(n, chunk, chunk_set, fd) == _bounds_model(n, chunk, chunk_set, fd)


@pytest.mark.parametrize("per", [1, 256, 40_001])
def test_equal_bounds(per):
    """equal_bounds(n, per) = {0, per, 2 per, ..., n}: the bounds and the chunk sizes equal the closed forms
    launch_chunked used before it took a bounds vector (chunk k = per items from k per, the last one the rest)."""
    for n in sorted({per - 1, per, per + 1, 2 * per, 2 * per + 1, 3 * per - 1, 1} - {0}):
        out = np.zeros(8, dtype=np.uint64)
        m = _lib().tp_equal_bounds(n, per, out.ctypes.data, len(out))
        b = [int(x) for x in out[:m]]
        nch = -(-n // per)
        assert b[0] == 0 and b[-1] == n and len(b) == nch + 1, (n, per, b)
        assert all(b[k + 1] - b[k] == per for k in range(nch - 1)) and 0 < b[-1] - b[-2] <= per, (n, per, b)
        for k in range(nch):
            assert b[k] == k * per and b[k + 1] - b[k] == min(per, n - k * per), (n, per, k, b)


# ---------------------------------------------------------------- key-use counts
def _exact(t, n_keys, nt):
    out = np.full(max(n_keys, 1), 0xdeadbeef, dtype=np.uint32)
    _lib().tp_count_exact(int(t.dtype == TXSIG12), t.ctypes.data, len(t), n_keys, nt, out.ctypes.data)
    return out


def _bincount(key_idx, n_keys):
    k = np.asarray(key_idx, dtype=np.int64)
    return np.bincount(k[k < n_keys], minlength=max(n_keys, 1)).astype(np.uint32)


def _exact_cases():
    rng = np.random.default_rng(11)
    n = 16 * 400  # every thread's slice holds 400 records at nt = 16
    wraps = rng.integers(0, 300, n)
    wraps[wraps == 7] = 8
    wraps[wraps == 9] = 10
    wraps[:256] = 7          # exactly 256 uses inside thread 0's slice at every nt: the byte counter wraps to 0
    wraps[1000:1700] = 9     # 700 uses: two wraps at nt = 1, spread over slices at nt = 16
    stray = rng.integers(0, 340, n)  # indices >= n_keys are ignored
    stray[5] = 0xffffffff
    return [("one_key", np.zeros(1000, dtype=np.int64), 1), ("wraps", wraps, 300), ("stray", stray, 300),
            ("no_keys", rng.integers(0, 5, 100), 0), ("no_sigs", np.zeros(0, dtype=np.int64), 300)]


@pytest.mark.parametrize("dtype", [TXSIG, TXSIG12], ids=["txsig24", "txsig12"])
@pytest.mark.parametrize("name, key_idx, n_keys", _exact_cases(), ids=[c[0] for c in _exact_cases()])
def test_exact_counts_equal_bincount_at_every_thread_count(dtype, name, key_idx, n_keys):
    t = _table(dtype, key_idx)
    want = _bincount(key_idx, n_keys)
    if name == "wraps":
        assert want[7] == 256 and want[9] == 700
    for nt in (1, 3, 16):
        assert np.array_equal(_exact(t, n_keys, nt), want), nt


def _sampled_model(key_idx, n_keys, S, B):
    """B consecutive records of every S * B, the block at a hashed position within its group."""
    n = len(key_idx)
    ng = -(-n // (S * B))
    g = np.arange(ng, dtype=np.uint64)
    h = (((g * np.uint64(0x9E3779B1)) & np.uint64(0xffffffff)) >> np.uint64(24)) % np.uint64(S)
    i0 = (g * np.uint64(S) + h) * np.uint64(B)
    idx = (i0[:, None] + np.arange(B, dtype=np.uint64)[None, :]).ravel()
    idx = idx[idx < n].astype(np.int64)
    return _bincount(np.asarray(key_idx)[idx], n_keys)


def _sampled(t, n_keys, nt, S, B):
    out = np.full(max(n_keys, 1), 0xdeadbeef, dtype=np.uint32)
    _lib().tp_count_sampled(int(t.dtype == TXSIG12), t.ctypes.data, len(t), n_keys, nt, S, B, out.ctypes.data)
    return out


@pytest.mark.parametrize("dtype", [TXSIG, TXSIG12], ids=["txsig24", "txsig12"])
@pytest.mark.parametrize("n", [2048, 2048 + 37])
def test_sampled_counts_follow_the_hashed_blocks(dtype, n):
    rng = np.random.default_rng(n)
    key_idx = rng.integers(0, 5, n)  # 4 keys and a stray index
    t = _table(dtype, key_idx)
    L = _lib()
    assert L.tp_sample_rate(0, n, 4) == 32 and L.tp_sample_block(8) == 8  # what the library picks for this call
    for S in (8, 32):
        for B in (1, 8, 64):
            want = _sampled_model(key_idx, 4, S, B)
            assert 0 < want.sum() <= -(-n // (S * B)) * B
            for nt in (1, 3, 16):
                assert np.array_equal(_sampled(t, 4, nt, S, B), want), (S, B, nt)


def test_sample_rate_and_overrides():
    L = _lib()
    assert L.tp_sample_rate(0, 256 * 4, 4) == 32      # keys average 256 uses: 1 in 32
    assert L.tp_sample_rate(0, 256 * 4 - 1, 4) == 1   # below: exact
    assert L.tp_sample_rate(0, 256, 0) == 32          # no keys counts as one
    assert L.tp_sample_rate(8, 10, 1000) == 8         # CG_TXSIG_SAMPLE overrides
    assert [L.tp_sample_override(x) for x in (0, 1, 8, 12, 32, 33)] == [0, 1, 8, 0, 32, 0]  # powers of two only
    assert [L.tp_sample_block(x) for x in (0, 1, 8, 64, 65)] == [8, 1, 8, 64, 8]


def _estimate_model(c, S, wmin, floor_hot):
    up = S * (c + 3 * math.ceil(math.sqrt(c)) + 1)
    e = (up if up >= wmin else S * c) if c else min(S, 8)
    if c and e < floor_hot:
        e = floor_hot
    return min(e, 0xfffffff0)


@pytest.mark.parametrize("c, S, wmin, floor_hot, want", [
    (0, 4, 1536, 0, 4),            # unsampled: min(S, 8), its row-0 table
    (0, 32, 1536, 0, 8),
    (0, 32, 1536, 1536, 8),        # the hot floor lifts sampled keys only
    (28, 32, 1536, 0, 896),        # S (c + 3 ceil(sqrt c) + 1) = 1504 stays below the wide threshold: plain S c
    (29, 32, 1536, 0, 1536),       # ... = 1536 reaches it: the raised estimate
    (1, 32, 1536, 1536, 1536),     # hot call (S = 32): a sampled key counts at least the wide threshold
    (1, 8, 1536, 0, 8),            # not a hot call: no floor
    (100, 32, 1536, 1536, 4192),   # above the floor: unchanged
    (1 << 32, 32, 1536, 0, 0xfffffff0),   # saturates
    ((1 << 27) - 1, 32, 1 << 40, 0, 0xffffffe0),  # the largest plain estimate below the cap
    (1 << 27, 32, 1 << 40, 0, 0xfffffff0),
])
def test_estimate(c, S, wmin, floor_hot, want):
    assert _lib().tp_estimate(c, S, wmin, floor_hot) == want == _estimate_model(c, S, wmin, floor_hot)


def test_estimate_matches_the_model_over_a_sweep_and_hot_floor():
    L = _lib()
    for S in (2, 8, 32, 64):
        for wmin in (32, 1024, 1536):
            for floor_hot in (0, 1536):
                for c in list(range(0, 200)) + [1000, 10**6, 10**9]:
                    assert L.tp_estimate(c, S, wmin, floor_hot) == _estimate_model(c, S, wmin, floor_hot)
    assert L.tp_hot_floor(32, 1536, 1024) == 1536 and L.tp_hot_floor(32, 100, 1024) == 1024
    assert L.tp_hot_floor(64, 1536, 1024) == 1536
    assert L.tp_hot_floor(16, 1536, 1024) == 0 and L.tp_hot_floor(1, 1536, 1024) == 0


def _uses(t, keys, nt, S, B, min_ed, min_ec):
    out = np.full(max(len(keys), 1), 0xdeadbeef, dtype=np.uint32)
    _lib().tp_key_use_counts(int(t.dtype == TXSIG12), t.ctypes.data, len(t), keys.ctypes.data, len(keys), nt, S, B,
                             min_ed, min_ec, out.ctypes.data)
    return out


@pytest.mark.parametrize("dtype", [TXSIG, TXSIG12], ids=["txsig24", "txsig12"])
def test_key_use_counts_pick_the_threshold_by_scheme(dtype):
    keys = np.zeros(3, dtype=KEY)
    keys["scheme"] = [ED25519, SECP256R1, SECP256K1]
    # 240 records of one key at 1 in 8, blocks of 1: 30 sampled; 8 (30 + 18 + 1) = 392
    for k, want in ((0, 240), (1, 392), (2, 392)):   # Ed25519 threshold 400 not reached, ECDSA's 300 reached
        t = _table(dtype, np.full(240, k))
        got = _uses(t, keys, 3, 8, 1, 400, 300)
        assert got[k] == want and all(got[j] == 8 for j in range(3) if j != k)
    # whole arrays against the model, hot call (S = 32: floor) and not, every thread count; S = 1 is exact
    rng = np.random.default_rng(5)
    key_idx = rng.integers(0, 4, 4096 + 37)
    t = _table(dtype, key_idx)
    for S, B in ((32, 8), (8, 8), (8, 1)):
        floor_hot = 1536 if S >= 32 else 0
        sampled = _sampled_model(key_idx, 3, S, B)
        want = [_estimate_model(int(sampled[k]), S, 1536 if k == 0 else 1024, floor_hot) for k in range(3)]
        for nt in (1, 3, 16):
            assert list(_uses(t, keys, nt, S, B, 1536, 1024)) == want, (S, B, nt)
    for nt in (1, 3, 16):
        assert np.array_equal(_uses(t, keys, nt, 1, 8, 1536, 1024), _bincount(key_idx, 3))


# ---------------------------------------------------------------- extents and resident intervals
def _add(x, off, length, arena_len):
    a = np.array(x, dtype=np.uint64)
    _lib().tp_extent_add(a.ctypes.data, off, length, arena_len)
    return int(a[0]), int(a[1])


def test_extent_add_clips_to_the_arena():
    empty = (U64_MAX, 0)
    L = _lib()
    assert L.tp_extent_empty(*empty) == 1
    assert _add(empty, 101, 4, 100) == empty                 # off past the arena: ignored
    assert _add(empty, 10, 20, 100) == (10, 30)
    assert _add((10, 30), 90, 20, 100) == (10, 100)          # a length running past the arena is clipped
    assert _add(empty, 90, U64_MAX, 100) == (90, 100)        # no wrap of off + len
    x = _add(empty, 100, 0, 100)                             # the arena's end with length 0: in range, no bytes
    assert x == (100, 100) and L.tp_extent_empty(*x) == 1
    assert _add((10, 30), 5, 1, 100) == (5, 30) and L.tp_extent_empty(5, 30) == 0


class _Resident:
    def __init__(self):
        self.L = _lib()
        self.h = self.L.tp_resident_new()

    def missing(self, lo, hi):
        out = np.zeros(2 * 64, dtype=np.uint64)
        n = self.L.tp_resident_missing(self.h, lo, hi, out.ctypes.data, 64)
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]

    def have(self):
        out = np.zeros(2 * 64, dtype=np.uint64)
        n = self.L.tp_resident_have(self.h, out.ctypes.data, 64)
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]

    def __del__(self):
        self.L.tp_resident_free(self.h)


@pytest.mark.parametrize("first, second, gaps, have", [
    ((10, 20), (30, 40), [(30, 40)], [(10, 20), (30, 40)]),   # disjoint
    ((30, 40), (10, 20), [(10, 20)], [(10, 20), (30, 40)]),
    ((10, 40), (20, 30), [], [(10, 40)]),                     # nested: fully resident, no gaps
    ((20, 30), (10, 40), [(10, 20), (30, 40)], [(10, 40)]),
    ((10, 20), (20, 30), [(20, 30)], [(10, 30)]),             # abutting: merged
    ((20, 30), (10, 20), [(10, 20)], [(10, 30)]),
    ((10, 25), (20, 30), [(25, 30)], [(10, 30)]),             # overlapping
    ((20, 30), (10, 25), [(10, 20)], [(10, 30)]),
    ((10, 20), (10, 20), [], [(10, 20)]),                     # the same extent again
    ((10, 20), (15, 15), [], [(10, 20)]),                     # an empty extent: nothing, nothing recorded
    ((10, 20), (U64_MAX, 0), [], [(10, 20)]),
])
def test_resident_intervals(first, second, gaps, have):
    r = _Resident()
    assert r.missing(*first) == [first] and r.have() == [first]
    assert r.missing(*second) == gaps
    assert r.have() == have


def test_resident_gaps_against_a_byte_mask():
    rng = np.random.default_rng(3)

    def runs(mask, lo, val):
        edges = np.flatnonzero(np.diff(np.concatenate(([0], (mask == val).astype(np.int8), [0]))))
        return [(lo + int(a), lo + int(b)) for a, b in zip(edges[::2], edges[1::2])]

    for _ in range(40):
        r = _Resident()
        mask = np.zeros(256, dtype=bool)
        for _ in range(12):
            lo = int(rng.integers(0, 250))
            hi = min(256, lo + int(rng.integers(0, 40)))
            assert r.missing(lo, hi) == runs(mask[lo:hi], lo, False)
            mask[lo:hi] = True
            assert r.have() == runs(mask, 0, True)


def _scan(t, f, e, n_ids, arena_len, nt):
    out = np.zeros(5, dtype=np.uint64)
    _lib().tp_scan_chunk(int(t.dtype == TXSIG12), t.ctypes.data, f, e, n_ids, arena_len, nt, out.ctypes.data)
    return [int(x) for x in out]


@pytest.mark.parametrize("n, f, e", [(5000, 0, 5000), (5000, 1234, 4321), (70_000, 0, 70_000), (70_000, 3, 69_999)],
                         ids=["one_part", "one_part_slice", "threaded", "threaded_slice"])
def test_chunk_extent_scan(n, f, e):
    rng = np.random.default_rng(n + f)
    arena_len, n_ids = 1_000_000, 900
    sig_off = rng.integers(1000, arena_len - 200, n).astype(np.uint64)
    sig_len = rng.integers(0, 140, n)
    tx_idx = rng.integers(100, 1000, n)  # some >= n_ids: ignored
    sig_off[f + 5] = arena_len + 1       # outside the arena: ignored
    sig_off[f + 9] = arena_len - 10      # runs past the arena's end: clipped
    sig_len[f + 9] = 64
    for dtype in (TXSIG, TXSIG12):
        t = _table(dtype, np.zeros(n, dtype=np.int64), tx_idx=tx_idx, sig_off=sig_off, sig_len=sig_len)
        tx = tx_idx[f:e][tx_idx[f:e] < n_ids]
        ids = [32 * int(tx.min()), 32 * int(tx.max()) + 32]
        if dtype is TXSIG:
            o, l = sig_off[f:e].astype(np.int64), sig_len[f:e]
            ok = o <= arena_len
            want = [int(o[ok].min()), int(np.minimum(o[ok] + l[ok], arena_len).max())] + ids + [0]
            assert want[1] == arena_len
        else:  # the 12-byte table: no offsets, the stream bytes of the slice
            want = [U64_MAX, 0] + ids + [int(((sig_len[f:e] + 3) & ~3).sum())]
        for nt in (1, 3, 16):  # below 2^16 records the scan is one part whatever nt
            assert _scan(t, f, e, n_ids, arena_len, nt) == want, (dtype, nt)
    assert _scan(_table(TXSIG, [0]), 0, 0, 10, 100, 3) == [U64_MAX, 0, U64_MAX, 0, 0]  # an empty chunk


def test_head_extent_and_packed_fixup():
    L = _lib()
    caller_len = 100
    keys = np.zeros(5, dtype=KEY)
    keys["off"] = [10, 100, 99, 101, 68]
    keys["len"] = [32, 0, 2, 0, 32]   # in range; the end with length 0 (in range); one byte past; off past; exact end
    tmpls = np.zeros(3, dtype=TMPL)
    tmpls["prefix_off"] = [0, 4, 200]
    tmpls["prefix_len"] = [4, 4, 4]
    tmpls["suffix_off"] = [50, 90, 0]
    tmpls["suffix_len"] = [8, 11, 0]  # in range; the suffix alone is outside; the prefix is outside
    kout, tout = np.zeros(5, dtype=KEY), np.zeros(3, dtype=TMPL)
    assert L.tp_fixup(keys.ctypes.data, 5, tmpls.ctypes.data, 3, caller_len, kout.ctypes.data, tout.ctypes.data) == 3
    kwant, twant = keys.copy(), tmpls.copy()
    kwant["off"][[2, 3]] = U64_MAX
    twant["prefix_off"][[1, 2]] = U64_MAX  # the template is switched off by its prefix offset; the rest is untouched
    assert np.array_equal(kout, kwant) and np.array_equal(tout, twant)
    # nothing out of range: no corrected copy is made
    assert L.tp_fixup(keys.ctypes.data, 2, tmpls.ctypes.data, 1, caller_len, kout.ctypes.data, tout.ctypes.data) == 0
    assert L.tp_fixup(keys.ctypes.data, 3, tmpls.ctypes.data, 1, caller_len, kout.ctypes.data, tout.ctypes.data) == 1
    assert L.tp_fixup(keys.ctypes.data, 0, tmpls.ctypes.data, 2, caller_len, kout.ctypes.data, tout.ctypes.data) == 2
    # the header's extent: the key and template bytes inside the arena (a run past the end is clipped)
    out = np.zeros(2, dtype=np.uint64)
    L.tp_head_extent(keys.ctypes.data, 5, tmpls.ctypes.data, 3, caller_len, out.ctypes.data)
    assert [int(x) for x in out] == [0, 100]
    L.tp_head_extent(keys.ctypes.data, 1, tmpls.ctypes.data, 0, caller_len, out.ctypes.data)
    assert [int(x) for x in out] == [10, 42]
