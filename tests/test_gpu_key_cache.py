"""GPU tests of the per-context wide-table cache (corda_amd/csrc/key_cache.h, verify.hip k_kc_*).

A context keeps the wide tables of its hot keys between calls, keyed by scheme and key bytes; a call
builds only those it does not find. Every case compares each call's verdicts with the C oracle and
reads the last call's counters (Engine.key_cache_stats: hits, built, evicted, fell_back per pool,
[0] Ed25519, [1] ECDSA). The batches follow tests/test_gpu_tables.py::wide_batch: hot keys of every
scheme, each at twice its wide threshold or more (1,536 Ed25519 / 512 ECDSA items), so that the
sampled use counts cannot put a hot key in another table mode, and a tail of cold keys."""
import numpy as np
import pytest

from corda_amd import batch as B
from oracle import c_oracle

pytestmark = pytest.mark.gpu

ED, R1, K1 = 4, 3, 2  # include/cordagpu.h scheme ids
ED_KEYS, R1_KEYS, K1_KEYS = 8, 6, 5


def _make(seed):
    from tools.workload import wl
    parts = [wl.ed25519_batch(26000, n_keys=ED_KEYS, msg_len=270, corrupt_permille=120, seed=seed, bad_key_every=5,
                              nthreads=16)[0],
             wl.ecdsa_batch(0, 9000, n_keys=R1_KEYS, msg_len=270, corrupt_permille=120, seed=seed + 1, nthreads=16)[0],
             wl.ecdsa_batch(1, 6000, n_keys=K1_KEYS, msg_len=270, corrupt_permille=120, seed=seed + 2, nthreads=16)[0],
             wl.ed25519_batch(1500, n_keys=300, msg_len=120, corrupt_permille=120, seed=seed + 3, nthreads=16)[0],
             wl.ecdsa_batch(0, 1000, n_keys=60, msg_len=90, corrupt_permille=120, seed=seed + 4, nthreads=16)[0]]
    b, _ = wl.concat(parts, shuffle_seed=seed + 5)
    uses = np.bincount(b.items["key_idx"], minlength=len(b.keys))
    ed = b.keys["scheme"] == ED
    hot = np.where(ed, uses >= 1536, uses >= 512)
    assert hot[ed].sum() == ED_KEYS and hot[~ed].sum() == R1_KEYS + K1_KEYS
    assert (uses[hot & ed] >= 2 * 1536).all() and (uses[hot & ~ed] >= 2 * 512).all()
    assert (uses[~hot] < 100).all()
    return b


def _ref(b, mode=B.MODE_DOVERIFY):
    return c_oracle.verify_batch(b, mode, 16)


@pytest.fixture(scope="module")
def batch_a():
    b = _make(701)
    return b, _ref(b)


@pytest.fixture(scope="module")
def batch_b():
    b = _make(801)  # the same layout, other keys: the same key_idx carries other bytes
    return b, _ref(b)


def _open(**kw):
    """A context of its own for each case. The tests also take the session's `engine`: while it is open the
    process holds the constant tables, so opening another context does not build them again."""
    from corda_amd.engine import Engine
    return Engine(0, **kw)


def _call(eng, b, ref, what, mode=B.MODE_DOVERIFY):
    st = eng.verify(b, mode)
    assert np.array_equal(st, ref), f"{what}: {np.count_nonzero(st != ref)} verdicts differ from the oracle"
    return eng.key_cache_stats()


def _total(x):
    return x[0] + x[1]


def _repeat_and_swap(eng, batch_a, batch_b):
    """Cases 1 and 2: A three times, then B, A, B. The pool holds both key sets, and empty slots are
    claimed before valid ones, so after its first call neither batch builds anything again."""
    (a, ra), (b, rb) = batch_a, batch_b
    s1 = _call(eng, a, ra, "A cold")
    assert s1["enabled"] and s1["slots"] > 0
    assert s1["built"][0] > 0 and s1["built"][1] > 0 and s1["hits"] == (0, 0), s1
    for k in (2, 3):
        s = _call(eng, a, ra, f"A call {k}")
        assert s["built"] == (0, 0) and s["hits"] == s1["built"] and s["evicted"] == (0, 0), (k, s, s1)
    sb = _call(eng, b, rb, "B cold")
    assert sb["hits"] == (0, 0) and sb["built"][0] > 0 and sb["built"][1] > 0, sb
    s = _call(eng, a, ra, "A after B")
    assert s["built"] == (0, 0) and s["hits"] == s1["built"], s
    s = _call(eng, b, rb, "B after A")
    assert s["built"] == (0, 0) and s["hits"] == sb["built"], s


def test_repeat_then_same_indices_other_keys(engine, batch_a, batch_b):
    with _open() as eng:
        _repeat_and_swap(eng, batch_a, batch_b)


def test_identity_is_the_bytes_not_the_index(engine, batch_a):
    a, ra = batch_a
    perm = np.random.default_rng(9).permutation(len(a.keys))  # new row r holds old row perm[r]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    items = a.items.copy()
    items["key_idx"] = inv[items["key_idx"]]
    p = B.Batch(np.ascontiguousarray(a.keys[perm]), items, a.arena)
    rp = _ref(p)
    assert np.array_equal(rp, ra)  # the same signatures under the same keys
    with _open() as eng:
        s1 = _call(eng, a, ra, "A")
        s = _call(eng, p, rp, "A with its key table permuted")
        assert s["built"] == (0, 0) and s["hits"] == s1["built"], (s, s1)


def test_eviction(engine, batch_a, batch_b, monkeypatch):
    (a, ra), (b, rb) = batch_a, batch_b
    monkeypatch.setenv("CG_TEST_WIDE_SLOTS", str(ED_KEYS))  # read at cg_open
    with _open() as eng:
        s = _call(eng, a, ra, "A")
        assert s["slots"] == ED_KEYS and s["built"][0] > 0
        # the ECDSA pool has ED_KEYS slots for R1_KEYS + K1_KEYS hot keys: the rest take full tables
        assert s["fell_back"][1] == R1_KEYS + K1_KEYS - ED_KEYS
        s = _call(eng, b, rb, "B")
        assert s["hits"] == (0, 0) and s["evicted"][0] > 0 and s["evicted"][1] > 0, s
        s = _call(eng, a, ra, "A again")
        assert s["built"][0] > 0 and s["evicted"][0] > 0, s
    monkeypatch.setenv("CG_TEST_WIDE_SLOTS", "3")
    with _open() as eng:
        s = _call(eng, a, ra, "A with 3 slots")
        assert s["slots"] == 3 and s["fell_back"] == (ED_KEYS - 3, R1_KEYS + K1_KEYS - 3), s
        s = _call(eng, b, rb, "B with 3 slots")
        assert s["hits"] == (0, 0), s
        _call(eng, a, ra, "A again with 3 slots")


def test_colliding_keys(engine, batch_a, batch_b, monkeypatch):
    monkeypatch.setenv("CG_TEST_KEY_CACHE_BITS", "1")  # two home entries for every key
    with _open() as eng:
        _repeat_and_swap(eng, batch_a, batch_b)


def test_duplicate_key_rows(engine, batch_a):
    a, _ = batch_a
    uses = np.bincount(a.items["key_idx"], minlength=len(a.keys))
    hot = np.flatnonzero((a.keys["scheme"] == ED) & (uses >= 1536))
    h0, h1 = int(hot[1]), int(hot[2])
    # a new key row with h0's bytes, copied to the arena's end; it takes over every item of h1
    k = a.keys[h0].copy()
    raw = a.arena[int(k["off"]):int(k["off"]) + int(k["len"])]
    pad = (-a.arena.size) % 4
    arena = np.concatenate([a.arena, np.zeros(pad + 1, np.uint8), raw, np.zeros(64, np.uint8)])
    k["off"] = a.arena.size + pad + 1  # an odd offset: other alignment, same bytes
    keys = np.concatenate([a.keys, np.array([k], dtype=a.keys.dtype)])
    items = a.items.copy()
    items["key_idx"][items["key_idx"] == h1] = len(keys) - 1
    d = B.Batch(keys, items, arena)
    rd = _ref(d)
    with _open() as eng:
        s1 = _call(eng, d, rd, "duplicate rows, cold")
        assert s1["hits"] == (0, 0) and s1["built"][0] > 0
        s = _call(eng, d, rd, "duplicate rows, warm")
        assert s["built"] == (0, 0) and s["hits"] == s1["built"], (s, s1)


def test_other_entry_points(engine, batch_a):
    from corda_amd import signable
    from tools.workload import wl
    pool, _, schemes = wl.notary_pool(1 << 14, ed_keys=8, ec_keys=6, seed=616, nthreads=16, sig_group=4)
    pre, _ = signable.template(1, 4)
    ids, id_idx = wl.pool_ids(pool, len(pre))
    idx = np.random.default_rng(617).integers(0, pool.n, 60000)
    pb = wl.tx_sig_stream(pool, schemes, idx, ids, id_idx, nthreads=16).packed()
    ref = _ref(pool)[idx]
    a, _ = batch_a
    ra_iv = _ref(a, B.MODE_ISVALID)
    with _open() as eng:
        st = eng.verify_tx_signatures_packed(pb)
        assert np.array_equal(st, ref)
        s1 = eng.key_cache_stats()
        assert _total(s1["built"]) > 0 and s1["hits"] == (0, 0), s1
        st = eng.verify_tx_signatures_packed(pb)
        assert np.array_equal(st, ref)
        s = eng.key_cache_stats()
        assert s["built"] == (0, 0) and s["hits"] == s1["built"], (s, s1)
        _call(eng, a, batch_a[1], "A cold")
        s = _call(eng, a, ra_iv, "A warm, isValid", B.MODE_ISVALID)
        assert s["built"] == (0, 0) and _total(s["hits"]) > 0, s


def test_switched_off(engine, batch_a):
    a, ra = batch_a
    with _open(key_cache=False) as eng:
        for k in range(2):
            s = _call(eng, a, ra, f"no cache, call {k}")
            assert not s["enabled"] and s["hits"] == (0, 0) and s["built"] == (0, 0), s
