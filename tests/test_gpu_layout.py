"""GPU tests at unaligned, poisoned and exact-end arena layouts.

include/cordagpu.h promises that any arena layout is correct: no offset needs an alignment. Every
input here is a content-preserving repack (tests/layout_util.py) of an ordinary 4-aligned one:
fields at byte phases drawn from a seeded RNG (mod 64 for transaction components), 0xFF in every gap
and directly behind every message, component and leaf, and the arena ending at the last byte of the
last field with arena_len % 4 in {1, 2, 3}. Each answer is compared bit for bit with a reference
that never sees the layout: hashlib, oracle.corda.tx_id, the tear-off oracle of tests/test_filtered.py,
or the C oracle on the original batch. tests/test_layout_util.py shows on the CPU that the repacks
alone meet the preconditions asserted here (unaligned share, phases, which field ends the arena).

What this reaches that 4-aligned, zero-padded inputs never did: the funnel shifts of sha2.h with a
non-zero shift, the masking of the bytes behind a message before the 0x80 padding byte is ORed in,
the dword-by-dword fallbacks at the arena's last partial chunk (cg_ld_dwords4, k_tx_leaves
load_sector), the two-sector LDS ring of k_tx_leaves at every offset mod 64 and its capped block
class, the key / signature / DER readers at odd offsets, and the host window logic of
cg_verify_batch with extents that start and end on odd bytes.
"""
import ctypes
import hashlib

import numpy as np
import pytest

import layout_util as LU
import txsig_util
from corda_amd import _lib
from corda_amd import batch as B
from corda_amd import merkle as M
from oracle import c_oracle, corda as ocorda

pytestmark = pytest.mark.gpu
MIN_UNALIGNED = 0.6


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


def _diff(st, want):
    bad = np.flatnonzero(st != want)
    return f"{bad.size} of {st.size} differ, first at {bad[:8].tolist()}: got {st[bad[:8]].tolist()} want {want[bad[:8]].tolist()}"


# ----------------------------------------------------------------------------- a. verify
@pytest.fixture(scope="module")
def verify_ref():
    """The batch of layout_util.verify_case and the C oracle's verdicts on it as generated (4-aligned,
    zero padding), per mode: the reference of every relaid-out run."""
    b = LU.verify_case()
    return b, {mode: c_oracle.verify_batch(b, mode, 16) for mode in (B.MODE_DOVERIFY, B.MODE_ISVALID)}


def _batch_preconditions(r, rem, last):
    st = LU.layout_stats(LU.batch_fields(r), r.arena.size)
    assert r.arena.size % 4 == rem
    for kind in ("key", "sig", "msg"):
        assert st[kind]["unaligned"] >= MIN_UNALIGNED and st[kind]["phases"] == {0, 1, 2, 3}
        assert st[kind]["ends"] == (kind == last)


@pytest.mark.parametrize("last", LU.VERIFY_LASTS)
@pytest.mark.parametrize("rem", LU.REMS)
@pytest.mark.parametrize("seed", LU.SEEDS)
def test_verify_relaid_out(engine, verify_ref, seed, rem, last):
    """All three schemes, message lengths at every SHA padding and block edge and on both sides of
    ITEM_LONG_MIN, the golden key encodings and one wide-table key per scheme, with keys, signatures
    and messages at odd byte phases, in doVerify and isValid mode."""
    b, ref = verify_ref
    r = LU.relayout_batch(b, seed, rem=rem, last=last)
    _batch_preconditions(r, rem, last)
    for mode, want in ref.items():
        st = engine.verify(r, mode)
        assert np.array_equal(st, want), f"mode {mode}: {_diff(st, want)}"


def test_verify_relaid_out_device_form(engine, verify_ref):
    """The same through cg_verify_batch_device: the HBM arena holds arena_len rounded up to 4 bytes
    (the device contract of include/cordagpu.h), the tail bytes 0xFF, and the exact arena_len is passed."""
    import torch
    b, ref = verify_ref
    dev = torch.device("cuda", 0)
    for rem, last in zip(LU.REMS, LU.VERIFY_LASTS):
        r = LU.relayout_batch(b, LU.SEEDS[0], rem=rem, last=last)
        _batch_preconditions(r, rem, last)
        padded = np.full((r.arena.size + 3) & ~3, 0xFF, np.uint8)
        padded[:r.arena.size] = r.arena
        kd = torch.from_numpy(r.keys.view(np.uint8)).to(dev)
        idd = torch.from_numpy(r.items.view(np.uint8)).to(dev)
        ad = torch.from_numpy(padded).to(dev)
        assert ad.data_ptr() % 4 == 0 and ad.numel() == (r.arena.size + 3) // 4 * 4
        for mode, want in ref.items():
            sd = torch.full((r.n,), 255, dtype=torch.uint8, device=dev)
            engine.verify_device(kd.data_ptr(), len(r.keys), idd.data_ptr(), r.n, ad.data_ptr(), r.arena.size,
                                 sd.data_ptr(), mode)
            torch.cuda.synchronize()
            st = sd.cpu().numpy()
            assert np.array_equal(st, want), f"rem {rem} mode {mode}: {_diff(st, want)}"


# ----------------------------------------------------------------------------- f. host window and chunks
def test_host_window_and_chunks(verify_ref):
    """cg_verify_batch in chunks of 257 items on the batch relaid out behind 1001 junk bytes with the
    keys behind the items: more than 8 chunks whose extents start and end on odd bytes, and a device
    window that starts at a non-zero offset that is no multiple of 16 (plan_host rounds it down)."""
    from corda_amd.engine import Engine
    b, ref = verify_ref
    r = LU.relayout_batch(b, LU.SEEDS[0], lead=1001, rem=3, last="key")
    _batch_preconditions(r, 3, "key")
    f = LU.batch_fields(r)
    lo = min(int(o.min()) for o, _ in f.values())
    assert lo >= 1001 and lo % 16 != 0
    assert f["key"][0].min() > max(f["sig"][0].max(), f["msg"][0].max())
    chunk = 257
    assert r.n > 8 * chunk
    first = [r.n * k // -(-r.n // chunk) for k in range(-(-r.n // chunk) + 1)]   # plan_host's split
    odd = 0
    for k in range(len(first) - 1):
        it = r.items[first[k]:first[k + 1]]
        e_lo = min(int(it["sig_off"].min()), int(it["msg_off"].min()))
        e_hi = max(int((it["sig_off"] + it["sig_len"]).max()), int((it["msg_off"] + it["msg_len"]).max()))
        odd += (e_lo % 4 != 0) + (e_hi % 4 != 0)
    assert odd >= len(first) - 1   # half of the chunk boundaries at least are no multiple of 4
    with Engine(0, chunk_items=chunk) as eng:
        for mode, want in ref.items():
            st = eng.verify(r, mode)
            assert np.array_equal(st, want), f"mode {mode}: {_diff(st, want)}"


# ----------------------------------------------------------------------------- b. hashing
def _hash_call(engine, name, size, spans, arena):
    out = np.zeros(size * len(spans), dtype=np.uint8)
    fn = getattr(_lib.lib(), name)
    _lib.check(fn(engine._h, _p(spans), len(spans), _p(arena), arena.size, _p(out)), name)
    return out.reshape(-1, size)


@pytest.fixture(scope="module")
def hash_msgs():
    rng = np.random.default_rng(23)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in list(range(0, 301)) + [1000, 5000]] * 4
    phases = np.repeat(np.arange(4), len(msgs) // 4)
    d256 = np.array([np.frombuffer(hashlib.sha256(m).digest(), np.uint8) for m in msgs])
    d512 = np.array([np.frombuffer(hashlib.sha512(m).digest(), np.uint8) for m in msgs])
    return msgs, phases, d256, d512


@pytest.mark.parametrize("rem", LU.REMS)
def test_sha_batches_relaid_out(engine, hash_msgs, rem):
    """cg_sha256_batch / cg_sha512_batch over every length 0..300, 1000 and 5000 at each of the four
    byte phases, 0xFF around every message, the last span ending the arena: against hashlib."""
    msgs, phases, d256, d512 = hash_msgs
    ph = phases.copy()
    ph[-1] = -1   # the last span's phase follows from arena.size % 4
    spans, arena = LU.relayout_spans(msgs, 29, lead=3, rem=rem, phases=ph)
    f = LU.spans_fields(spans)
    assert arena.size % 4 == rem and LU.layout_stats(f, arena.size)["span"]["ends"]
    assert np.array_equal(spans["off"][:-1] % 4, phases[:-1])
    assert int(spans["off"][-1] + spans["len"][-1]) == arena.size and spans["len"][-1] == 5000
    got = _hash_call(engine, "cg_sha256_batch", 32, spans, arena)
    bad = np.flatnonzero((got != d256).any(axis=1))
    assert bad.size == 0, f"sha256: (len, phase) {[(len(msgs[i]), int(spans['off'][i] % 4)) for i in bad[:10]]}"
    got = _hash_call(engine, "cg_sha512_batch", 64, spans, arena)
    bad = np.flatnonzero((got != d512).any(axis=1))
    assert bad.size == 0, f"sha512: (len, phase) {[(len(msgs[i]), int(spans['off'][i] % 4)) for i in bad[:10]]}"


# ----------------------------------------------------------------------------- c. transaction ids
@pytest.fixture(scope="module")
def tx_ref():
    cases, cph, sph = LU.tx_case()
    txs, comps, arena = M.pack_transactions(cases)
    ids = np.array([np.frombuffer(ocorda.tx_id(blobs, salt, sb), np.uint8) for blobs, salt, sb in cases])
    return cases, cph, sph, txs, comps, arena, ids


@pytest.mark.parametrize("last", ["comp", "salt"])
@pytest.mark.parametrize("rem", LU.REMS)
def test_tx_ids_relaid_out(engine, tx_ref, rem, last):
    """cg_tx_ids (k_tx_leaves) against oracle.corda.tx_id: a 3-leaf transaction per component offset
    mod 64 and per length at the one- and two-block padding edges (with the nonce suffix and, for the
    salt leaf, without), 200 transactions in the capped block class with mixed block counts per wave,
    leaf counts 1..130, salts at every phase, a component or a salt ending the arena, a partial last wave."""
    cases, cph, sph, txs, comps, arena, ids = tx_ref
    t2, c2, a2 = LU.relayout_tx(txs, comps, arena, 37, lead=5, rem=rem, last=last, comp_phase=cph, salt_phase=sph)
    st = LU.layout_stats(LU.tx_fields(t2, c2), a2.size, mod=64)
    assert a2.size % 4 == rem and len(c2) % 64 != 0
    assert st["comp"]["phases"] == set(range(64)) and st["comp"]["ends"] == (last == "comp")
    assert {p % 4 for p in st["salt"]["phases"]} == {0, 1, 2, 3} and st["salt"]["ends"] == (last == "salt")
    n = c2["len"].astype(np.int64) + np.where(c2["flags"] & 1, 0, 32)
    capped = (n + 9 + 63) // 64 >= 16
    assert capped.sum() > 64 and len(set(((n[capped] + 72) // 64).tolist())) >= 4
    got, status = engine.tx_ids(t2, c2, a2)
    assert np.all(status == 0)
    bad = np.flatnonzero((got != ids).any(axis=1))
    assert bad.size == 0, (f"{bad.size} ids differ; (n leaves, component off % 64, len) of the first: "
                           f"{[(int(t2['n'][t]), (c2['off'][int(t2['first'][t]):][:3] % 64).tolist(), c2['len'][int(t2['first'][t]):][:3].tolist()) for t in bad[:6]]}")


# ----------------------------------------------------------------------------- d. tear-offs
@pytest.mark.parametrize("last", ["nonce", "node"])
def test_filtered_relaid_out(engine, last):
    """cg_verify_filtered on the tear-offs of test_filtered_random_vs_oracle (300 of them) with leaf
    blobs, nonces, node hashes and roots at odd phases; a nonce / a node hash is the arena's last 32 bytes."""
    import test_filtered
    ftxs, want = test_filtered.random_tearoffs(300)
    assert set(np.unique(want).tolist()) == {0, 1, 2}
    t, n, lv, arena = M.pack_filtered(ftxs)
    for rem in LU.REMS:
        t2, n2, l2, a2 = LU.relayout_filtered(t, n, lv, arena, 13, rem=rem, last=last)
        st = LU.layout_stats(LU.filtered_fields(t2, n2, l2), a2.size)
        assert a2.size % 4 == rem
        for kind in ("leaf", "nonce", "node", "root"):
            assert st[kind]["unaligned"] >= MIN_UNALIGNED and st[kind]["phases"] == {0, 1, 2, 3}
            assert st[kind]["ends"] == (kind == last)
        got = engine.verify_filtered(t2, n2, l2, a2)
        assert np.array_equal(got, want), f"rem {rem}: {_diff(got, want)}"


# ----------------------------------------------------------------------------- e. tx signatures
@pytest.fixture(scope="module")
def txsig_ref():
    tb, tm = LU.txsig_case()
    mb = txsig_util.to_message_batch(tb)
    ref = {mode: c_oracle.verify_batch(mb, mode, 16) for mode in (B.MODE_DOVERIFY, B.MODE_ISVALID)}
    assert (ref[0] == B.VALID).sum() > tb.n // 2 and (ref[0] == B.INVALID).any()
    return tb, tm, ref


@pytest.mark.parametrize("rem,last", list(zip(LU.REMS, ["sig", "prefix", "key"])))
def test_tx_signatures_relaid_out(engine, txsig_ref, rem, last):
    """Ed25519 and both ECDSA curves through the SignableData splice for every template of
    layout_util.TMPL_LENS, template, key and signature bytes at odd phases with 0xFF around them:
    the 24-byte table and the packed 12-byte form, once with the items of each template in a call
    of their own (every wave shares one template: the wave-uniform branch of the hash kernels) and
    once with the templates interleaved item by item (the per-lane branch)."""
    tb, tm, ref = txsig_ref
    r = LU.relayout_txsig(tb, 17, rem=rem, last=last)
    st = LU.layout_stats(LU.txsig_fields(r), r.arena.size)
    assert r.arena.size % 4 == rem
    for kind in ("key", "sig", "prefix"):
        assert st[kind]["unaligned"] >= MIN_UNALIGNED and st[kind]["phases"] == {0, 1, 2, 3}
        assert st[kind]["ends"] == (kind == last)
    # interleaved: item j of the call has template j % n
    order = np.argsort((np.arange(r.n) % 120) * len(LU.TMPL_LENS) + tm)   # 120 consecutive items a template
    mixed = r.subset(order)
    assert np.array_equal(mixed.sigs["tmpl"][:2 * len(LU.TMPL_LENS)], np.tile(np.arange(len(LU.TMPL_LENS)), 2))
    for mode, want in ref.items():
        got = engine.verify_tx_signatures(mixed, mode)
        assert np.array_equal(got, want[order]), f"24-byte, interleaved, mode {mode}: {_diff(got, want[order])}"
        got = engine.verify_tx_signatures_packed(mixed.packed(), mode)
        assert np.array_equal(got, want[order]), f"packed, interleaved, mode {mode}: {_diff(got, want[order])}"
    want = ref[B.MODE_DOVERIFY]
    for j, lens in enumerate(LU.TMPL_LENS):
        idx = np.flatnonzero(tm == j)
        one = r.subset(idx)
        got = engine.verify_tx_signatures(one)
        assert np.array_equal(got, want[idx]), f"24-byte, template {lens}: {_diff(got, want[idx])}"
        got = engine.verify_tx_signatures_packed(one.packed())
        assert np.array_equal(got, want[idx]), f"packed, template {lens}: {_diff(got, want[idx])}"
