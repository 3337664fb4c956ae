"""CPU tests of tests/layout_util.py: the repackers keep content, the C oracle's verdicts do not
depend on the layout, and every precondition tests/test_gpu_layout.py states (unaligned share, all
phases present, arena.size % 4, which kind of field ends the arena, poison behind every field)
holds for every parametrisation it uses. These are conditions on the repack alone, not tolerances."""
import numpy as np
import pytest

import layout_util as LU
from corda_amd import batch as B
from corda_amd import merkle as M
from oracle import c_oracle

MIN_UNALIGNED = 0.6


@pytest.fixture(scope="module")
def verify_ref():
    b = LU.verify_case()
    return b, {mode: c_oracle.verify_batch(b, mode, 8) for mode in (B.MODE_DOVERIFY, B.MODE_ISVALID)}


def test_verify_case_shape():
    """Every length of VERIFY_LENS occurs for every scheme, one key per family is above the
    wide-table threshold, and raw and SPKI keys are both present."""
    b = LU.verify_case()
    ln = b.items["msg_len"]
    for want in LU.VERIFY_LENS:
        for scheme in (2, 3, 4):
            assert np.any((ln == want) & (b.keys["scheme"][b.items["key_idx"]] == scheme)), (want, scheme)
    uses = np.bincount(b.items["key_idx"], minlength=len(b.keys))
    ed = b.keys["scheme"] == 4
    assert (uses[ed] >= LU.WIDE_ED_USES).any() and (uses[~ed] >= LU.WIDE_EC_USES).sum() >= 2
    assert {B.KEY_RAW, B.KEY_SPKI} <= set(b.keys["fmt"].tolist())


@pytest.mark.parametrize("last", LU.VERIFY_LASTS)
@pytest.mark.parametrize("rem", LU.REMS)
@pytest.mark.parametrize("seed", LU.SEEDS)
def test_relayout_batch_keeps_content_and_verdicts(verify_ref, seed, rem, last):
    b, ref = verify_ref
    r = LU.relayout_batch(b, seed, rem=rem, last=last)
    assert r.arena.size % 4 == rem
    LU.same_content(LU.batch_fields(b), b.arena, LU.batch_fields(r), r.arena)
    st = LU.layout_stats(LU.batch_fields(r), r.arena.size)
    for kind in ("key", "sig", "msg"):
        assert st[kind]["unaligned"] >= MIN_UNALIGNED and st[kind]["phases"] == {0, 1, 2, 3}, (kind, st[kind])
        assert st[kind]["ends"] == (kind == last)
    for mode, want in ref.items():
        assert np.array_equal(c_oracle.verify_batch(r, mode, 8), want)


def test_relayout_batch_lead_and_poison(verify_ref):
    """The host-window case of test_gpu_layout: 1001 leading bytes, the keys behind the items."""
    b, ref = verify_ref
    r = LU.relayout_batch(b, LU.SEEDS[0], lead=1001, rem=3, last="key")
    f = LU.batch_fields(r)
    LU.same_content(LU.batch_fields(b), b.arena, f, r.arena)
    lo = min(int(o.min()) for o, _ in f.values())
    assert lo >= 1001 and lo % 16 != 0 and np.all(r.arena[:lo] == 0xFF)
    assert f["key"][0].min() > max(f["sig"][0].max(), f["msg"][0].max())
    assert np.array_equal(c_oracle.verify_batch(r, B.MODE_DOVERIFY, 8), ref[B.MODE_DOVERIFY])
    z = LU.relayout_batch(b, LU.SEEDS[0], poison=0, rem=2)
    LU.same_content(LU.batch_fields(b), b.arena, LU.batch_fields(z), z.arena, poison=0)


@pytest.mark.parametrize("rem", LU.REMS)
def test_relayout_spans(rem):
    rng = np.random.default_rng(3)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in list(range(0, 70)) * 4]
    phases = np.repeat(np.arange(4), 70)
    spans, arena = LU.relayout_spans(msgs, 5, lead=7, rem=rem, phases=np.where(np.arange(280) == 279, -1, phases))
    assert arena.size % 4 == rem and len(spans) == 280
    end = 0
    for i, m in enumerate(msgs):
        o, n = int(spans[i]["off"]), int(spans[i]["len"])
        assert arena[o:o + n].tobytes() == m and (o + n == arena.size or arena[o + n] == 0xFF)
        assert i == 279 or o % 4 == phases[i]
        end = max(end, o + n)
    assert end == arena.size and int(spans[279]["off"]) + 69 == arena.size
    assert np.all(arena[:7] == 0xFF)


@pytest.mark.parametrize("last", ["comp", "salt"])
@pytest.mark.parametrize("rem", LU.REMS)
def test_relayout_tx(rem, last):
    cases, cph, sph = LU.tx_case()
    txs, comps, arena = M.pack_transactions(cases)
    assert len(comps) % 64 != 0 and len(comps) == len(cph)
    t2, c2, a2 = LU.relayout_tx(txs, comps, arena, 9, rem=rem, last=last, comp_phase=cph, salt_phase=sph)
    assert a2.size % 4 == rem
    LU.same_content(LU.tx_fields(txs, comps), arena, LU.tx_fields(t2, c2), a2)
    st = LU.layout_stats(LU.tx_fields(t2, c2), a2.size, mod=64)
    assert st["comp"]["phases"] == set(range(64)) and st["comp"]["unaligned"] >= MIN_UNALIGNED
    assert st["comp"]["ends"] == (last == "comp") and st["salt"]["ends"] == (last == "salt")
    assert {p % 4 for p in st["salt"]["phases"]} == {0, 1, 2, 3}
    fixed = np.flatnonzero(cph >= 0)
    assert np.array_equal(c2["off"][fixed] % 64, cph[fixed])
    for f in ("first", "n"):
        assert np.array_equal(t2[f], txs[f])
    assert np.array_equal(c2["len"], comps["len"]) and np.array_equal(c2["flags"], comps["flags"])


@pytest.mark.parametrize("last", ["nonce", "node", "leaf", "root"])
def test_relayout_filtered(last):
    import test_filtered
    ftxs, want = test_filtered.random_tearoffs(300)
    assert set(np.unique(want).tolist()) == {0, 1, 2}
    t, n, lv, arena = M.pack_filtered(ftxs)
    for rem in LU.REMS:
        t2, n2, l2, a2 = LU.relayout_filtered(t, n, lv, arena, 13, rem=rem, last=last)
        assert a2.size % 4 == rem
        LU.same_content(LU.filtered_fields(t, n, lv), arena, LU.filtered_fields(t2, n2, l2), a2)
        st = LU.layout_stats(LU.filtered_fields(t2, n2, l2), a2.size)
        for kind in ("leaf", "nonce", "node", "root"):
            assert st[kind]["unaligned"] >= MIN_UNALIGNED and st[kind]["phases"] == {0, 1, 2, 3}
            assert st[kind]["ends"] == (kind == last)
        assert np.array_equal(n2["kind"], n["kind"]) and np.array_equal(l2["flags"], lv["flags"])


@pytest.mark.parametrize("last", ["sig", "key", "prefix"])
def test_relayout_txsig(last):
    import txsig_util
    tb, tm = LU.txsig_case()
    assert tb.n == 120 * len(LU.TMPL_LENS) and np.array_equal(np.bincount(tm), [120] * len(LU.TMPL_LENS))
    ref = c_oracle.verify_batch(txsig_util.to_message_batch(tb), B.MODE_DOVERIFY, 8)
    assert (ref == B.VALID).sum() > tb.n // 2 and (ref == B.INVALID).any()
    for rem in LU.REMS:
        r = LU.relayout_txsig(tb, 17, rem=rem, last=last)
        assert r.arena.size % 4 == rem
        LU.same_content(LU.txsig_fields(tb), tb.arena, LU.txsig_fields(r), r.arena)
        st = LU.layout_stats(LU.txsig_fields(r), r.arena.size)
        for kind in ("key", "sig", "prefix"):
            assert st[kind]["unaligned"] >= MIN_UNALIGNED and st[kind]["phases"] == {0, 1, 2, 3}
            assert st[kind]["ends"] == (kind == last)
        assert np.array_equal(c_oracle.verify_batch(txsig_util.to_message_batch(r), B.MODE_DOVERIFY, 8), ref)


def test_packed_mirror_of_a_signature_outside_the_arena():
    """TxSigBatch.packed() on an exact-end arena whose last signature claims one byte more than the
    arena holds: the 24-byte form answers CG_NOT_RUN for it, and the packed mirror says the same in
    the only way its table can (an id index outside the id table) instead of raising."""
    tb, _ = LU.txsig_case()
    r = LU.relayout_txsig(tb, 19, rem=1, last="sig")
    j = int(np.flatnonzero(r.sigs["sig_off"] + r.sigs["sig_len"] == r.arena.size)[0])
    r.sigs["sig_len"][j] += 1
    pb = r.packed()
    assert pb.sigs["tx_idx"][j] == 0xFFFFFFFF and pb.sigs["sig_len"][j] == r.sigs["sig_len"][j]
    keep = np.arange(r.n) != j
    assert np.array_equal(pb.sigs["tx_idx"][keep], r.sigs["tx_idx"][keep])
    span = (r.sigs["sig_len"].astype(np.int64) + 3) & ~3
    rel = np.concatenate([[0], np.cumsum(span)[:-1]])
    assert pb.stream.size == span.sum()
    for q in (0, j - 1, r.n - 1):
        if q != j:
            o, ln = int(r.sigs["sig_off"][q]), int(r.sigs["sig_len"][q])
            assert np.array_equal(pb.stream[rel[q]:rel[q] + ln], r.arena[o:o + ln])
