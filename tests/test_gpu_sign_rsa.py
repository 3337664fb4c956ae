"""GPU tests of the RSA-PSS signer (cg_rsa_signers_load, cg_rsa_sign_batch, cg_rsa_sign_tx_ids and its device
and pool forms): every signature byte for byte hostverify.rsa_pss_sign's (Python integers) for the given
salt, length included; every fixture record (which OpenSSL accepted when it was generated) then VALID on the
same context's RSA verifier; the wave and block edges with the seven key sizes interleaved request by
request; every status; the load refusals; the three signer sets' independence; the ordering with a verify
call on one context; and the pool's failover."""
import ctypes
import hashlib

import numpy as np
import pytest

import hostsignrsa as H
from corda_amd import _lib, signable
from corda_amd import batch as B
from oracle import ecdsa_bc as bc
from oracle import ed25519_i2p as ed

pytestmark = pytest.mark.gpu

OTHER = (b"\x01\x00other-metadata-prefix:", b"\x07\x08")
TEMPLATES = [signable.template(1, 1), OTHER]
IDS = np.frombuffer(b"".join(hashlib.sha256(b"rsa id %d" % i).digest() for i in range(5)), dtype=np.uint8).reshape(-1, 32)
PERIOD = 35  # distinct (signer, id, template, salt) tuples: the reference signs each once


def p_(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


@pytest.fixture(scope="module")
def rsa_engine(engine):  # after the session engine: torch's HIP runtime has opened the device first
    from corda_amd.engine import Engine
    e = Engine(0, rsa=True)
    yield e
    e.close()


def load_sizes(eng):
    """The seven key sizes as signers 0 .. 6, so request j's key size is j % 7."""
    st = eng.load_rsa_signers([H.signer_key(H.key(kid)) for kid in H.SIZES])
    assert not st.any()


def tuple_of(j):
    t = j % PERIOD
    return t % 7, t % 5, (t // 7) % 2, hashlib.sha256(b"salt %d" % t).digest()


_ref = {}


def ref_sig(j):
    t = j % PERIOD
    if t not in _ref:
        signer, i, tm, salt = tuple_of(t)
        pre, suf = TEMPLATES[tm]
        _ref[t] = H.sign(H.SIZES[signer], pre + IDS[i].tobytes() + suf, salt)
    return _ref[t]


def make_sr(tx_idx, signer, tmpl):
    b = B.SignRequestBuilder()
    for pre, suf in TEMPLATES:
        b.template(pre, suf)
    base = b.build()
    reqs = np.zeros(len(tx_idx), dtype=B.SIGN_REQ_DTYPE)
    reqs["tx_idx"], reqs["signer"], reqs["tmpl"] = tx_idx, signer, tmpl
    return B.SignRequests(IDS, reqs, base.tmpls, base.arena)


def requests(n, first=0):
    cols = [tuple_of(j) for j in range(first, first + n)]
    sr = make_sr([c[1] for c in cols], [c[0] for c in cols], [c[2] for c in cols])
    return sr, np.frombuffer(b"".join(c[3] for c in cols), dtype=np.uint8).copy()


def check(sigs, ln, st, n, first=0):
    assert not st.any()
    for j in range(n):
        want = ref_sig(first + j)
        assert (int(ln[j]), sigs[j].tobytes()) == (len(want), H.slot(want)), f"request {j}"


def verify_all(eng, triples):
    """(fixture key id, signature, message) -> the context's verdicts (needs rsa=True)."""
    b = B.BatchBuilder()
    for kid, sig, msg in triples:
        b.add_with_key(1, B.KEY_SPKI, bytes.fromhex(H.fixture()["keys"][kid]["spki"]), sig, msg)
    return eng.verify(b.build(), B.MODE_DOVERIFY)


# 1 ---------------------------------------------------------------- the fixture
def test_fixture_records_byte_equal_then_valid_on_the_same_context(rsa_engine):
    recs = H.records()
    kids = list(H.fixture()["keys"])
    assert len(kids) == 9 and len(recs) == 54
    st = rsa_engine.load_rsa_signers([H.signer_key(H.key(k)) for k in kids])
    assert not st.any()
    sigs, ln, st = rsa_engine.sign_rsa([(kids.index(r["key"]), r["msg"]) for r in recs], [r["salt"] for r in recs])
    for r, sig, l, s in zip(recs, sigs, ln, st):
        k = (H.fixture()["keys"][r["key"]]["bits"] + 7) // 8
        assert len(r["sig"]) == k
        assert (int(s), int(l), sig.tobytes()) == (0, k, H.slot(r["sig"])), (r["key"], len(r["msg"]))
    v = verify_all(rsa_engine, [(r["key"], sigs[j, :int(ln[j])].tobytes(), r["msg"]) for j, r in enumerate(recs)])
    assert np.array_equal(v, np.full(len(recs), B.VALID, np.uint8))
    # the splice form of one record per key: prefix || id || suffix cut out of the record's own message
    b = B.SignRequestBuilder()
    spl = [r for r in recs if len(r["msg"]) in (64, 270)]
    for r in spl:
        m = r["msg"]
        b.add_request(kids.index(r["key"]), b.tx_id(m[7:39]), b.template(m[:7], m[39:]))
    sigs, ln, st = rsa_engine.sign_rsa_tx_ids(b.build(), [r["salt"] for r in spl])
    for r, sig, l, s in zip(spl, sigs, ln, st):
        assert (int(s), int(l), sig.tobytes()) == (0, len(r["sig"]), H.slot(r["sig"])), (r["key"], len(r["msg"]))


# 2 ---------------------------------------------------------------- wave and block edges, sizes interleaved
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_counts_match_python_pow_sizes_interleaved(engine, n):
    load_sizes(engine)
    sr, salts = requests(n)
    assert [int(s) for s in sr.reqs["signer"][:7]] == list(range(7))[:min(n, 7)]
    sigs, ln, st = engine.sign_rsa_tx_ids(sr, salts)
    assert not salts.any()  # the array the C ABI read is zeroed
    check(sigs, ln, st, n)


# 3 ---------------------------------------------------------------- the device form on a side stream
def test_device_form_on_a_side_stream_equals_host_form(engine):
    import torch
    load_sizes(engine)
    n = 70
    sr, salts = requests(n, first=3)
    keep = salts.copy()
    h = engine.sign_rsa_tx_ids(sr, salts)
    check(*h, n, first=3)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.array(x, copy=True).view(np.uint8)).to(dev)  # noqa: E731
    d_ids, d_reqs, d_salts = up(sr.ids), up(sr.reqs), up(keep)
    d_arena = up(np.concatenate([sr.arena, np.zeros(-sr.arena.size % 4, np.uint8)]))
    d_sigs = torch.full((4 + 512 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_ln = torch.full((2 + 2 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_st = torch.full((3 + n,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        engine.sign_rsa_tx_ids_device(d_ids.data_ptr(), sr.n_ids, d_reqs.data_ptr(), n, sr.tmpls, d_arena.data_ptr(),
                                      sr.arena.size, d_salts.data_ptr(), d_sigs.data_ptr() + 4, d_ln.data_ptr() + 2,
                                      d_st.data_ptr() + 3, stream=s.cuda_stream)
        got, got_ln, got_st = d_sigs.clone(), d_ln.clone(), d_st.clone()
    torch.cuda.synchronize()
    got, got_ln, got_st = got.cpu().numpy(), got_ln.cpu().numpy(), got_st.cpu().numpy()
    assert np.array_equal(got[4:].reshape(-1, 512), h[0]) and np.array_equal(got_ln[2:].view(np.uint16), h[1])
    assert np.array_equal(got_st[3:], h[2])
    assert (got[:4] == 0xA5).all() and (got_ln[:2] == 0xA5).all() and (got_st[:3] == 0xA5).all()


# 4 ---------------------------------------------------------------- statuses, refusals, the three signer sets
def _raw(h, sr, salts, fill=0xA5):
    sigs = np.full(512 * sr.n, fill, dtype=np.uint8)
    ln, st = np.full(sr.n, fill * 257, dtype=np.uint16), np.full(sr.n, fill, dtype=np.uint8)
    rc = _lib.lib().cg_rsa_sign_tx_ids(h, p_(sr.ids), sr.n_ids, p_(sr.reqs), sr.n, p_(sr.tmpls), len(sr.tmpls),
                                       p_(sr.arena), sr.arena.size, p_(salts), p_(sigs), p_(ln), p_(st))
    return rc, sigs.reshape(-1, 512), ln, st


def test_statuses_load_refusals_and_the_three_signer_sets():
    from corda_amd.engine import Engine
    good = H.key("rsa2048")
    ref = H.refused()
    assert [r[0] for r in ref] == ["dp_plus_2", "n_plus_2", "even_p", "e_zero", "n_1016_bits"]
    # signers: good 1024, the five refused keys, good 2048
    keys = [H.signer_key(H.key("rsa1024"))] + [H.signer_key(k) for _, _, k in ref] + [H.signer_key(good)]
    salt = [hashlib.sha256(b"s%d" % j).digest() for j in range(12)]
    #     good  refused at load     good  signer  tx_idx  template
    sg = [0, 1, 2, 3, 4, 5, 6, 7, 0, 6]
    tx = [1, 0, 0, 0, 0, 0, 2, 0, 5, 0]
    tm = [0, 0, 0, 0, 0, 0, 1, 0, 0, 2]
    sr = make_sr(tx, sg, tm)
    salts = np.frombuffer(b"".join(salt[:10]), dtype=np.uint8).copy()
    want = [0] + [B.NOT_RUN] * 5 + [0] + [B.NOT_RUN] * 3
    ed_seed = ed.entropy_seed(20)
    ed_sr = B.SignRequests(IDS, np.zeros(1, dtype=B.SIGN_REQ_DTYPE), sr.tmpls, sr.arena)
    ec_d = 0x1234567
    ec_k = hashlib.sha256(b"ec k").digest()
    with Engine(0) as eng:
        # no RSA signers: CG_ERR_ARG, nothing written -- also with the other two sets loaded
        eng.load_signers([ed_seed])
        eng.load_ec_signers([(3, ec_d.to_bytes(32, "big"))])
        rc, sigs, ln, st = _raw(eng._h, sr, salts)
        assert rc == -1 and (sigs == 0xA5).all() and (ln == 0xA5A5).all() and (st == 0xA5).all()
        assert "no RSA signers" in _lib.last_error()
        lst = eng.load_rsa_signers(keys)
        assert list(lst) == [0] + [s for _, s, _ in ref] + [0]
        assert list(lst[1:6]) == [B.KEY_INVALID] * 4 + [B.UNSUPPORTED]
        rc, sigs, ln, st = _raw(eng._h, sr, salts)
        assert rc == 0 and list(st) == want
        for j, w in enumerate(want):
            if w:
                assert not sigs[j].any() and ln[j] == 0, "an unsigned request gets 512 zero bytes and length 0"
        pre, suf = TEMPLATES[0]
        w0 = H.sign("rsa1024", pre + IDS[1].tobytes() + suf, salt[0])
        w6 = H.sign(good, OTHER[0] + IDS[2].tobytes() + OTHER[1], salt[6])
        assert (int(ln[0]), sigs[0].tobytes()) == (128, H.slot(w0)) and (int(ln[6]), sigs[6].tobytes()) == (256, H.slot(w6))
        # the other two sets are untouched by the RSA load, and still sign
        e_sig, e_st = eng.sign_tx_ids(ed_sr)
        assert not e_st.any() and e_sig[0].tobytes() == ed.sign(ed_seed, pre + IDS[0].tobytes() + suf)
        c_sig, c_ln, c_st = eng.sign_ec([(0, b"abc")], [ec_k])
        assert not c_st.any() and c_sig[0, :c_ln[0]].tobytes() == bc.der_encode_sig(
            *bc.sign(3, ec_d, b"abc", int.from_bytes(ec_k, "big")))
        # clearing either of them leaves the RSA set signing the same bytes
        eng.clear_signers()
        eng.clear_ec_signers()
        rc, sigs2, ln2, st2 = _raw(eng._h, sr, salts)
        assert rc == 0 and np.array_equal(sigs2, sigs) and np.array_equal(ln2, ln) and list(st2) == want
        eng.load_signers([ed_seed])
        # the arena form: the empty check first (before the signer), a signer out of range, a refused signer
        s3, l3, t3 = eng.sign_rsa([(0, b"abc"), (99, b""), (2, b""), (99, b"abc"), (2, b"abc"), (6, b"xyz" * 50)],
                                  salt[:6])
        assert list(t3) == [0, B.EMPTY, B.EMPTY, B.NOT_RUN, B.NOT_RUN, 0] and not s3[1:5].any() and not l3[1:5].any()
        assert s3[0].tobytes() == H.slot(H.sign("rsa1024", b"abc", salt[0]))
        assert s3[5].tobytes() == H.slot(H.sign(good, b"xyz" * 50, salt[5])) and list(l3[[0, 5]]) == [128, 256]
        # bytes outside the arena
        items = np.zeros(2, dtype=B.SIGN_ITEM_DTYPE)
        items["msg_off"], items["msg_len"], items["signer"] = [0, 6], [8, 3], [0, 0]
        arena = np.frombuffer(b"01234567" + bytes(8), dtype=np.uint8).copy()
        sg4, l4, st4 = np.full(1024, 0xA5, np.uint8), np.full(2, 0xA5A5, np.uint16), np.full(2, 0xA5, np.uint8)
        two = np.frombuffer(salt[0] * 2, dtype=np.uint8).copy()
        assert _lib.lib().cg_rsa_sign_batch(eng._h, p_(items), 2, p_(arena), 8, p_(two), p_(sg4), p_(l4), p_(st4)) == 0
        assert list(st4) == [0, B.NOT_RUN] and sg4[:512].tobytes() == H.slot(H.sign("rsa1024", b"01234567", salt[0]))
        assert not sg4[512:].any() and list(l4) == [128, 0]
        # n == 0 is a no-op
        assert _lib.lib().cg_rsa_sign_batch(eng._h, None, 0, None, 0, None, None, None, None) == 0
        # a reload replaces the set; a number outside `secrets` refuses that signer alone
        table = np.zeros(2, dtype=[(f, "<u4") for f in ("n_off", "n_len", "p_off", "p_len", "q_off", "q_len", "dp_off",
                                                        "dp_len", "dq_off", "dq_len", "qinv_off", "qinv_len", "e")])
        parts = [H.be(good[f]) for f in ("n", "p", "q", "dp", "dq", "qinv")]
        sec = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        at = 0
        for f, v in zip(("n", "p", "q", "dp", "dq", "qinv"), parts):
            table[f + "_off"], table[f + "_len"] = at, len(v)
            at += len(v)
        table["e"] = good["e"]
        table[1]["qinv_len"] += 1  # one byte past the end
        lst = np.full(2, 0xA5, np.uint8)
        assert _lib.lib().cg_rsa_signers_load(eng._h, p_(table), 2, p_(sec), sec.size, p_(lst)) == 0
        assert list(lst) == [0, B.KEY_INVALID]
        s5, l5, t5 = eng.sign_rsa([(0, b"abc"), (1, b"abc")], salt[:2])
        assert list(t5) == [0, B.NOT_RUN] and s5[0].tobytes() == H.slot(H.sign(good, b"abc", salt[0]))
        # cleared: CG_ERR_ARG again, nothing written; the Ed25519 set still signs
        eng.clear_rsa_signers()
        rc, sigs, ln, st = _raw(eng._h, sr, salts)
        assert rc == -1 and (sigs == 0xA5).all() and (st == 0xA5).all()
        eng.clear_rsa_signers()  # a no-op when none is loaded
        e_sig2, e_st2 = eng.sign_tx_ids(ed_sr)
        assert not e_st2.any() and np.array_equal(e_sig2, e_sig)
        assert _lib.lib().cg_rsa_signers_load(eng._h, p_(table), 0, p_(sec), sec.size, p_(lst)) == -1
        assert _lib.lib().cg_rsa_signers_load(eng._h, p_(table), 65536, p_(sec), sec.size, p_(lst)) == -1


# 5 ---------------------------------------------------------------- a verify call between two sign calls
def test_a_verify_call_between_two_sign_calls_on_one_context(rsa_engine):
    load_sizes(rsa_engine)
    n = 21
    a = rsa_engine.sign_rsa_tx_ids(*requests(n))
    triples = []
    for j in range(n):
        signer, i, tm, _ = tuple_of(j)
        pre, suf = TEMPLATES[tm]
        triples.append((H.SIZES[signer], a[0][j, :int(a[1][j])].tobytes(), pre + IDS[i].tobytes() + suf))
    v = verify_all(rsa_engine, triples)
    b = rsa_engine.sign_rsa_tx_ids(*requests(n, first=14))
    check(*a, n)
    assert np.array_equal(v, np.full(n, B.VALID, np.uint8))
    check(*b, n, first=14)


# 6 ---------------------------------------------------------------- the pool: one slot, failover
def test_pool_signs_on_one_slot_and_fails_over():
    from corda_amd.engine import EnginePool
    n = 40
    sr, salts = requests(n)
    with EnginePool([0, 0], chunk_items=16) as ep:
        sigs0, ln0, st0 = np.full(512 * n, 0xA5, np.uint8), np.full(n, 0xA5A5, np.uint16), np.full(n, 0xA5, np.uint8)
        rc = _lib.lib().cg_pool_rsa_sign_tx_ids(ep._h, p_(sr.ids), sr.n_ids, p_(sr.reqs), sr.n, p_(sr.tmpls), len(sr.tmpls),
                                                p_(sr.arena), sr.arena.size, p_(salts), p_(sigs0), p_(ln0), p_(st0), None)
        assert rc == -1 and (sigs0 == 0xA5).all() and (ln0 == 0xA5A5).all() and (st0 == 0xA5).all()  # no signers yet
        load_sizes(ep)
        sigs, ln, st = ep.sign_rsa_tx_ids(sr, salts.copy())
        assert ep.last_stats["reruns"] == 0 and ep.last_stats["failed_slots"] == 0
        check(sigs, ln, st, n)
        ep.inject_fault(0)  # a software flag: no device fault is provoked
        sigs2, ln2, st2 = ep.sign_rsa_tx_ids(sr, salts.copy())
        assert np.array_equal(sigs2, sigs) and np.array_equal(ln2, ln) and not st2.any()
        assert ep.last_stats["reruns"] == 1 and ep.last_stats["failed_slots"] == 1 and ep.last_stats["not_run"] == 0
        assert ep.healthy() == [False, True]
        ep.inject_fault(1)
        sigs3, ln3, st3 = ep.sign_rsa_tx_ids(sr, salts.copy(), allow_partial=True)  # nothing healthy
        assert (st3 == B.NOT_RUN).all() and not sigs3.any() and not ln3.any() and ep.last_stats["not_run"] == n
        ep.inject_fault(0, False)
        ep.inject_fault(1, False)
        sigs4, ln4, st4 = ep.sign_rsa_tx_ids(sr, salts.copy())
        assert np.array_equal(sigs4, sigs) and not st4.any() and ep.healthy() == [True, True]
        ep.clear_rsa_signers()
