"""GPU tests of the ECDSA signer (cg_ec_signers_load, cg_ec_sign_batch, cg_ec_sign_tx_ids and its device and
pool forms): every signature byte for byte BC's DER bytes for the given k (oracle.ecdsa_bc.sign +
der_encode_sig), lengths and statuses included; the fixture's crafted k at the G table's digit edges; the
wave, block, chunk and 16 x 64 inversion-run edges with the two curves interleaved lane by lane; every
fixed-base radix; the two signer sets' independence; the ordering with verify calls on one context; and
the pool's failover."""
import ctypes
import hashlib

import numpy as np
import pytest

import hostsignec as H
from corda_amd import _lib, signable
from corda_amd import batch as B
from oracle import ecdsa_bc as bc
from oracle import ed25519_i2p as ed

pytestmark = pytest.mark.gpu

RUN_K = 16  # corda_amd/csrc/sign_ec.hip SIGN_EC_RUN_K: items per lane of the two inversion runs
OTHER = (b"\x01\x00other-metadata-prefix:", b"\x07\x08")
TEMPLATES = [signable.template(1, 3), OTHER]
# signers: even indices secp256k1, odd secp256r1, so request j's curve is j % 2: lane by lane
D = [int.from_bytes(hashlib.sha256(b"ec signer %d" % i).digest(), "big") % (bc.CURVES[2 + i % 2].n - 1) + 1 for i in range(4)]
SIGNERS = [(2 + i % 2, d.to_bytes(32, "big")) for i, d in enumerate(D)]
PERIOD = 96  # distinct (signer, id, template, k) tuples: the oracle signs each once
IDS = np.frombuffer(b"".join(hashlib.sha256(b"id %d" % i).digest() for i in range(7)), dtype=np.uint8).reshape(-1, 32)


def p_(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


def tuple_of(j):
    """(signer, id index, template, k) of request j; j % 2 is the curve."""
    t = j % PERIOD
    signer = t % 4
    k = int.from_bytes(hashlib.sha256(b"nonce %d" % t).digest(), "big") % (bc.CURVES[2 + signer % 2].n - 1) + 1
    return signer, t % 7, (t // 4) % 2, k


_oracle = {}


def oracle_sig(j):
    t = j % PERIOD
    if t not in _oracle:
        signer, i, tm, k = tuple_of(t)
        pre, suf = TEMPLATES[tm]
        _oracle[t] = bc.der_encode_sig(*bc.sign(SIGNERS[signer][0], D[signer], pre + IDS[i].tobytes() + suf, k))
    return _oracle[t]


def make_sr(tx_idx, signer, tmpl, ids=IDS, templates=TEMPLATES):
    b = B.SignRequestBuilder()
    for pre, suf in templates:
        b.template(pre, suf)
    base = b.build()
    reqs = np.zeros(len(tx_idx), dtype=B.SIGN_REQ_DTYPE)
    reqs["tx_idx"], reqs["signer"], reqs["tmpl"] = tx_idx, signer, tmpl
    return B.SignRequests(ids, reqs, base.tmpls, base.arena)


def requests(n, first=0):
    cols = [tuple_of(j) for j in range(first, first + n)]
    sr = make_sr([c[1] for c in cols], [c[0] for c in cols], [c[2] for c in cols])
    nonces = np.frombuffer(b"".join(c[3].to_bytes(32, "big") for c in cols), dtype=np.uint8).copy()
    return sr, nonces


def check(sigs, ln, st, n, first=0, which=None):
    assert not st.any()
    for j in (range(n) if which is None else which):
        want = oracle_sig(first + j)
        assert (int(ln[j]), sigs[j].tobytes()) == (len(want), H.slot(want)), f"request {j}"


def load(engine):
    pubs, st = engine.load_ec_signers(SIGNERS)
    assert not st.any() and pubs == [bc.raw_key(bc.public_point(s, d)) for (s, _), d in zip(SIGNERS, D)]
    return pubs


# 1 ---------------------------------------------------------------- the fixture
def _fixture_signers(engine):
    keys = []
    for r in H.records():
        if (r["scheme"], r["d"]) not in keys:
            keys.append((r["scheme"], r["d"]))
    pubs, st = engine.load_ec_signers(keys)
    assert not st.any()
    for (s, d), pub in zip(keys, pubs):
        assert pub == bc.raw_key(bc.public_point(s, int.from_bytes(d, "big")))
    return keys


def test_fixture_records_byte_equal_arena_and_host_splice_forms(engine):
    recs = H.records()
    keys = _fixture_signers(engine)
    # the arena form: every record (a splice record as its materialised message)
    sigs, ln, st = engine.sign_ec([(keys.index((r["scheme"], r["d"])), H.record_message(r)) for r in recs],
                                  [r["k"] for r in recs])
    for r, sig, l, s in zip(recs, sigs, ln, st):
        assert (int(s), int(l), sig.tobytes()) == (r["status"], len(r["sig"]), H.slot(r["sig"])), r["note"]
    assert sorted(set(int(s) for s in st)) == [0, B.EMPTY, B.NONCE_REJECTED]
    # the host splice form
    spl = [r for r in recs if "prefix" in r]
    b = B.SignRequestBuilder()
    for r in spl:
        b.add_request(keys.index((r["scheme"], r["d"])), b.tx_id(r["id"]), b.template(r["prefix"], r["suffix"]))
    sigs, ln, st = engine.sign_ec_tx_ids(b.build(), [r["k"] for r in spl])
    for r, sig, l, s in zip(spl, sigs, ln, st):
        assert (int(s), int(l), sig.tobytes()) == (0, len(r["sig"]), H.slot(r["sig"])), r["note"]


def test_fixture_splice_records_byte_equal_device_form(engine):
    """The fixture's splice records (the real template, the straddling prefixes 0, 1, 2, 3, 45, 81, 233) through
    cg_ec_sign_tx_ids_device on caller-owned device buffers: the resumed-midstate SpliceLd path."""
    import torch
    keys = _fixture_signers(engine)
    spl = [r for r in H.records() if "prefix" in r]
    assert {len(r["prefix"]) for r in spl} == {0, 1, 2, 3, 45, 81, 233, 234}
    b = B.SignRequestBuilder()
    for r in spl:
        b.add_request(keys.index((r["scheme"], r["d"])), b.tx_id(r["id"]), b.template(r["prefix"], r["suffix"]))
    sr = b.build()
    n = sr.n
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    d_ids, d_reqs, d_arena = up(sr.ids), up(sr.reqs), up(np.concatenate([sr.arena, np.zeros(-sr.arena.size % 4, np.uint8)]))
    d_k = up(np.frombuffer(b"".join(r["k"] for r in spl), dtype=np.uint8).copy())
    d_sigs = torch.full((72 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_ln = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        engine.sign_ec_tx_ids_device(d_ids.data_ptr(), sr.n_ids, d_reqs.data_ptr(), n, sr.tmpls, d_arena.data_ptr(),
                                     sr.arena.size, d_k.data_ptr(), d_sigs.data_ptr(), d_ln.data_ptr(), d_st.data_ptr(),
                                     stream=s.cuda_stream)
    torch.cuda.synchronize()
    sigs, ln, st = d_sigs.cpu().numpy().reshape(-1, 72), d_ln.cpu().numpy(), d_st.cpu().numpy()
    for r, sig, l, t in zip(spl, sigs, ln, st):
        assert (int(t), int(l), sig.tobytes()) == (0, len(r["sig"]), H.slot(r["sig"])), r["note"]


def test_fixture_edge_scalars_at_this_radix_arena_form(engine):
    """The G-table edge scalars of all three radixes as k, on the default (2^26) context."""
    edges, msg = H.edges(), H.edge_msg()
    engine.load_ec_signers([(s, H.key(s)[0]) for s in (2, 3)])
    sigs, ln, st = engine.sign_ec([(s - 2, msg) for s, _, _ in edges], [k for _, k, _ in edges])
    assert not st.any()
    for (s, k, dg), sig, l in zip(edges, sigs, ln):
        assert H.digest(sig[:int(l)].tobytes()) == dg and not sig[int(l):].any(), (s, k.hex())


# 2 ---------------------------------------------------------------- wave, block and inversion-run edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1023, 1024, 1025])
def test_counts_match_oracle_curves_interleaved(engine, n):
    """1023 / 1024 / 1025 = 64 x RUN_K - 1, + 0, + 1: the last lane's partial inversion run."""
    assert 64 * RUN_K == 1024
    load(engine)
    sr, nonces = requests(n)
    assert set(int(s) % 2 for s in sr.reqs["signer"][0::2]) == {0} and (n < 2 or set(int(s) % 2 for s in sr.reqs["signer"][1::2]) == {1})
    sigs, ln, st = engine.sign_ec_tx_ids(sr, nonces)
    assert not nonces.any()  # the array the C ABI read is zeroed
    check(sigs, ln, st, n)


# 3 ---------------------------------------------------------------- four chunks, then verified on the GPU
def _verify_batch(sr, sigs, ln, pubs, schemes):
    keys = np.zeros(len(pubs), dtype=B.KEY_DTYPE)
    head = b"".join(pubs)
    keys["off"], keys["len"] = 64 * np.arange(len(pubs)), 64
    keys["scheme"], keys["fmt"] = schemes, B.KEY_RAW
    tmpls = sr.tmpls.copy()
    tmpls["prefix_off"] += len(head)
    tmpls["suffix_off"] += len(head)
    arena = np.concatenate([np.frombuffer(head, dtype=np.uint8), sr.arena])
    s12 = np.zeros(sr.n, dtype=B.TXSIG12_DTYPE)
    s12["tx_idx"], s12["key_idx"], s12["tmpl"], s12["sig_len"] = sr.reqs["tx_idx"], sr.reqs["signer"], sr.reqs["tmpl"], ln
    stream = np.concatenate([sigs[j, :(int(ln[j]) + 3) & ~3] for j in range(sr.n)])  # the slot's zeros pad to 4
    return B.PackedTxSigBatch(keys, sr.ids, s12, stream, tmpls, arena)


def test_four_chunks_sign_then_verify_on_the_same_context():
    from corda_amd.engine import Engine
    n, chunk = 6001, 1501
    sr, nonces = requests(n)
    with Engine(0, chunk_items=chunk) as eng:
        pubs = load(eng)
        sigs, ln, st = eng.sign_ec_tx_ids(sr, nonces)
        assert -(-n // chunk) == 4
        check(sigs, ln, st, n)
        pb = _verify_batch(sr, sigs, ln, pubs, [s for s, _ in SIGNERS])
        assert np.array_equal(eng.verify_tx_signatures_packed(pb), np.full(n, B.VALID, np.uint8))
        flipped = IDS.copy()
        flipped[:, 5] ^= 0x10
        bad = B.PackedTxSigBatch(pb.keys, flipped, pb.sigs, pb.stream, pb.tmpls, pb.arena)
        assert np.array_equal(eng.verify_tx_signatures_packed(bad), np.full(n, B.INVALID, np.uint8))


# 4 ---------------------------------------------------------------- host form against device form
def test_device_form_equals_host_form_at_odd_offsets(engine):
    import torch
    load(engine)
    n = 3001
    sr, nonces = requests(n, first=5)
    keep = nonces.copy()
    h = engine.sign_ec_tx_ids(sr, nonces)
    check(*h, n, first=5)
    dev = torch.device("cuda", 0)
    # the request table at an odd multiple of its 8 bytes, the ids, the nonces and the signatures at odd
    # multiples of 4 bytes, inside larger 4-byte-aligned buffers
    req_b = sr.reqs.view(np.uint8)
    req_at = 8 * 5
    ids_at = req_at + req_b.size + 4 * 7
    non_at = ids_at + sr.ids.size + 4 * 3
    buf = np.full(non_at + keep.size + 64, 0xEE, dtype=np.uint8)
    buf[req_at:req_at + req_b.size] = req_b
    buf[ids_at:ids_at + sr.ids.size] = sr.ids
    buf[non_at:non_at + keep.size] = keep
    assert ids_at % 8 == 4 and non_at % 4 == 0
    d_buf = torch.from_numpy(buf).to(dev)
    d_arena = torch.from_numpy(sr.arena).to(dev)
    d_out = torch.full((12 + 72 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_ln = torch.full((n + 3,), 0xA5, dtype=torch.uint8, device=dev)
    d_st = torch.full((n + 3,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        engine.sign_ec_tx_ids_device(d_buf.data_ptr() + ids_at, sr.n_ids, d_buf.data_ptr() + req_at, n, sr.tmpls,
                                     d_arena.data_ptr(), sr.arena.size, d_buf.data_ptr() + non_at, d_out.data_ptr() + 12,
                                     d_ln.data_ptr() + 3, d_st.data_ptr() + 3, stream=s.cuda_stream)
        got, got_ln, got_st = d_out.clone(), d_ln.clone(), d_st.clone()
    torch.cuda.synchronize()
    got, got_ln, got_st = got.cpu().numpy(), got_ln.cpu().numpy(), got_st.cpu().numpy()
    assert np.array_equal(got[12:].reshape(-1, 72), h[0]) and np.array_equal(got_ln[3:], h[1]) and np.array_equal(got_st[3:], h[2])
    assert (got[:12] == 0xA5).all() and (got_ln[:3] == 0xA5).all() and (got_st[:3] == 0xA5).all()


# 5 ---------------------------------------------------------------- statuses and the signer sets
def _raw(h, sr, nonces, fill=0xA5):
    sigs = np.full(72 * sr.n, fill, dtype=np.uint8)
    ln, st = np.full(sr.n, fill, dtype=np.uint8), np.full(sr.n, fill, dtype=np.uint8)
    rc = _lib.lib().cg_ec_sign_tx_ids(h, p_(sr.ids), sr.n_ids, p_(sr.reqs), sr.n, p_(sr.tmpls), len(sr.tmpls),
                                      p_(sr.arena), sr.arena.size, p_(nonces), p_(sigs), p_(ln), p_(st))
    return rc, sigs.reshape(-1, 72), ln, st


def test_statuses_and_the_two_signer_sets():
    from corda_amd.engine import Engine
    n2, n3 = bc.CURVES[2].n, bc.CURVES[3].n
    # signers: good k1, good r1, d = 0 (k1), d = n (r1), another scheme
    keys = [SIGNERS[0], SIGNERS[1], (2, bytes(32)), (3, n3.to_bytes(32, "big")), (4, SIGNERS[0][1])]
    k = [tuple_of(0)[3], tuple_of(1)[3]]
    #            good  good  refused signers      signer  tx_idx  template  k = 0  k = n
    tx = [tuple_of(0)[1], tuple_of(1)[1], 0, 0, 0, 0, 7, 0, 0, 0]
    sg = [0, 1, 2, 3, 4, 5, 0, 1, 0, 1]
    tm = [tuple_of(0)[2], tuple_of(1)[2], 0, 0, 0, 0, 0, 2, 0, 0]
    sr = make_sr(tx, sg, tm)
    kk = [k[0], k[1], 5, 5, 5, 5, 5, 5, 0, n3]
    nonces = np.frombuffer(b"".join(v.to_bytes(32, "big") for v in kk), dtype=np.uint8).copy()
    want = [0, 0] + [B.NOT_RUN] * 6 + [B.NONCE_REJECTED] * 2
    ed_seed = ed.entropy_seed(20)
    ed_sr = B.SignRequests(IDS, np.zeros(1, dtype=B.SIGN_REQ_DTYPE), sr.tmpls, sr.arena)
    with Engine(0) as eng:
        # no ECDSA signers: CG_ERR_ARG, nothing written -- also with an Ed25519 set loaded
        eng.load_signers([ed_seed])
        rc, sigs, ln, st = _raw(eng._h, sr, nonces)
        assert rc == -1 and (sigs == 0xA5).all() and (ln == 0xA5).all() and (st == 0xA5).all()
        assert "no ECDSA signers" in _lib.last_error()
        pubs, lst = eng.load_ec_signers(keys)
        assert list(lst) == [0, 0, B.KEY_INVALID, B.KEY_INVALID, B.UNSUPPORTED]
        assert pubs[:2] == [bc.raw_key(bc.public_point(s, d)) for (s, _), d in zip(SIGNERS[:2], D)]
        assert all(p == bytes(64) for p in pubs[2:])
        rc, sigs, ln, st = _raw(eng._h, sr, nonces)
        assert rc == 0 and list(st) == want
        for j, w in enumerate(want):
            if w:
                assert not sigs[j].any() and ln[j] == 0, "an unsigned request gets 72 zero bytes and length 0"
        check(sigs, ln, st[:2], 2)
        # the Ed25519 set is untouched by the ECDSA load, and the reverse
        e_sig, e_st = eng.sign_tx_ids(ed_sr)
        pre, suf = TEMPLATES[0]
        assert not e_st.any() and e_sig[0].tobytes() == ed.sign(ed_seed, pre + IDS[0].tobytes() + suf)
        eng.clear_signers()
        rc, sigs2, ln2, st2 = _raw(eng._h, sr, nonces)
        assert rc == 0 and np.array_equal(sigs2, sigs) and list(st2) == want
        eng.load_signers([ed_seed])
        # the arena form: the empty check first (before the signer and the nonce), a span out of range
        s3, l3, t3 = eng.sign_ec([(0, b"abc"), (9, b""), (2, b""), (9, b"abc"), (1, b"xyz" * 50)],
                                 [k[0].to_bytes(32, "big"), bytes(32), bytes(32), bytes(32), k[1].to_bytes(32, "big")])
        assert list(t3) == [0, B.EMPTY, B.EMPTY, B.NOT_RUN, 0] and not s3[1:4].any() and not l3[1:4].any()
        for j, (i, m) in ((0, (0, b"abc")), (4, (1, b"xyz" * 50))):
            w = bc.der_encode_sig(*bc.sign(SIGNERS[i][0], D[i], m, k[i]))
            assert (int(l3[j]), s3[j].tobytes()) == (len(w), H.slot(w))
        items = np.zeros(2, dtype=B.SIGN_ITEM_DTYPE)
        items["msg_off"], items["msg_len"], items["signer"] = [0, 6], [8, 3], [0, 0]
        arena = np.frombuffer(b"01234567" + bytes(8), dtype=np.uint8).copy()
        sg4, l4, st4 = np.full(144, 0xA5, np.uint8), np.full(2, 0xA5, np.uint8), np.full(2, 0xA5, np.uint8)
        two = np.frombuffer(k[0].to_bytes(32, "big") * 2, dtype=np.uint8).copy()
        assert _lib.lib().cg_ec_sign_batch(eng._h, p_(items), 2, p_(arena), 8, p_(two), p_(sg4), p_(l4), p_(st4)) == 0
        w = bc.der_encode_sig(*bc.sign(2, D[0], b"01234567", k[0]))
        assert list(st4) == [0, B.NOT_RUN] and sg4[:72].tobytes() == H.slot(w) and not sg4[72:].any() and list(l4) == [len(w), 0]
        # n == 0 is a no-op
        assert _lib.lib().cg_ec_sign_batch(eng._h, None, 0, None, 0, None, None, None, None) == 0
        # a reload replaces the set: signer 0 is now the r1 key
        pubs, lst = eng.load_ec_signers([SIGNERS[1]])
        assert not lst.any()
        one = make_sr([tuple_of(1)[1]] * 2, [0, 1], [tuple_of(1)[2]] * 2)
        kn = np.frombuffer(k[1].to_bytes(32, "big") * 2, dtype=np.uint8).copy()
        rc, sigs, ln, st = _raw(eng._h, one, kn)
        assert rc == 0 and list(st) == [0, B.NOT_RUN] and sigs[0, :ln[0]].tobytes() == oracle_sig(1)
        # cleared: CG_ERR_ARG again, nothing written; the Ed25519 set still signs
        eng.clear_ec_signers()
        rc, sigs, ln, st = _raw(eng._h, one, kn)
        assert rc == -1 and (sigs == 0xA5).all() and (st == 0xA5).all()
        eng.clear_ec_signers()  # a no-op when none is loaded
        e_sig2, e_st2 = eng.sign_tx_ids(ed_sr)
        assert not e_st2.any() and np.array_equal(e_sig2, e_sig)
        bad = np.zeros(64, dtype=np.uint8)
        assert _lib.lib().cg_ec_signers_load(eng._h, p_(bad), p_(bad), 0, p_(bad), p_(bad)) == -1
        assert _lib.lib().cg_ec_signers_load(eng._h, p_(bad), p_(bad), 65536, p_(bad), p_(bad)) == -1
    assert n2 != n3


# 6 ---------------------------------------------------------------- every fixed-base radix
@pytest.mark.parametrize("bits", [24, 22])
def test_smaller_tables_sign_the_same_bytes_for_the_crafted_k(bits):
    """The fixture's crafted-k records (k = 1, 2, n - 2, n - 1, the refusals, the short r) and every edge
    scalar, on a radix 2^24 / 2^22 context: the same bytes."""
    from corda_amd.engine import Engine
    recs = [r for r in H.records() if "msg" in r and r["msg"]]
    edges, msg = H.edges(), H.edge_msg()
    with Engine(0, table_bytes_max=_lib.lib().cg_table_bytes(bits)) as eng:
        assert eng.info()["fixed_base_bits"] == bits
        keys = _fixture_signers(eng)
        sigs, ln, st = eng.sign_ec([(keys.index((r["scheme"], r["d"])), r["msg"]) for r in recs], [r["k"] for r in recs])
        for r, sig, l, s in zip(recs, sigs, ln, st):
            assert (int(s), int(l), sig.tobytes()) == (r["status"], len(r["sig"]), H.slot(r["sig"])), r["note"]
        kidx = {s: keys.index((s, H.key(s)[0])) for s in (2, 3)}
        sigs, ln, st = eng.sign_ec([(kidx[s], msg) for s, _, _ in edges], [k for _, k, _ in edges])
        assert not st.any()
        for (s, k, dg), sig, l in zip(edges, sigs, ln):
            assert H.digest(sig[:int(l)].tobytes()) == dg, (s, k.hex())


# 7 ---------------------------------------------------------------- two caller streams, a verify between
def test_two_sign_calls_on_two_streams_with_a_verify_between(engine):
    import torch
    pubs = load(engine)
    n = 4000
    reqs = [requests(n, first=f) for f in (0, 31)]
    keep = [q[1].copy() for q in reqs]
    single = [engine.sign_ec_tx_ids(*q) for q in reqs]
    pb = _verify_batch(reqs[0][0], single[0][0], single[0][1], pubs, [s for s, _ in SIGNERS])
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    d = [dict(ids=up(sr.ids), reqs=up(sr.reqs), arena=up(sr.arena), k=up(kk),
              sigs=torch.full((72 * n,), 0xA5, dtype=torch.uint8, device=dev),
              ln=torch.full((n,), 0xA5, dtype=torch.uint8, device=dev),
              st=torch.full((n,), 255, dtype=torch.uint8, device=dev)) for (sr, _), kk in zip(reqs, keep)]
    head = np.concatenate([pb.arena, np.zeros(-pb.arena.size % 4, np.uint8)])  # the stream starts 4-aligned
    v = dict(keys=up(pb.keys), ids=up(pb.ids), sigs=up(pb.sigs), arena=up(np.concatenate([head, pb.stream])),
             st=torch.full((n,), 255, dtype=torch.uint8, device=dev))
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()

    def sign_on(i):
        sr = reqs[i][0]
        engine.sign_ec_tx_ids_device(d[i]["ids"].data_ptr(), sr.n_ids, d[i]["reqs"].data_ptr(), n, sr.tmpls,
                                     d[i]["arena"].data_ptr(), sr.arena.size, d[i]["k"].data_ptr(), d[i]["sigs"].data_ptr(),
                                     d[i]["ln"].data_ptr(), d[i]["st"].data_ptr(), stream=streams[i].cuda_stream)

    sign_on(0)
    engine.verify_tx_signatures_packed_device(v["keys"].data_ptr(), len(pb.keys), v["ids"].data_ptr(), pb.n_ids,
                                              v["sigs"].data_ptr(), n, head.size, pb.stream.size, pb.tmpls,
                                              v["arena"].data_ptr(), head.size + pb.stream.size, v["st"].data_ptr(),
                                              stream=streams[1].cuda_stream)
    sign_on(1)
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(d[i]["sigs"].cpu().numpy().reshape(-1, 72), single[i][0]), f"sign call {i}"
        assert np.array_equal(d[i]["ln"].cpu().numpy(), single[i][1]) and np.array_equal(d[i]["st"].cpu().numpy(), single[i][2])
    assert np.array_equal(v["st"].cpu().numpy(), np.full(n, B.VALID, np.uint8))
    check(*single[1], n, first=31)


# 8 ---------------------------------------------------------------- the pool: one slot, failover
def test_pool_signs_on_one_slot_and_fails_over():
    from corda_amd.engine import EnginePool
    n = 2500
    sr, nonces = requests(n)
    keep = nonces.copy()
    with EnginePool([0, 0], chunk_items=1000) as ep:
        sigs0, ln0, st0 = np.full(72 * n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
        rc = _lib.lib().cg_pool_ec_sign_tx_ids(ep._h, p_(sr.ids), sr.n_ids, p_(sr.reqs), sr.n, p_(sr.tmpls), len(sr.tmpls),
                                               p_(sr.arena), sr.arena.size, p_(keep), p_(sigs0), p_(ln0), p_(st0), None)
        assert rc == -1 and (sigs0 == 0xA5).all() and (ln0 == 0xA5).all() and (st0 == 0xA5).all()  # no signers yet
        pubs, lst = ep.load_ec_signers(SIGNERS)
        assert not lst.any() and pubs == [bc.raw_key(bc.public_point(s, d)) for (s, _), d in zip(SIGNERS, D)]
        sigs, ln, st = ep.sign_ec_tx_ids(sr, keep.copy())
        assert ep.last_stats["reruns"] == 0 and ep.last_stats["failed_slots"] == 0
        check(sigs, ln, st, n)
        ep.inject_fault(0)  # a software flag: no device fault is provoked
        sigs2, ln2, st2 = ep.sign_ec_tx_ids(sr, keep.copy())
        assert np.array_equal(sigs2, sigs) and np.array_equal(ln2, ln) and not st2.any()
        assert ep.last_stats["reruns"] == 1 and ep.last_stats["failed_slots"] == 1 and ep.last_stats["not_run"] == 0
        assert ep.healthy() == [False, True]
        ep.inject_fault(1)
        sigs3, ln3, st3 = ep.sign_ec_tx_ids(sr, keep.copy(), allow_partial=True)  # nothing healthy
        assert (st3 == B.NOT_RUN).all() and not sigs3.any() and not ln3.any() and ep.last_stats["not_run"] == n
        ep.inject_fault(0, False)
        ep.inject_fault(1, False)
        sigs4, ln4, st4 = ep.sign_ec_tx_ids(sr, keep.copy())
        assert np.array_equal(sigs4, sigs) and not st4.any() and ep.healthy() == [True, True]
        ep.clear_ec_signers()
