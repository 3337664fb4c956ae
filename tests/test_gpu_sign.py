"""GPU tests of the Ed25519 signer (cg_signers_load, cg_sign_batch, cg_sign_tx_ids and its device and
pool forms): every signature byte for byte what the Python oracle (RFC 8032, i2p EdDSAEngine.engineSign)
writes, the statuses, the chunk, wave, block and inversion-batch edges, every fixed-base radix, the
ordering with verify calls on one context, and the pool's failover.

The r of a signature is a hash output, so these tests cannot steer it to the fixed-base table's digit
edges; tests/test_sign_host.py holds those on the CPU and test_gpu_scalar_edges.py on the GPU through
crafted-S verifies over the same table."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from corda_amd import _lib, signable
from corda_amd import batch as B
from oracle import ed25519_i2p as ed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ED_FINISH_K = 16  # corda_amd/csrc/sign_ed.hip: items per lane of the batched inversion
REAL = signable.template(1, 4)
OTHER = (b"\x01\x00other-metadata-prefix:", b"\x07\x08")
SEEDS3 = [ed.entropy_seed(n) for n in (20, 70, 80)]


def records():
    with open(os.path.join(HERE, "golden", "ed25519_sign.json")) as f:
        return json.load(f)["records"]


def make_sr(ids, tx_idx, signer, tmpl, templates):
    """SignRequests over `ids` ([n_ids, 32] uint8) from request columns and (prefix, suffix) templates."""
    b = B.SignRequestBuilder()
    for pre, suf in templates:
        b.template(pre, suf)
    base = b.build()
    assert len(base.tmpls) == len(templates)
    reqs = np.zeros(len(tx_idx), dtype=B.SIGN_REQ_DTYPE)
    reqs["tx_idx"], reqs["signer"], reqs["tmpl"] = tx_idx, signer, tmpl
    return B.SignRequests(ids, reqs, base.tmpls, base.arena)


def rand_ids(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


_oracle = {}


def oracle_sig(seed, templates, tmpl, tx_id):
    """The oracle's signature over prefix || id || suffix, computed once per distinct input."""
    k = (seed, templates[tmpl], bytes(tx_id))
    if k not in _oracle:
        pre, suf = templates[tmpl]
        _oracle[k] = ed.sign(seed, pre + bytes(tx_id) + suf)
    return _oracle[k]


def check_against_oracle(sr, sigs, seeds, templates, which):
    for j in which:
        q = sr.reqs[j]
        want = oracle_sig(seeds[int(q["signer"])], templates, int(q["tmpl"]), sr.ids.reshape(-1, 32)[int(q["tx_idx"])])
        assert sigs[j].tobytes() == want, f"request {j}"


# 1 ---------------------------------------------------------------- the fixture
def test_fixture_records_byte_equal(engine):
    recs = records()
    seeds = sorted({r["seed"] for r in recs})
    pubs = engine.load_signers([bytes.fromhex(s) for s in seeds])
    for s, p in zip(seeds, pubs):
        assert {r["pub"] for r in recs if r["seed"] == s} == {p.hex()}
    msgs = [r for r in recs if "msg" in r]
    sigs, st = engine.sign([(seeds.index(r["seed"]), bytes.fromhex(r["msg"])) for r in msgs])
    for r, sig, s in zip(msgs, sigs, st):
        assert (int(s), sig.tobytes().hex()) == (r["status"], r["sig"]), r["note"]
    assert sorted(set(int(s) for s in st)) == [0, B.EMPTY]
    spl = [r for r in recs if "prefix" in r]
    b = B.SignRequestBuilder()
    for r in spl:
        t = b.template(bytes.fromhex(r["prefix"]), bytes.fromhex(r["suffix"]))
        b.add_request(seeds.index(r["seed"]), b.tx_id(bytes.fromhex(r["id"])), t)
    sr = b.build()
    assert len(sr.tmpls) == 15
    sigs, st = engine.sign_tx_ids(sr)
    for r, sig, s in zip(spl, sigs, st):
        assert (int(s), sig.tobytes().hex()) == (0, r["sig"]), r["note"]


# 2 ---------------------------------------------------------------- wave, block and inversion-batch edges
@pytest.mark.parametrize("n", sorted({1, 63, 64, 65, 255, 257, 1023, 1025, 64 * ED_FINISH_K - 1, 64 * ED_FINISH_K + 1}))
def test_counts_match_oracle(engine, n):
    """Signers cycle over 3 keys; the (signer, id, template) triples cycle over 3 x 67 x 2 distinct ones,
    so every signature is compared with the oracle and the oracle signs each distinct one once."""
    assert engine.load_signers(SEEDS3) == [ed.public_from_seed(s) for s in SEEDS3]
    ids = rand_ids(67, 1)
    j = np.arange(n)
    templates = [REAL, OTHER]
    sr = make_sr(ids, j % 67, j % 3, (j // 201) % 2, templates)
    sigs, st = engine.sign_tx_ids(sr)
    assert not st.any()
    check_against_oracle(sr, sigs, SEEDS3, templates, range(n))


# 3 ---------------------------------------------------------------- several chunks, then verified on the GPU
def _verify_batch(sr, sigs, pubs):
    """The signatures as cg_verify_tx_signatures_packed input over the same ids and templates."""
    keys = np.zeros(len(pubs), dtype=B.KEY_DTYPE)
    head = b"".join(pubs)
    keys["off"], keys["len"] = 32 * np.arange(len(pubs)), 32
    keys["scheme"], keys["fmt"] = B.EDDSA_ED25519_SHA512, B.KEY_RAW
    tmpls = sr.tmpls.copy()
    tmpls["prefix_off"] += len(head)
    tmpls["suffix_off"] += len(head)
    arena = np.concatenate([np.frombuffer(head, dtype=np.uint8), sr.arena])
    s12 = np.zeros(sr.n, dtype=B.TXSIG12_DTYPE)
    s12["tx_idx"], s12["key_idx"], s12["tmpl"], s12["sig_len"] = sr.reqs["tx_idx"], sr.reqs["signer"], sr.reqs["tmpl"], 64
    return B.PackedTxSigBatch(keys, sr.ids, s12, np.ascontiguousarray(sigs).reshape(-1), tmpls, arena)


def test_150k_requests_over_four_chunks_sign_then_verify():
    from corda_amd.engine import Engine
    from oracle import c_oracle
    n, n_ids, chunk = 150_000, 50_000, 40_001
    seeds = [hashlib.sha256(b"signer %d" % k).digest() for k in range(64)]
    templates = [REAL, OTHER]
    rng = np.random.default_rng(2024)
    ids = rand_ids(n_ids, 7)
    sr = make_sr(ids, rng.integers(0, n_ids, n), rng.integers(0, 64, n), rng.integers(0, 2, n), templates)
    with Engine(0, chunk_items=chunk) as eng:
        pubs = eng.load_signers(seeds)
        assert pubs[:4] == [ed.public_from_seed(s) for s in seeds[:4]]
        sigs, st = eng.sign_tx_ids(sr)
        assert not st.any()
        per = -(-n // -(-n // chunk))  # equal chunks of at most `chunk` (txsig_plan.h equal_chunk)
        assert per == 37_500
        edge = [j for f in range(0, n, per) for j in list(range(f, f + 8)) + list(range(min(f + per, n) - 8, min(f + per, n)))]
        sample = np.random.default_rng(99).choice(n, 256, replace=False)
        check_against_oracle(sr, sigs, seeds, templates, sorted(set(edge) | set(int(j) for j in sample)))
        # every one of them verifies on the same context, and not vacuously
        pb = _verify_batch(sr, sigs, pubs)
        assert np.array_equal(eng.verify_tx_signatures_packed(pb), np.full(n, B.VALID, np.uint8))
        flipped = ids.copy()
        flipped[:, 5] ^= 0x10
        bad = B.PackedTxSigBatch(pb.keys, flipped, pb.sigs, pb.stream, pb.tmpls, pb.arena)
        assert np.array_equal(eng.verify_tx_signatures_packed(bad), np.full(n, B.INVALID, np.uint8))
    # a 20 000-item sample, materialised, through the C oracle
    pick = np.sort(np.random.default_rng(5).choice(n, 20_000, replace=False))
    bb = B.BatchBuilder()
    kidx = [bb.key(B.EDDSA_ED25519_SHA512, B.KEY_RAW, p) for p in pubs]
    for j in pick:
        q = sr.reqs[j]
        pre, suf = templates[int(q["tmpl"])]
        bb.add(kidx[int(q["signer"])], sigs[j].tobytes(), pre + ids[int(q["tx_idx"])].tobytes() + suf)
    assert np.array_equal(c_oracle.verify_batch(bb.build(), B.MODE_DOVERIFY, 16), np.full(len(pick), B.VALID, np.uint8))


# 4 ---------------------------------------------------------------- host form against device form
def test_device_form_equals_host_form_at_odd_offsets(engine):
    import torch
    engine.load_signers(SEEDS3)
    n = 3001
    j = np.arange(n)
    templates = [REAL, OTHER]
    sr = make_sr(rand_ids(500, 3), (j * 7) % 500, j % 3, j % 2, templates)
    h_sigs, h_st = engine.sign_tx_ids(sr)
    dev = torch.device("cuda", 0)
    # the request table at an odd multiple of its 8 bytes, the ids at an odd multiple of 4 bytes, inside
    # one larger buffer; the signatures at an odd multiple of 4 bytes of theirs
    req_b, ids_b = sr.reqs.view(np.uint8), sr.ids
    req_at, ids_at = 8 * 5, 8 * 5 + req_b.size + 4 * 7
    buf = np.full(ids_at + ids_b.size + 64, 0xEE, dtype=np.uint8)
    buf[req_at:req_at + req_b.size] = req_b
    buf[ids_at:ids_at + ids_b.size] = ids_b
    d_buf = torch.from_numpy(buf).to(dev)
    d_arena = torch.from_numpy(sr.arena).to(dev)
    d_out = torch.full((12 + 64 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        engine.sign_tx_ids_device(d_buf.data_ptr() + ids_at, sr.n_ids, d_buf.data_ptr() + req_at, n, sr.tmpls,
                                  d_arena.data_ptr(), sr.arena.size, d_out.data_ptr() + 12, d_st.data_ptr(),
                                  stream=s.cuda_stream)
        got, got_st = d_out.clone(), d_st.clone()
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(got[12:].reshape(-1, 64), h_sigs) and np.array_equal(got_st.cpu().numpy(), h_st)
    assert (got[:12] == 0xA5).all() and not h_st.any()
    check_against_oracle(sr, h_sigs, SEEDS3, templates, range(0, n, 97))


# 5 ---------------------------------------------------------------- statuses
def _raw_sign_tx_ids(h, sr, fill=0xA5):
    sigs = np.full(64 * sr.n, fill, dtype=np.uint8)
    st = np.full(sr.n, fill, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None  # noqa: E731
    rc = _lib.lib().cg_sign_tx_ids(h, p(sr.ids), sr.n_ids, p(sr.reqs), sr.n, p(sr.tmpls), len(sr.tmpls), p(sr.arena),
                                   sr.arena.size, p(sigs), p(st))
    return rc, sigs.reshape(-1, 64), st


def test_statuses_and_the_signer_set():
    from corda_amd.engine import Engine
    templates = [REAL, OTHER]
    ids = rand_ids(4, 11)
    #        good  signer  tx_idx  template  good
    tx = [0, 1, 4, 2, 3]
    sg = [0, 3, 1, 2, 2]
    tm = [0, 0, 1, 2, 1]
    sr = make_sr(ids, tx, sg, tm, templates)
    want = [0, B.NOT_RUN, B.NOT_RUN, B.NOT_RUN, 0]
    with Engine(0) as eng:
        # no signers: CG_ERR_ARG, nothing written
        rc, sigs, st = _raw_sign_tx_ids(eng._h, sr)
        assert rc == -1 and (sigs == 0xA5).all() and (st == 0xA5).all() and "no signers" in _lib.last_error()
        eng.load_signers(SEEDS3)
        rc, sigs, st = _raw_sign_tx_ids(eng._h, sr)
        assert rc == 0 and list(st) == want
        for j, w in enumerate(want):
            if w:
                assert not sigs[j].any(), "an unsigned request gets 64 zero bytes"
        check_against_oracle(sr, sigs, SEEDS3, templates, [0, 4])
        # a template outside the arena
        out = B.SignRequests(sr.ids, sr.reqs[[0, 4]].copy(), sr.tmpls.copy(), sr.arena)
        out.tmpls["suffix_off"][1] = sr.arena.size - 1
        rc, sigs2, st2 = _raw_sign_tx_ids(eng._h, out)
        assert rc == 0 and list(st2) == [0, B.NOT_RUN] and not sigs2[1].any() and np.array_equal(sigs2[0], sigs[0])
        # the arena form: an empty message, a signer and a span out of range
        s2, t2 = eng.sign([(0, b"abc"), (1, b""), (3, b"abc"), (2, b"xyz" * 50)])
        assert list(t2) == [0, B.EMPTY, B.NOT_RUN, 0] and not s2[1].any() and not s2[2].any()
        assert s2[0].tobytes() == ed.sign(SEEDS3[0], b"abc") and s2[3].tobytes() == ed.sign(SEEDS3[2], b"xyz" * 50)
        items = np.zeros(2, dtype=B.SIGN_ITEM_DTYPE)
        items["msg_off"], items["msg_len"], items["signer"] = [0, 6], [8, 3], [0, 0]
        arena = np.frombuffer(b"01234567" + bytes(8), dtype=np.uint8).copy()
        sg3, st3 = np.full(128, 0xA5, np.uint8), np.full(2, 0xA5, np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        assert _lib.lib().cg_sign_batch(eng._h, p(items), 2, p(arena), 8, p(sg3), p(st3)) == 0
        assert list(st3) == [0, B.NOT_RUN] and sg3[:64].tobytes() == ed.sign(SEEDS3[0], b"01234567") and not sg3[64:].any()
        # n == 0 is a no-op
        assert _lib.lib().cg_sign_batch(eng._h, None, 0, None, 0, None, None) == 0
        # a reload replaces the set
        pubs = eng.load_signers([SEEDS3[2]])
        assert pubs == [ed.public_from_seed(SEEDS3[2])]
        one = make_sr(ids, [0, 0], [0, 1], [0, 0], templates)
        rc, sigs, st = _raw_sign_tx_ids(eng._h, one)
        assert rc == 0 and list(st) == [0, B.NOT_RUN]
        assert sigs[0].tobytes() == oracle_sig(SEEDS3[2], templates, 0, ids[0])
        # cleared: CG_ERR_ARG again, nothing written
        eng.clear_signers()
        rc, sigs, st = _raw_sign_tx_ids(eng._h, one)
        assert rc == -1 and (sigs == 0xA5).all() and (st == 0xA5).all()
        eng.clear_signers()  # a no-op when none is loaded
        bad = np.zeros(32, dtype=np.uint8)
        assert _lib.lib().cg_signers_load(eng._h, p(bad), 0, p(bad)) == -1
        assert _lib.lib().cg_signers_load(eng._h, p(bad), 65536, p(bad)) == -1


def test_sign_batch_messages_at_every_byte_phase(engine):
    """cg_sign_batch over a raw cg_sign_item table whose messages start at every offset mod 4 (Engine.sign
    packs them 4-aligned): the funnel-shift realignment of both prefix hashes, at lengths on either side
    of the SHA-512 padding boundaries, the last message ending at the arena's last byte."""
    engine.load_signers(SEEDS3)
    rng = np.random.default_rng(12)
    msgs, chunks, off = [], [], 0
    for ln in (1, 2, 3, 47, 48, 79, 80, 111, 112, 127, 128, 129, 175, 176, 303, 304):
        for phase in (1, 2, 3, 0):
            pad = (phase - off) % 4
            chunks.append(bytes(pad))
            off += pad
            m = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
            msgs.append((off, m))
            chunks.append(m)
            off += ln
    arena_len = off
    arena = np.frombuffer(b"".join(chunks) + bytes(8), dtype=np.uint8).copy()
    items = np.zeros(len(msgs), dtype=B.SIGN_ITEM_DTYPE)
    items["msg_off"], items["msg_len"] = [o for o, _ in msgs], [len(m) for _, m in msgs]
    items["signer"] = np.arange(len(msgs)) % 3
    assert sorted(set(int(o) % 4 for o in items["msg_off"])) == [0, 1, 2, 3]
    assert int(items["msg_off"][-1]) + int(items["msg_len"][-1]) == arena_len
    sigs, st = np.full(64 * len(msgs), 0xA5, np.uint8), np.full(len(msgs), 0xA5, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert _lib.lib().cg_sign_batch(engine._h, p(items), len(msgs), p(arena), arena_len, p(sigs), p(st)) == 0
    assert not st.any()
    for j, (o, m) in enumerate(msgs):
        assert sigs[64 * j:64 * j + 64].tobytes() == ed.sign(SEEDS3[j % 3], m), (o % 4, len(m))


# 6 ---------------------------------------------------------------- every fixed-base radix
@pytest.mark.parametrize("bits", [24, 22])
def test_smaller_tables_sign_the_same_bytes(engine, bits):
    from corda_amd.engine import Engine
    engine.load_signers(SEEDS3)
    j = np.arange(2048)
    sr = make_sr(rand_ids(256, bits), j % 256, j % 3, j % 2, [REAL, OTHER])
    want, st = engine.sign_tx_ids(sr)
    assert not st.any()
    with Engine(0, table_bytes_max=_lib.lib().cg_table_bytes(bits)) as eng:
        assert eng.info()["fixed_base_bits"] == bits
        assert eng.load_signers(SEEDS3) == [ed.public_from_seed(s) for s in SEEDS3]
        got, st = eng.sign_tx_ids(sr)
    assert not st.any() and np.array_equal(got, want)
    check_against_oracle(sr, got, SEEDS3, [REAL, OTHER], range(0, 2048, 41))


# 7 ---------------------------------------------------------------- two caller streams, a verify between
def test_two_sign_calls_on_two_streams_with_a_verify_between(engine):
    import torch
    pubs = engine.load_signers(SEEDS3)
    templates = [REAL, OTHER]
    n = 20_000
    j = np.arange(n)
    srs = [make_sr(rand_ids(999, 40 + k), (j * (3 + k)) % 999, (j + k) % 3, j % 2, templates) for k in range(2)]
    single = [engine.sign_tx_ids(sr) for sr in srs]
    pb = _verify_batch(srs[0], single[0][0], pubs)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    d = [dict(ids=up(sr.ids), reqs=up(sr.reqs), arena=up(sr.arena),
              sigs=torch.full((64 * n,), 0xA5, dtype=torch.uint8, device=dev),
              st=torch.full((n,), 255, dtype=torch.uint8, device=dev)) for sr in srs]
    head = np.concatenate([pb.arena, np.zeros(-pb.arena.size % 4, np.uint8)])  # the stream starts 4-aligned
    v = dict(keys=up(pb.keys), ids=up(pb.ids), sigs=up(pb.sigs), arena=up(np.concatenate([head, pb.stream])),
             st=torch.full((n,), 255, dtype=torch.uint8, device=dev))
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()

    def sign_on(k):
        engine.sign_tx_ids_device(d[k]["ids"].data_ptr(), srs[k].n_ids, d[k]["reqs"].data_ptr(), n, srs[k].tmpls,
                                  d[k]["arena"].data_ptr(), srs[k].arena.size, d[k]["sigs"].data_ptr(),
                                  d[k]["st"].data_ptr(), stream=streams[k].cuda_stream)

    sign_on(0)
    engine.verify_tx_signatures_packed_device(v["keys"].data_ptr(), len(pb.keys), v["ids"].data_ptr(), pb.n_ids,
                                              v["sigs"].data_ptr(), n, head.size, pb.stream.size, pb.tmpls,
                                              v["arena"].data_ptr(), head.size + pb.stream.size, v["st"].data_ptr(),
                                              stream=streams[1].cuda_stream)
    sign_on(1)
    torch.cuda.synchronize()
    for k in range(2):
        assert np.array_equal(d[k]["sigs"].cpu().numpy().reshape(-1, 64), single[k][0]), f"sign call {k}"
        assert np.array_equal(d[k]["st"].cpu().numpy(), single[k][1])
    assert np.array_equal(v["st"].cpu().numpy(), np.full(n, B.VALID, np.uint8))
    check_against_oracle(srs[1], single[1][0], SEEDS3, templates, range(0, n, 331))


# 8 ---------------------------------------------------------------- the pool: one slot, failover
def test_pool_signs_on_one_slot_and_fails_over():
    from corda_amd.engine import EnginePool
    templates = [REAL, OTHER]
    j = np.arange(5000)
    sr = make_sr(rand_ids(300, 8), j % 300, j % 3, j % 2, templates)
    with EnginePool([0, 0], chunk_items=2000) as ep:
        sigs0 = np.full(64 * sr.n, 0xA5, dtype=np.uint8)
        st0 = np.full(sr.n, 0xA5, dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        rc = _lib.lib().cg_pool_sign_tx_ids(ep._h, p(sr.ids), sr.n_ids, p(sr.reqs), sr.n, p(sr.tmpls), len(sr.tmpls),
                                            p(sr.arena), sr.arena.size, p(sigs0), p(st0), None)
        assert rc == -1 and (sigs0 == 0xA5).all() and (st0 == 0xA5).all()  # no signers yet
        assert ep.load_signers(SEEDS3) == [ed.public_from_seed(s) for s in SEEDS3]
        sigs, st = ep.sign_tx_ids(sr)
        assert not st.any() and ep.last_stats["reruns"] == 0 and ep.last_stats["failed_slots"] == 0
        check_against_oracle(sr, sigs, SEEDS3, templates, range(0, sr.n, 13))
        ep.inject_fault(0)
        sigs2, st2 = ep.sign_tx_ids(sr)
        assert np.array_equal(sigs2, sigs) and not st2.any()
        assert ep.last_stats["reruns"] == 1 and ep.last_stats["failed_slots"] == 1 and ep.last_stats["not_run"] == 0
        assert ep.healthy() == [False, True]
        ep.inject_fault(1)
        sigs3, st3 = ep.sign_tx_ids(sr, allow_partial=True)  # nothing healthy: NOT_RUN, zero bytes
        assert (st3 == B.NOT_RUN).all() and not sigs3.any() and ep.last_stats["not_run"] == sr.n
        ep.inject_fault(0, False)
        ep.inject_fault(1, False)
        sigs4, st4 = ep.sign_tx_ids(sr)
        assert np.array_equal(sigs4, sigs) and not st4.any() and ep.healthy() == [True, True]
        ep.clear_signers()
