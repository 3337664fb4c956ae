"""GPU tests of the per-transaction verdicts (cg_tx_verdicts(_device), cg_verify_required_signatures_packed
(_device), cg_pool_verify_required_signatures_packed): TransactionWithSignatures.verifySignaturesExcept
reduced on the device.

The kernels' reference is the host build of the same lane logic (corda_amd/csrc/txverdict.h through
tests/native/txverdict_test.cpp), which tests/test_txverdict.py checks against a restatement of the
rules; the fused calls' statuses are the C oracle's on the materialised SignableData."""
import numpy as np
import pytest

from corda_amd import batch as B
from oracle import c_oracle

import txsig_util
import txverdict_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(engine):
    """The session's engine (tests/conftest.py: torch's HIP runtime opens the device before the library's)."""
    return engine


def _gpu(eng, c):
    return eng.tx_verdicts(c.sigs, c.status, c.keys, c.checks, c.reqs, c.nodes, c.key_class)


# ---------------------------------------------------------------- 1. the kernels on synthetic statuses
@pytest.mark.parametrize("stride", [12, 24])
@pytest.mark.parametrize("with_class", [False, True])
def test_kernels_equal_the_cpu_lane_function(eng, stride, with_class):
    """Spans of 0-9 signatures for n_tx around the wave and block sizes, the small / wave boundary (32,
    33, 64, 65 signatures), 5 000-signature spans whose only bad status is the last / the first, and
    the malformed tables (all but the visit-budget DAG), for both record strides, key_class NULL and given."""
    for n_tx in (0, 1, 63, 64, 65, 2049):
        c = C.random_case(100 + n_tx, n_tx, stride, with_class)
        C.assert_same(_gpu(eng, c), C.run_native(c), what=f"n_tx {n_tx}")
    c = C.boundary_case(3, stride, with_class)
    want = C.run_native(c)
    assert want[0][7].tolist()[:2] == (4999, B.INVALID) and want[0][9].tolist()[:2] == (0, B.NOT_RUN)
    C.assert_same(_gpu(eng, c), want, what="boundary")
    C.assert_same(want, C.run_native(c, 64), what="boundary, the wave form on the CPU")
    c = C.hostile_case(stride, with_class)
    C.assert_same(_gpu(eng, c), C.run_native(c), c.names, "malformed tables")


def test_device_form_on_a_stream_and_argument_errors(eng):
    """cg_tx_verdicts_device on a torch stream (a cg_tx_check with reserved != 0 comes back SPAN_BAD there;
    the host form refuses it), results visible to work enqueued on that stream afterwards; CG_ERR_ARG
    for a bad stride, a non-zero reserved and NULL tables with non-zero counts."""
    import ctypes
    import torch
    from corda_amd import _lib
    c = C.hostile_case(12, True, reserved=True)
    want = C.run_native(c)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    d = {k: up(getattr(c, k)) for k in ("sigs", "status", "keys", "key_class", "checks", "reqs", "nodes")}
    vd = torch.zeros(8 * len(c.checks), dtype=torch.uint8, device=dev)
    rs = torch.zeros(len(c.reqs), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        eng.tx_verdicts_device(d["sigs"].data_ptr(), 12, len(c.sigs), d["status"].data_ptr(), d["keys"].data_ptr(),
                               len(c.keys), d["key_class"].data_ptr(), d["checks"].data_ptr(), len(c.checks),
                               d["reqs"].data_ptr(), len(c.reqs), d["nodes"].data_ptr(), len(c.nodes), vd.data_ptr(),
                               rs.data_ptr(), stream=s.cuda_stream)
        vd2, rs2 = vd.clone(), rs.clone()
    torch.cuda.synchronize()
    C.assert_same((vd2.cpu().numpy().view(B.TX_VERDICT_DTYPE), rs2.cpu().numpy()), want, c.names, "device form")
    L, h, p = _lib.lib(), eng._h, lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out_v, out_r = np.zeros(len(c.checks), B.TX_VERDICT_DTYPE), np.zeros(len(c.reqs), np.uint8)

    def call(stride=12, checks=c.checks, nodes=p(c.nodes), reqs=p(c.reqs)):
        return L.cg_tx_verdicts(h, p(c.sigs), stride, len(c.sigs), p(c.status), p(c.keys), len(c.keys), p(c.key_class),
                                p(checks), len(checks), reqs, len(c.reqs), nodes, len(c.nodes), p(out_v), p(out_r))

    assert call() == -1 and "reserved" in _lib.last_error()
    ok = c.checks.copy()
    ok["reserved"] = 0
    assert call(checks=ok) == 0
    assert call(stride=16, checks=ok) == -1 and "sig_stride" in _lib.last_error()
    assert call(checks=ok, nodes=None) == -1 and call(checks=ok, reqs=None) == -1


# ---------------------------------------------------------------- 2. the fused call, real signatures
@pytest.fixture(scope="module")
def notary():
    """~20 000 draws over a 4 096-item signable pool, grouped into ~4 000 transactions of up to 5 signatures
    over one id, one leaf and one 2-of-3 composite requirement each; statuses from the C oracle on the
    materialised SignableData, verdicts from the CPU lane function over those."""
    from corda_amd import signable
    from tools.workload import wl
    pool, labels, schemes = wl.notary_pool(1 << 12, ed_keys=64, ec_keys=16, seed=404, nthreads=16, sig_group=4)
    ids, id_idx = wl.pool_ids(pool, len(signable.template(1, 4)[0]))
    rng = np.random.default_rng(405)
    idx = rng.integers(0, pool.n, 20_000)
    idx = idx[np.argsort(id_idx[idx], kind="stable")]
    tb = wl.tx_sig_stream(pool, schemes, idx, ids, id_idx, nthreads=16)
    of_id = id_idx[idx].astype(np.int64)
    run = np.arange(len(idx)) - np.searchsorted(of_id, of_id, side="left")  # ordinal among the draws of its id
    start = (run % 5) == 0
    tx_of = np.cumsum(start) - 1
    n_tx = int(tx_of[-1]) + 1
    sigs = tb.sigs.copy()
    sigs["tx_idx"] = tx_of
    tb = B.TxSigBatch(tb.keys, ids[of_id[start]], sigs, tb.tmpls, tb.arena)
    status = c_oracle.verify_batch(txsig_util.to_message_batch(tb), B.MODE_DOVERIFY, 16)
    assert 0.05 < np.mean(status != B.VALID) < 0.5
    n_keys = len(tb.keys)
    nodes = np.zeros(2 * n_tx + 3 * n_tx, B.REQ_NODE_DTYPE)  # per transaction a leaf root and a 2-of-3 root, then the blocks
    signer = sigs["key_idx"][np.flatnonzero(start)]
    nodes["a"][0:2 * n_tx:2] = np.where(rng.random(n_tx) < 0.7, signer, rng.integers(0, n_keys, n_tx))
    nodes["a"][1:2 * n_tx:2] = 2 * n_tx + 3 * np.arange(n_tx)
    nodes["n_children"][1:2 * n_tx:2] = 3
    nodes["threshold"][1:2 * n_tx:2] = 2
    kids = rng.integers(0, n_keys, (n_tx, 3))
    kids[:, 0] = signer
    last = sigs["key_idx"][np.concatenate([np.flatnonzero(start)[1:], [len(idx)]]) - 1]
    kids[:, 1] = np.where(rng.random(n_tx) < 0.6, last, kids[:, 1])
    nodes["a"][2 * n_tx:] = kids.reshape(-1)
    nodes["weight"][2 * n_tx:] = 1
    checks = np.zeros(n_tx, B.TX_CHECK_DTYPE)
    checks["first_sig"] = np.flatnonzero(start)
    checks["n_sigs"] = np.bincount(tx_of, minlength=n_tx)
    checks["first_req"], checks["n_req"] = 2 * np.arange(n_tx), 2
    reqs = np.arange(2 * n_tx, dtype=np.uint32)
    pb = tb.packed()
    c = C.case(pb.sigs, status, pb.keys, None, checks, reqs, nodes)
    want = C.run_native(c)
    assert 3500 < n_tx < 6000 and len(np.unique(want[0]["status"])) >= 3
    for code in (B.REQ_FULFILLED, B.REQ_MISSING):
        assert np.count_nonzero(want[1][0::2] == code) > 200 and np.count_nonzero(want[1][1::2] == code) > 200
    return tb, pb, c, status, want


@pytest.mark.parametrize("chunk", [0, 4001])
def test_fused_call_equals_the_reduced_oracle_statuses(eng, notary, chunk):
    """Host form with and without status_out and the device form on a torch stream, in one verify chunk
    and in chunks of 4 001 signatures that spans straddle (a verdict kernel launched before the last
    chunk had finished would read statuses not yet written)."""
    import torch
    from corda_amd.engine import Engine
    tb, pb, c, status, want = notary
    with Engine(0, chunk_items=chunk) as eng:  # a second context on the device, with its own chunk size
        vd, rs = eng.verify_required_signatures_packed(pb, c.checks, c.reqs, c.nodes)
        C.assert_same((vd, rs), want, what=f"host form, status_out NULL, chunk {chunk}")
        vd, rs, st = eng.verify_required_signatures_packed(pb, c.checks, c.reqs, c.nodes, want_status=True)
        assert np.array_equal(st, status)
        C.assert_same((vd, rs), want, what=f"host form, chunk {chunk}")
        dev = torch.device("cuda", 0)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
        kd, ijd, sgd, ad = up(pb.keys), up(pb.ids), up(pb.sigs), up(tb.arena)
        ckd, rqd, ndd = up(c.checks), up(c.reqs), up(c.nodes)
        s = torch.cuda.Stream(device=dev)
        sd = torch.full((pb.n,), 255, dtype=torch.uint8, device=dev)
        vdd = torch.zeros(8 * len(c.checks), dtype=torch.uint8, device=dev)
        rsd = torch.zeros(len(c.reqs), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            eng.verify_required_signatures_packed_device(
                kd.data_ptr(), len(pb.keys), ijd.data_ptr(), pb.n_ids, sgd.data_ptr(), pb.n, pb.arena.size,
                pb.stream.size, pb.tmpls, ad.data_ptr(), tb.arena.size, 0, ckd.data_ptr(), len(c.checks),
                rqd.data_ptr(), len(c.reqs), ndd.data_ptr(), len(c.nodes), sd.data_ptr(), vdd.data_ptr(),
                rsd.data_ptr(), stream=s.cuda_stream)
            got = vdd.clone(), rsd.clone(), sd.clone()  # enqueued on the caller's stream right after the call
        torch.cuda.synchronize()
        assert np.array_equal(got[2].cpu().numpy(), status)
        C.assert_same((got[0].cpu().numpy().view(B.TX_VERDICT_DTYPE), got[1].cpu().numpy()), want,
                      what=f"device form, chunk {chunk}")


# ---------------------------------------------------------------- 3. a 2-of-3 composite notary key
def test_composite_notary_with_genuine_signatures(eng):
    """Genuine Ed25519 signatures over SignableData under a 2-of-3 CompositeKey requirement: two signers
    fulfil it; one signer leaves it MISSING, with the serial path's SignaturesMissingException out of
    verify_signatures_except_batch; a tampered second signature is first_bad = 1 / INVALID with the
    fulfilment bytes still reported; a template index out of range gives a NOT_RUN verdict."""
    from corda_amd import signable, transactions as T
    from corda_amd.composite import CompositeKey
    from corda_amd.crypto import PublicKey, SignatureException, TransactionSignature, _Crypto
    from oracle import ed25519_i2p as ed
    rng = np.random.default_rng(31)
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(4)]
    pubs = [ed.public_from_seed(s) for s in seeds]
    raw = [PublicKey(4, p, B.KEY_RAW) for p in pubs]
    notary = CompositeKey.Builder().add_keys(*raw[:3]).build(2)

    def stx(t, who, tamper=None):
        tx_id = bytes([t + 1]) * 32
        sigs = []
        for j, k in enumerate(who):
            sb = ed.sign(seeds[k], signable.serialize(tx_id, 1, 4))
            if tamper == j:
                sb = sb[:10] + bytes([sb[10] ^ 1]) + sb[11:]
            # the second signer names its key by the SPKI form: equal to the raw key the requirement holds
            by = raw[k] if j == 0 else PublicKey(4, bytes.fromhex("302a300506032b6570032100") + pubs[k], B.KEY_SPKI)
            sigs.append(TransactionSignature(sb, by))
        return T.SignedTransaction(tx_id, sigs, {notary, raw[3]}, [T.Command("Move", (raw[3],))], notary)

    stxs = [stx(0, [0, 2, 3]), stx(1, [1, 3]), stx(2, [0, 1, 3], tamper=1), stx(3, [2, 1, 3])]
    ids = [s.id for s in stxs]
    pb, checks, reqs, nodes, key_class, req_keys, req_errors = T.pack_required_signatures(stxs, ids)
    assert not req_errors and len(set(key_class)) == 4 and len(key_class) > 4
    vd, rs = eng.verify_required_signatures_packed(pb, checks, reqs, nodes, key_class)

    def req_of(t):
        first = int(checks[t]["first_req"])
        return {k: int(rs[first + r]) for r, k in enumerate(req_keys[t])}

    assert vd[0].tolist() == (B.NO_BAD, B.VALID, 0, 0) and set(req_of(0).values()) == {B.REQ_FULFILLED}
    assert vd[1].tolist() == (B.NO_BAD, B.VALID, 0, 1)
    assert req_of(1) == {notary: B.REQ_MISSING, raw[3]: B.REQ_FULFILLED}
    assert vd[2].tolist() == (1, B.INVALID, 0, 0) and set(req_of(2).values()) == {B.REQ_FULFILLED}
    assert vd[3].tolist() == (B.NO_BAD, B.VALID, 0, 0)
    crypto = _Crypto()
    crypto.use_engine(eng)
    got = T.verify_signatures_except_batch(stxs, None, (), crypto)
    assert got[0] is None and got[3] is None
    assert isinstance(got[1], T.SignaturesMissingException) and got[1].missing == {notary} and got[1].id == ids[1]
    assert got[1].descriptions == ["notary"]
    assert type(got[2]) is SignatureException and str(got[2]) == "Signature Verification failed!"
    # an out-of-range template on transaction 3's second signature
    pb.sigs["tmpl"][int(checks[3]["first_sig"]) + 1] = 40
    vd, rs = eng.verify_required_signatures_packed(pb, checks, reqs, nodes, key_class)
    assert vd[3].tolist() == (1, B.NOT_RUN, 0, 0) and vd[0].tolist() == (B.NO_BAD, B.VALID, 0, 0)


# ---------------------------------------------------------------- 4. the pool form
def test_pool_form_with_a_drill_fault(eng, notary):
    from corda_amd.engine import EnginePool
    tb, pb, c, status, want = notary
    with EnginePool([0, 0], chunk_items=3000) as ep:
        vd, rs, st = ep.verify_required_signatures_packed(pb, c.checks, c.reqs, c.nodes, want_status=True)
        assert ep.last_stats["shards"] == 2 and np.array_equal(st, status)
        C.assert_same((vd, rs), want, what="pool")
        ep.inject_fault(0)
        vd, rs = ep.verify_required_signatures_packed(pb, c.checks, c.reqs, c.nodes)
        assert ep.last_stats["reruns"] == 1
        C.assert_same((vd, rs), want, what="pool after the re-run")
