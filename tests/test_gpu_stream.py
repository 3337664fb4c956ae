"""GPU tests of the streaming paths (include/cordagpu.h, ABI v2):
  * chunked verify calls: one key-table build, items in chunks (device and host-buffer forms,
    arena windows copied by extent, any item order / layout), against the C oracle;
  * a BASELINE configs[4]-shaped call of more than 8M items through cg_verify_batch (the JNI
    path): every occurrence of a pool item gets the pool item's verdict, and the pool's verdicts
    equal the C oracle's;
  * async device calls on two streams sharing one context (ordered by the context);
  * cg_pool on one GPU (two contexts on device 0), including a drill fault and its re-run;
  * every other device form on a caller's stream, behind two calls the library refuses."""
import numpy as np
import pytest

from corda_amd import batch as B
from oracle import c_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    from tools.workload import wl
    b, labels, schemes = wl.notary_pool(1 << 16, ed_keys=512, ec_keys=128, seed=77, nthreads=16)
    ref = c_oracle.verify_batch(b, B.MODE_DOVERIFY, 16)
    return b, labels, schemes, ref


def test_chunked_device_and_host_paths(pool):
    import torch
    from corda_amd.batch import Batch
    from corda_amd.engine import Engine
    b, labels, schemes, ref = pool
    # reverse the item order: chunk extents then run backwards through the arena
    rb = Batch(b.keys, b.items[::-1].copy(), b.arena)
    with Engine(0, chunk_items=7001) as eng:
        st = eng.verify(b)
        assert np.array_equal(st, ref), f"host path: {np.count_nonzero(st != ref)} mismatches"
        st_r = eng.verify(rb)
        assert np.array_equal(st_r, ref[::-1]), "host path, reversed items"
        dev = torch.device("cuda", 0)
        kd = torch.from_numpy(b.keys.view(np.uint8)).to(dev)
        idd = torch.from_numpy(b.items.view(np.uint8)).to(dev)
        ad = torch.from_numpy(b.arena).to(dev)
        sd = torch.full((b.n,), 255, dtype=torch.uint8, device=dev)
        eng.verify_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size, sd.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(sd.cpu().numpy(), ref), "device path"


def test_host_window_keys_after_items(pool):
    """Keys stored behind every item in the arena: the window spans both; verdicts unchanged."""
    from corda_amd.batch import Batch
    from corda_amd.engine import Engine
    b, _, _, ref = pool
    keys = b.keys.copy()
    parts, off = [b.arena], b.arena.size
    for j in range(len(keys)):
        o, n = int(keys[j]["off"]), int(keys[j]["len"])
        pad = (-off) % 4
        parts.append(np.zeros(pad, np.uint8))
        off += pad
        parts.append(b.arena[o:o + n])
        keys[j]["off"] = off
        off += n
    b2 = Batch(keys, b.items, np.concatenate(parts + [np.zeros(64, np.uint8)]))
    with Engine(0, chunk_items=9000) as eng:
        assert np.array_equal(eng.verify(b2), ref)


def test_notary_shard_over_8m_items_one_call(pool):
    """> 8M items (BASELINE configs[4] per-GPU shape, 70/20/10) in ONE cg_verify_batch call: several
    device chunks and host pipeline chunks. Bit-exact at full size through idempotence: each item
    is a draw from the pool, so its verdict must equal the pool item's, which equals the oracle's."""
    from corda_amd.engine import Engine
    from tools.workload import wl
    b, labels, _, ref = pool
    n = 8_400_000
    big, idx = wl.index_stream(b, n, seed=5)
    with Engine(0) as eng:
        st = eng.verify(big)
    assert not np.any(st == B.NOT_RUN)
    bad = np.nonzero(st != ref[idx])[0]
    assert bad.size == 0, f"{bad.size} of {n} verdicts differ from the oracle's verdict on the same pool item"
    assert np.all(st[labels[idx] == 0] == B.VALID)


def test_async_calls_on_two_streams_share_one_context(pool):
    """two device calls enqueued back to back on different streams of one context share
    its workspace; the context orders them, so both results are exact."""
    import torch
    from corda_amd.batch import Batch
    from corda_amd.engine import Engine
    b, _, _, ref = pool
    dev = torch.device("cuda", 0)
    half = b.n // 2
    parts = [Batch(b.keys, b.items[:half].copy(), b.arena), Batch(b.keys, b.items[half:].copy(), b.arena)]
    kd = torch.from_numpy(b.keys.view(np.uint8)).to(dev)
    ad = torch.from_numpy(b.arena).to(dev)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    with Engine(0) as eng:
        outs = []
        for p, s in zip(parts, streams):
            idd = torch.from_numpy(p.items.view(np.uint8)).to(dev)
            sd = torch.full((p.n,), 255, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            outs.append((idd, sd))
        for (idd, sd), p, s in zip(outs, parts, streams):
            eng.verify_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), p.n, ad.data_ptr(), b.arena.size,
                              sd.data_ptr(), stream=s.cuda_stream)
        torch.cuda.synchronize()
        got = np.concatenate([sd.cpu().numpy() for _, sd in outs])
    assert np.array_equal(got, ref)


def test_pool_two_contexts_and_drill_fault(pool):
    from corda_amd._lib import EngineUnavailable
    from corda_amd.engine import EnginePool
    b, _, _, ref = pool
    with EnginePool([0, 0], chunk_items=20000) as ep:
        assert np.array_equal(ep.verify(b), ref)
        assert ep.last_stats["shards"] == 2 and ep.last_stats["reruns"] == 0
        ep.inject_fault(1)
        assert np.array_equal(ep.verify(b), ref)           # slot 1's shard re-ran on slot 0
        assert ep.last_stats["reruns"] == 1 and ep.healthy() == [True, False]
        assert np.array_equal(ep.verify(b), ref)           # unhealthy slot skipped
        assert ep.last_stats["shards"] == 1
        ep.inject_fault(0)
        st = ep.verify(b, allow_partial=True)              # nothing healthy: every item NOT_RUN
        assert np.all(st == B.NOT_RUN)
        with pytest.raises(EngineUnavailable):
            ep.verify(b)
        ep.inject_fault(0, False)
        ep.inject_fault(1, False)
        assert ep.healthy() == [True, True]
        assert np.array_equal(ep.verify(b), ref)


def test_prepared_keys_survive_the_caller_reusing_its_key_bytes():
    """cg_prepare_keys_device ends with the context's stream behind the side streams' decodes and
    table builds, so its end on the caller's stream is the end of its reads of the caller's key
    bytes, and the next call may rewrite the key workspace (the launch schedule). On one
    caller stream, with no pause: prepare key set A, prepare key set B (as many keys, other bytes),
    fill the arena B was prepared from with 0xFF, then verify B's items over a second arena, in
    which the key bytes are 0xFF too (no item stage reads key bytes: k_ec_prep and k_ed_hash take
    the key from the key workspace). Thousands of keys per family keep the decodes in flight while
    the fill is enqueued.
    This is the end-to-end witness of what tests/test_launch_schedule.py proves on the CPU. It
    depends on timing: without the joins a kind schedule still gives the oracle's verdicts, and an
    unkind one gives CG_KEY_INVALID verdicts, never worse (the one run made without them had 5983 of
    the 8192 verdicts wrong)."""
    import torch
    from corda_amd.engine import Engine
    from tools.workload import wl
    a, _, _ = wl.notary_pool(1 << 12, ed_keys=3000, ec_keys=2000, seed=901, nthreads=16)
    b, _, _ = wl.notary_pool(1 << 13, ed_keys=3000, ec_keys=2000, seed=902, nthreads=16)
    assert len(a.keys) == len(b.keys) >= 7000 and not np.array_equal(a.arena[:4096], b.arena[:4096])
    ref = c_oracle.verify_batch(b, B.MODE_DOVERIFY, 16)
    assert (ref == B.VALID).any() and (ref == B.INVALID).any()
    items_arena = b.arena.copy()
    for k in b.keys:
        items_arena[int(k["off"]):int(k["off"]) + int(k["len"])] = 0xFF
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    ka, aa, kb, ab, ib, ab2 = (up(x) for x in (a.keys, a.arena, b.keys, b.arena, b.items, items_arena))
    sd = torch.full((b.n,), 255, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with Engine(0, chunk_items=3000) as eng:
        with torch.cuda.stream(s):
            eng.prepare_keys_device(ka.data_ptr(), len(a.keys), aa.data_ptr(), a.arena.size, stream=s.cuda_stream)
            eng.prepare_keys_device(kb.data_ptr(), len(b.keys), ab.data_ptr(), b.arena.size, stream=s.cuda_stream)
            ab.fill_(0xFF)
            aa.fill_(0xFF)
            eng.verify_items_device(kb.data_ptr(), len(b.keys), ib.data_ptr(), b.n, ab2.data_ptr(), b.arena.size,
                                    sd.data_ptr(), stream=s.cuda_stream)
            got = sd.clone()
        torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} of {b.n} verdicts differ from the oracle's"


def test_device_forms_on_a_caller_stream():
    """Every device form no other test runs on a caller's stream: cg_prepare_keys_device +
    cg_verify_items_device, cg_sha256_batch_device, cg_tx_ids_device, cg_verify_transactions_device,
    cg_verify_tx_signatures_device (24-byte table) and cg_verify_filtered_device, each on a torch side
    stream with a clone() of its result enqueued on that stream right behind it and no synchronisation
    in between; every result equals the host form's and the oracle's. chunk_items=1500: a call over the
    2^12-item pool has three chunks and uses both item workspaces. Before them, two calls the library
    refuses (CG_ERR_ARG) on the same stream, which must leave the stream and the context usable."""
    import hashlib
    import torch
    import test_filtered
    from corda_amd import _lib, merkle as M, signable
    from corda_amd.engine import Engine
    from oracle import corda as ocorda
    from tools.workload import wl
    pool, _, schemes = wl.notary_pool(1 << 12, ed_keys=24, ec_keys=12, seed=515, nthreads=16, sig_group=4)
    ref = c_oracle.verify_batch(pool, B.MODE_DOVERIFY, 16)
    assert (ref == B.VALID).any() and (ref == B.INVALID).any()
    ids, id_idx = wl.pool_ids(pool, len(signable.template(1, 4)[0]))
    idx = np.random.default_rng(516).permutation(pool.n)
    tb = wl.tx_sig_stream(pool, schemes, idx, ids, id_idx, nthreads=16)
    pb = tb.packed()
    w = wl.tx_pipeline(300, n_keys=37, seed=517, corrupt_permille=80, nthreads=16)
    ftxs, fwant = test_filtered.random_tearoffs(300)
    ft, fn, fl, fa = M.pack_filtered(ftxs)
    msgs = [np.random.default_rng(518).integers(0, 256, n, dtype=np.uint8).tobytes() for n in range(0, 400)]
    spans, sarena = Engine._spans(msgs)

    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    out = lambda n: torch.full((n,), 255, dtype=torch.uint8, device=dev)  # noqa: E731
    L = _lib.lib()
    got = {}
    d = {k: up(v) for k, v in dict(
        keys=pool.keys, items=pool.items, arena=pool.arena, spans=spans, sarena=sarena, txs=w.txs, comps=w.comps,
        wkeys=w.keys, wsigs=w.sigs, warena=w.arena, tkeys=tb.keys, tids=tb.ids, tsigs=tb.sigs, tarena=tb.arena,
        psigs=pb.sigs, ft=ft, fn=fn, fl=fl, fa=fa).items()}
    o = dict(ist=out(pool.n), sha=out(32 * len(msgs)), ids=out(32 * len(w.txs)), idst=out(len(w.txs)),
             wids=out(32 * len(w.txs)), wtx=out(len(w.txs)), wsig=out(len(w.sigs)), tsig=out(tb.n), psig=out(pb.n),
             ftx=out(len(ft)))
    p = {k: v.data_ptr() for k, v in {**d, **o}.items()}
    s = torch.cuda.Stream(device=dev)
    st = s.cuda_stream
    torch.cuda.synchronize()
    with Engine(0, chunk_items=1500) as eng:
        with torch.cuda.stream(s):
            # refused: items before any prepare on this context; a signature stream outside the arena
            with pytest.raises(_lib.EngineUnavailable, match=r"\(-1\).*not prepared"):
                eng.verify_items_device(p["keys"], len(pool.keys), p["items"], pool.n, p["arena"], pool.arena.size,
                                        o["ist"].data_ptr(), stream=st)
            with pytest.raises(_lib.EngineUnavailable, match=r"\(-1\).*outside the arena"):
                eng.verify_tx_signatures_packed_device(p["tkeys"], len(pb.keys), p["tids"], pb.n_ids, p["psigs"], pb.n,
                                                       tb.arena.size - 8, pb.stream.size, pb.tmpls, p["tarena"],
                                                       tb.arena.size, p["psig"], stream=st)
            # the good call behind them: exact verdicts
            eng.verify_tx_signatures_packed_device(p["tkeys"], len(pb.keys), p["tids"], pb.n_ids, p["psigs"], pb.n,
                                                   pb.arena.size, pb.stream.size, pb.tmpls, p["tarena"], tb.arena.size,
                                                   p["psig"], stream=st)
            got["psig"] = o["psig"].clone()
            eng.prepare_keys_device(p["keys"], len(pool.keys), p["arena"], pool.arena.size, stream=st)
            eng.verify_items_device(p["keys"], len(pool.keys), p["items"], pool.n, p["arena"], pool.arena.size,
                                    o["ist"].data_ptr(), stream=st)
            got["items"] = o["ist"].clone()
            _lib.check(L.cg_sha256_batch_device(eng._h, p["spans"], len(msgs), p["sarena"], sarena.size - 8, p["sha"], st),
                       "cg_sha256_batch_device")
            got["sha"] = o["sha"].clone()
            _lib.check(L.cg_tx_ids_device(eng._h, p["txs"], len(w.txs), p["comps"], len(w.comps), p["warena"],
                                          w.arena.size, p["ids"], p["idst"], st), "cg_tx_ids_device")
            got["ids"], got["idst"] = o["ids"].clone(), o["idst"].clone()
            eng.verify_transactions_device(p["txs"], len(w.txs), p["comps"], len(w.comps), p["wkeys"], len(w.keys),
                                           p["wsigs"], len(w.sigs), w.tmpls, p["warena"], w.arena.size, p["wids"],
                                           p["wtx"], p["wsig"], stream=st)
            got["wids"], got["wtx"], got["wsig"] = o["wids"].clone(), o["wtx"].clone(), o["wsig"].clone()
            eng.verify_tx_signatures_device(p["tkeys"], len(tb.keys), p["tids"], tb.n_ids, p["tsigs"], tb.n, tb.tmpls,
                                            p["tarena"], tb.arena.size, p["tsig"], stream=st)
            got["tsig"] = o["tsig"].clone()
            eng.verify_filtered_device(p["ft"], len(ft), p["fn"], len(fn), p["fl"], len(fl), p["fa"], fa.size, p["ftx"],
                                       stream=st)
            got["ftx"] = o["ftx"].clone()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        # the host forms, on the same context
        h_items = eng.verify(pool)
        h_sha = eng.sha256(msgs)
        h_ids, h_idst = eng.tx_ids(w.txs, w.comps, w.arena)
        h_wids, h_wtx, h_wsig = eng.verify_transactions(w.txs, w.comps, w.keys, w.sigs, w.tmpls, w.arena)
        h_tsig = eng.verify_tx_signatures(tb)
        h_ftx = eng.verify_filtered(ft, fn, fl, fa)
    for name, host, oracle in (("psig", h_tsig, ref[idx]), ("items", h_items, ref), ("tsig", h_tsig, ref[idx]),
                               ("ftx", h_ftx, fwant), ("idst", h_idst, np.zeros(len(w.txs), np.uint8)),
                               ("wtx", h_wtx, np.zeros(len(w.txs), np.uint8)),
                               ("ids", h_ids.reshape(-1), w.ids.reshape(-1)),
                               ("wids", h_wids.reshape(-1), w.ids.reshape(-1)),
                               ("wsig", h_wsig, np.where(w.labels == 0, B.VALID, B.INVALID).astype(np.uint8))):
        assert np.array_equal(got[name], oracle), f"{name}: {np.count_nonzero(got[name] != oracle)} differ from the oracle"
        assert np.array_equal(got[name], host), f"{name}: {np.count_nonzero(got[name] != host)} differ from the host form"
    assert [got["sha"][32 * i:32 * i + 32].tobytes() for i in range(len(msgs))] == h_sha == \
        [hashlib.sha256(m).digest() for m in msgs]
    a = w.arena.tobytes()
    for t in range(0, len(w.txs), 29):  # the generator's ids are the oracle's
        r = w.txs[t]
        blobs = [a[c["off"]:c["off"] + c["len"]] for c in w.comps[r["first"]:r["first"] + r["n"]]]
        assert ocorda.tx_id(blobs[:-1], a[r["salt_off"]:r["salt_off"] + 32], blobs[-1]) == w.ids[t].tobytes()
    assert np.count_nonzero(w.labels) > 0 and len(np.unique(fwant)) == 3
