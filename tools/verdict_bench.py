"""What the per-transaction verdict stage costs on the headline shard (run on the GPU box).

The shard is bench.py's: 12.5M signatures drawn from a 2^20-item notary pool, the signatures of one
transaction adjacent (about 2.5M transactions of about 5), the packed device form, a warm context.
Every transaction requires one leaf key and the notary's 2-of-3 CompositeKey (one shared subtree).
Timed with HIP events on the caller's stream, alternating in one process:
  (a) cg_verify_tx_signatures_packed_device
  (b) cg_verify_required_signatures_packed_device (the same verify, then the verdict kernels)
  (c) cg_tx_verdicts_device alone, over (a)'s statuses
and the verdicts of (b) and (c) are checked against a numpy reduction of (a)'s statuses. Prints one JSON
line: medians and minima of (a), (b), (c), (b) - (a), and the stage's byte count. A library without
the verdict entry points (CORDA_AMD_LIB pointing at an older build) times (a) only: alternate the two
libraries' processes in one job to compare their (a)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spans_of(tx_idx):
    """Runs of equal tx_idx: (first record of each run, run index of each record)."""
    start = np.concatenate([[True], tx_idx[1:] != tx_idx[:-1]])
    return np.flatnonzero(start), np.cumsum(start) - 1


def numpy_verdicts(status, key_idx, first, tx_of, leaf_cls, kids):
    """(first_bad, status, leaf fulfilled, composite fulfilled) per transaction, from per-signature statuses."""
    n = len(status)
    ordinal = np.arange(n) - first[tx_of]
    bad = status != 0
    fb = np.minimum.reduceat(np.where(bad, ordinal, 0xFFFFFFFF), first)
    st = np.where(fb == 0xFFFFFFFF, 0, status[np.minimum(first + fb, n - 1)])
    leaf = np.logical_or.reduceat(key_idx == leaf_cls[tx_of], first)
    votes = sum(np.logical_or.reduceat(key_idx == k, first).astype(np.int32) for k in kids)
    return fb.astype(np.uint32), st.astype(np.uint8), leaf, votes >= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=12_500_000)
    ap.add_argument("--pool", type=int, default=1 << 20)
    ap.add_argument("--ed-keys", type=int, default=4096)
    ap.add_argument("--ec-keys", type=int, default=1024)
    ap.add_argument("--sigs-per-tx", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only-a", action="store_true", help="time (a) alone, as a library without the verdict "
                    "entry points does (the like-for-like process for comparing two libraries' (a))")
    a = ap.parse_args()

    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()  # torch's HIP runtime opens the device before the library's (tests/conftest.py)
    from corda_amd import _lib, signable
    from corda_amd import batch as B
    from corda_amd.engine import Engine
    from tools.workload import wl

    pool, _, schemes = wl.notary_pool(a.pool, ed_keys=a.ed_keys, ec_keys=a.ec_keys, seed=a.seed, nthreads=a.threads,
                                      sig_group=a.sigs_per_tx)
    ids, id_idx = wl.pool_ids(pool, len(signable.template(1, 4)[0]))
    idx = wl.tx_ordered_draws(pool.n, a.items, id_idx, seed=a.seed + 1)
    tb = wl.tx_sig_stream(pool, schemes, idx, ids, id_idx, nthreads=a.threads)
    # transaction t = the t-th run of equal ids: its own row of the id table, tx_idx == t
    first, tx_of = spans_of(tb.sigs["tx_idx"])
    n_tx = len(first)
    new_ids = tb.ids.reshape(-1, 32)[tb.sigs["tx_idx"][first]]
    tb.sigs["tx_idx"] = tx_of
    tb = B.TxSigBatch(tb.keys, new_ids, tb.sigs, tb.tmpls, tb.arena)
    pb = tb.packed()
    n_keys = len(pb.keys)
    rng = np.random.default_rng(a.seed + 2)
    key_idx = pb.sigs["key_idx"].astype(np.int64)
    # requirements: leaf roots 0 .. n_keys-1 (class = key index), then the notary's 2-of-3 and its three leaves
    leaf_cls = np.where(rng.random(n_tx) < 0.7, key_idx[first], rng.integers(0, n_keys, n_tx))
    kids = [int(k) for k in np.argsort(np.bincount(key_idx, minlength=n_keys))[-3:]]
    nodes = np.zeros(n_keys + 4, B.REQ_NODE_DTYPE)
    nodes["a"][:n_keys] = np.arange(n_keys)
    nodes[n_keys] = (n_keys + 1, 3, 0, 2)
    for j, k in enumerate(kids):
        nodes[n_keys + 1 + j] = (k, 0, 1, 0)
    reqs = np.empty(2 * n_tx, np.uint32)
    reqs[0::2], reqs[1::2] = leaf_cls, n_keys
    checks = np.zeros(n_tx, B.TX_CHECK_DTYPE)
    checks["first_sig"], checks["n_sigs"] = first, np.diff(np.concatenate([first, [pb.n]]))
    checks["first_req"], checks["n_req"] = 2 * np.arange(n_tx), 2

    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    off = -(-pb.arena.size // 16) * 16
    har = np.zeros(off + pb.stream.size, np.uint8)
    har[:pb.arena.size], har[off:] = pb.arena, pb.stream
    d = dict(k=up(pb.keys), i=up(pb.ids), s=up(pb.sigs), a=up(har), ck=up(checks), rq=up(reqs), nd=up(nodes))
    st_a = torch.full((pb.n,), 255, dtype=torch.uint8, device=dev)
    st_b = torch.full((pb.n,), 255, dtype=torch.uint8, device=dev)
    vd = [torch.zeros(8 * n_tx, dtype=torch.uint8, device=dev) for _ in range(2)]
    rs = [torch.zeros(2 * n_tx, dtype=torch.uint8, device=dev) for _ in range(2)]
    has_txv = hasattr(_lib.lib(), "cg_tx_verdicts_device") and not a.only_a
    stream = torch.cuda.Stream(device=dev)
    eng = Engine(0)
    eng.reserve(n_keys, pb.n)
    sp = stream.cuda_stream
    sig_args = (d["k"].data_ptr(), n_keys, d["i"].data_ptr(), pb.n_ids, d["s"].data_ptr(), pb.n, off, pb.stream.size,
                pb.tmpls, d["a"].data_ptr(), har.size)
    tab_args = (0, d["ck"].data_ptr(), n_tx, d["rq"].data_ptr(), len(reqs), d["nd"].data_ptr(), len(nodes))

    def call_a():
        eng.verify_tx_signatures_packed_device(*sig_args, st_a.data_ptr(), stream=sp)

    def call_b():
        eng.verify_required_signatures_packed_device(*sig_args, *tab_args, st_b.data_ptr(), vd[0].data_ptr(),
                                                     rs[0].data_ptr(), stream=sp)

    def call_c():
        eng.tx_verdicts_device(d["s"].data_ptr(), 12, pb.n, st_a.data_ptr(), d["k"].data_ptr(), n_keys, 0,
                               d["ck"].data_ptr(), n_tx, d["rq"].data_ptr(), len(reqs), d["nd"].data_ptr(), len(nodes),
                               vd[1].data_ptr(), rs[1].data_ptr(), stream=sp)

    calls = {"a": call_a, "b": call_b, "c": call_c} if has_txv else {"a": call_a}
    ms = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for r in range(a.warmup + a.rounds):
            for name, fn in calls.items():  # alternating: a, b, c, a, b, c, ...
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if r >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    out = {"lib": os.path.basename(_lib.LIB_PATH), "n_sigs": int(pb.n), "n_tx": int(n_tx), "n_keys": int(n_keys),
           "rounds": a.rounds}
    for name, v in ms.items():
        out[f"ms_{name}"] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
                             "all": [round(float(x), 4) for x in v]}
    out["msigs_per_s_a"] = round(pb.n / np.median(ms["a"]) / 1e3, 2)
    if has_txv:
        t0 = time.time()
        status = st_a.cpu().numpy()
        fb, st, leaf, comp = numpy_verdicts(status, key_idx, first, tx_of, leaf_cls, kids)
        want_rs = np.empty(2 * n_tx, np.uint8)
        want_rs[0::2], want_rs[1::2] = np.where(leaf, 0, 1), np.where(comp, 0, 1)
        ok = bool(np.array_equal(st_b.cpu().numpy(), status))
        for k in range(2):
            got = vd[k].cpu().numpy().view(B.TX_VERDICT_DTYPE)
            ok &= bool(np.array_equal(got["first_bad"], fb) and np.array_equal(got["status"], st) and
                       not got["flags"].any() and
                       np.array_equal(got["n_missing"], (~leaf).astype(np.uint16) + (~comp).astype(np.uint16)) and
                       np.array_equal(rs[k].cpu().numpy(), want_rs))
        out["verdicts_match_numpy"] = ok
        out["numpy_reduction_s"] = round(time.time() - t0, 2)
        out["tx_with_bad_signature"] = int(np.count_nonzero(fb != 0xFFFFFFFF))
        out["req_missing"] = int(np.count_nonzero(want_rs))
        out["ms_b_minus_a"] = round(float(np.median(ms["b"]) - np.median(ms["a"])), 4)
        # what the stage moves: 13 B per signature (record + status), 24 + 8 B per transaction, the requirement
        # entries and their status bytes (4 + 1 B each, written twice: preset, result), the node table once
        traffic = 13 * pb.n + 32 * n_tx + (4 + 2) * len(reqs) + nodes.nbytes
        out["stage_bytes"] = int(traffic)
        out["stage_gb_per_s_c"] = round(traffic / np.median(ms["c"]) / 1e6, 1)
    eng.close()
    print(json.dumps(out))
    return 0 if out.get("verdicts_match_numpy", True) else 1


if __name__ == "__main__":
    sys.exit(main())
