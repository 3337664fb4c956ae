"""Throughput of tear-off building on one GPU: Engine.build_filtered_device (cg_build_filtered_device) on
transactions resident in HBM, timed with HIP events (DESIGN.md §3 "Tear-off building"), next to two other
figures from the same run on the same transactions:

  * the host path it replaces: merkle.merkle_tree (one SHA-256 batch call per tree level) and then
    PartialMerkleTree.build, per transaction, through the same engine (wall clock, leaf hashes given);
  * Engine.tx_ids_device (cg_tx_ids_device): the same leaf and node hashes without the tear-off.

The shape is tools/workload/wl.py's tear-off shape (1 + Poisson(1) inputs, Poisson(3) outputs, 1 + Poisson(3)
commands, notary, components of 80..600 bytes) plus a time window, filtered as NotaryFlow.Client does:
inputs and the time window stay visible. `--unique` transactions are generated and their rows tiled to
`--txs` (the component rows are copied, the bytes are shared). Every transaction must build, and the first
`--check` of them are compared with the oracle. One JSON line.

  python tools/tearoff_build_bench.py --steps 20 --warmup 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from corda_amd import batch as B  # noqa: E402
from corda_amd import merkle as M  # noqa: E402


def transactions(n_unique, seed=5, comp_len=(80, 600)):
    """[(blobs, salt32, salt_blob)] and the NotaryFlow.Client masks."""
    rng = np.random.default_rng(seed)
    txs, masks = [], []
    for _ in range(n_unique):
        n_in, n_out, n_cmd = 1 + rng.poisson(1), rng.poisson(3), 1 + rng.poisson(3)
        n = n_in + n_out + n_cmd + 2  # + notary, time window
        blobs = [rng.integers(0, 256, int(rng.integers(comp_len[0], comp_len[1] + 1)), dtype=np.uint8).tobytes()
                 for _ in range(n)]
        salt = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        txs.append((blobs, salt, b"\x01" + salt))
        masks.append([1] * n_in + [0] * (n - n_in - 1) + [1])
    return txs, masks


def tile(t, c, vis, n_tx):
    """The tables repeated to n_tx transactions: every copy has component rows of its own."""
    reps = (n_tx + len(t) - 1) // len(t)
    tt, cc = np.tile(t, reps), np.tile(c, reps)
    tt["first"] += np.repeat(np.arange(reps, dtype=np.uint64) * len(c), len(t))
    keep = int(tt[n_tx - 1]["first"]) + int(tt[n_tx - 1]["n"])
    return np.ascontiguousarray(tt[:n_tx]), np.ascontiguousarray(cc[:keep]), np.tile(vis, reps)[:keep].copy()


def timed(stream, steps, warmup, call):
    import torch
    ms = []
    for step in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        stream.synchronize()
        if step >= warmup:
            ms.append(e0.elapsed_time(e1))
    return np.array(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique", type=int, default=4096)
    ap.add_argument("--txs", type=int, default=1 << 17)
    ap.add_argument("--host-txs", type=int, default=256, help="transactions the host path is timed on")
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import hashlib

    import torch
    torch.cuda.init()
    from corda_amd.engine import Engine
    dev = torch.device("cuda", 0)
    txs, masks = transactions(a.unique)
    t0, c0, arena = M.pack_transactions(txs)
    t, c, vis = tile(t0, c0, M.pack_visible(txs, masks), a.txs)
    n_tx, n_comps = len(t), len(c)
    node_cap, leaf_cap, out_cap = 4 * n_comps, n_comps, 32 * (n_tx + 3 * n_comps)  # the bound that is always enough
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    buf = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)  # noqa: E731
    d_t, d_c, d_v = up(t), up(c), up(vis)
    d_a = up(np.concatenate([arena, np.zeros(-arena.size % 4, np.uint8)]))
    d_f, d_n, d_l, d_o = buf(40 * n_tx), buf(16 * node_cap), buf(24 * leaf_cap), buf(out_cap)
    d_s, d_tot, d_ids, d_ist = buf(n_tx), buf(32), buf(32 * n_tx), buf(n_tx)
    with Engine(0) as eng:
        stream = torch.cuda.Stream(device=dev)  # not the legacy default stream: the events bracket the call

        def build():
            eng.build_filtered_device(d_t.data_ptr(), n_tx, d_c.data_ptr(), n_comps, d_a.data_ptr(), arena.size,
                                      d_v.data_ptr(), 0, d_f.data_ptr(), d_n.data_ptr(), node_cap, d_l.data_ptr(),
                                      leaf_cap, d_o.data_ptr(), out_cap, d_s.data_ptr(), d_tot.data_ptr(),
                                      stream.cuda_stream)

        def ids():
            eng.tx_ids_device(d_t.data_ptr(), n_tx, d_c.data_ptr(), n_comps, d_a.data_ptr(), arena.size,
                              d_ids.data_ptr(), d_ist.data_ptr(), stream.cuda_stream)

        ms_build = timed(stream, a.steps, a.warmup, build)
        ms_ids = timed(stream, a.steps, a.warmup, ids)
        tot = d_tot.cpu().numpy().view(B.BUILD_TOTALS_DTYPE)[0]
        assert not d_s.cpu().numpy().any() and not d_ist.cpu().numpy().any() and int(tot["over"]) == 0
        out, ftxs = d_o.cpu().numpy(), d_f.cpu().numpy().view(B.FTX_DTYPE)
        assert np.array_equal(out[ftxs["root_off"].astype(np.int64)[:, None] + np.arange(32)], d_ids.cpu().numpy().reshape(-1, 32))
        # the host path on the first transactions, leaf hashes given; its trees are the check of the device's
        nodes = d_n.cpu().numpy().view(B.PMT_NODE_DTYPE)
        hashes = []
        for blobs, salt, salt_blob in txs[:a.host_txs]:
            nonce = [hashlib.sha256(salt + i.to_bytes(4, "big")).digest() for i in range(len(blobs))]
            hashes.append([hashlib.sha256(b + x).digest() for b, x in zip(blobs, nonce)] +
                          [hashlib.sha256(salt_blob).digest()])
        w0 = time.perf_counter()
        host = []
        for hs, mask in zip(hashes, masks):
            tree = M.merkle_tree(hs, eng)
            host.append((tree.hash, M.PartialMerkleTree.build(tree, [h for h, v in zip(hs, mask) if v])))
        host_s = time.perf_counter() - w0
        for k, (root, pmt) in enumerate(host[:a.check]):
            f = ftxs[k]
            rows = nodes[int(f["first_node"]):int(f["first_node"]) + int(f["n_nodes"])]
            got = [(int(r["kind"]), None if r["kind"] == B.PMT_NODE else out[int(r["hash_off"]):int(r["hash_off"]) + 32].tobytes())
                   for r in rows]
            assert got == pmt.postorder() and out[int(f["root_off"]):int(f["root_off"]) + 32].tobytes() == root, k
    med_b, med_i = float(np.median(ms_build)), float(np.median(ms_ids))
    print(json.dumps({"txs": n_tx, "components": n_comps, "visible": int(tot["n_leaves"]), "nodes": int(tot["n_nodes"]),
                      "out_bytes": int(tot["out_bytes"]), "steps": a.steps, "warmup": a.warmup,
                      "build_ms_median": round(med_b, 3), "build_ms_min": round(float(ms_build.min()), 3),
                      "build_ms_max": round(float(ms_build.max()), 3),
                      "build_tx_per_s": round(n_tx / (med_b * 1e-3)),
                      "tx_ids_ms_median": round(med_i, 3), "tx_ids_ms_min": round(float(ms_ids.min()), 3),
                      "tx_ids_ms_max": round(float(ms_ids.max()), 3),
                      "tx_ids_tx_per_s": round(n_tx / (med_i * 1e-3)),
                      "build_over_tx_ids": round(med_b / med_i, 3),
                      "host_path_txs": len(host), "host_path_tx_per_s": round(len(host) / host_s, 1)}), flush=True)


if __name__ == "__main__":
    main()
