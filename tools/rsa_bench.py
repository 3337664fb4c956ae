"""Throughput of RSA_SHA256 (RSASSA-PSS) verification on one GPU: Engine(rsa=True).verify_device on an
RSA-only batch resident in HBM, timed with HIP events (DESIGN.md "RSA_SHA256 on the GPU").

Per modulus size: `--keys` keys from the OpenSSL CLI, `--sigs` messages signed with them (Python
integers, corda_amd/hostverify.rsa_pss_sign) and tiled to `--items` items; nothing is cached per
signature, so every item is the full work. Every verdict must be VALID. One JSON line per size.

Key generation and signing take minutes at 4096 bits and need no GPU: `--prepare-only --cache FILE`
makes them once, a later run with the same `--cache` loads them.

  python tools/rsa_bench.py --cache /tmp/rsa_bench.json --prepare-only
  python tools/rsa_bench.py --cache /tmp/rsa_bench.json --steps 10 --warmup 2

The host figure to compare with: `openssl speed -multi 16 rsa2048 rsa3072 rsa4096` (verify/s).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from corda_amd import batch as B  # noqa: E402
from corda_amd import hostverify  # noqa: E402


def gen_key(bits, d):
    key = os.path.join(d, "k.pem")
    subprocess.run(["openssl", "genpkey", "-algorithm", "RSA", "-pkeyopt", f"rsa_keygen_bits:{bits}", "-out", key],
                   check=True, capture_output=True)
    pub = subprocess.run(["openssl", "pkey", "-in", key, "-pubout", "-outform", "DER"], check=True,
                         capture_output=True).stdout
    txt = subprocess.run(["openssl", "pkey", "-in", key, "-text", "-noout"], check=True,
                         capture_output=True).stdout.decode()
    body = txt.split("privateExponent:")[1].split("prime1")[0]
    return pub, int("".join(body.split()).replace(":", ""), 16)


def prepare(bits, n_keys, n_sigs, seed):
    rng = np.random.default_rng(seed)
    keys, sigs = [], []
    with tempfile.TemporaryDirectory() as d:
        for _ in range(n_keys):
            keys.append(gen_key(bits, d))
    for j in range(n_sigs):
        spki, dd = keys[j % n_keys]
        n, _ = hostverify.rsa_decode_key(spki)
        msg = rng.integers(0, 256, 270, dtype=np.uint8).tobytes()  # a SignableData-sized message
        sig = hostverify.rsa_pss_sign(n, dd, msg, rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
        sigs.append((j % n_keys, sig.hex(), msg.hex()))
    return {"keys": [k.hex() for k, _ in keys], "sigs": sigs}


def build_batch(data, n_items):
    bb = B.BatchBuilder()
    kidx = [bb.key(1, B.KEY_SPKI, bytes.fromhex(k)) for k in data["keys"]]
    base = [bb.add(kidx[k], bytes.fromhex(s), bytes.fromhex(m)) for k, s, m in data["sigs"]]
    b = bb.build()
    reps = (n_items + len(base) - 1) // len(base)
    items = np.tile(b.items, reps)[:n_items]
    return B.Batch(b.keys, np.ascontiguousarray(items), b.arena)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[2048, 3072, 4096])
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--sigs", type=int, default=256)
    ap.add_argument("--items", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cache", default="")
    ap.add_argument("--prepare-only", action="store_true")
    a = ap.parse_args()
    cache = {}
    if a.cache and os.path.exists(a.cache):
        cache = json.load(open(a.cache))
    for bits in a.bits:
        tag = f"{bits}/{a.keys}/{a.sigs}"
        if tag not in cache:
            t0 = time.time()
            cache[tag] = prepare(bits, a.keys, a.sigs, bits)
            print(f"# prepared {tag} in {time.time() - t0:.1f} s", file=sys.stderr)
            if a.cache:
                json.dump(cache, open(a.cache, "w"))
    if a.prepare_only:
        return
    import torch
    torch.cuda.init()
    from corda_amd import _lib
    from corda_amd.engine import Engine
    dev = torch.device("cuda", 0)
    with Engine(0, table_bytes_max=int(_lib.lib().cg_table_bytes(22)), rsa=True) as eng:
        for bits in a.bits:
            b = build_batch(cache[f"{bits}/{a.keys}/{a.sigs}"], a.items)
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
            kd, idd, ad = up(b.keys), up(b.items), up(b.arena)
            sd = torch.full((b.n,), 255, dtype=torch.uint8, device=dev)
            eng.reserve(len(b.keys), b.n)
            stream = torch.cuda.Stream(device=dev)  # not the legacy default stream: the events bracket the call
            ms = []
            for step in range(a.warmup + a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                eng.verify_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size,
                                  sd.data_ptr(), B.MODE_DOVERIFY, stream.cuda_stream)
                e1.record(stream)
                stream.synchronize()
                if step >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
            st = sd.cpu().numpy()
            assert (st == B.VALID).all(), np.bincount(st, minlength=6).tolist()
            ms = np.array(ms)
            print(json.dumps({"bits": bits, "keys": len(b.keys), "items": b.n, "steps": a.steps,
                              "ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(ms.min()), 3),
                              "ms_max": round(float(ms.max()), 3),
                              "sigs_per_s": round(b.n / (float(np.median(ms)) * 1e-3))}), flush=True)


if __name__ == "__main__":
    main()
