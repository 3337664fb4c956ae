"""The Ed25519 signer's rate on one MI355X against the verify path over the same signatures (run on the
GPU box): cg_sign_tx_ids_device for 2^22 requests over the real SignableData template, with 1 signer and
with 64, inputs resident in HBM; then cg_verify_tx_signatures_packed_device over the signatures the
64-signer call wrote, on the same warm context: the yardstick.

Timed with device events on the caller's stream around `--steps` calls after `--warmup` warm-up calls,
the whole sequence (sign 1, sign 64, verify) repeated `--repeats` times, alternating, in one process.
Before timing, 256 seeded signatures of each sign call are compared with the Python oracle and the
verify call's statuses are all CG_VALID. Writes one JSON object (--out, default
profiles/sign/sign_bench.json) and prints it:
  msigs_per_s: per leg, every repeat's rate, their median, min and max
  accept: median sign rate (64 signers) >= median verify rate - (max - min of the verify repeats)
  d2h_bytes_per_signature: 64 (the host form copies 64 B of signature and 1 status byte back per request)
The share of a sign call in each of its five kernels comes from a kernel trace of this tool run with
--sign-only --repeats 1, in a run of its own (its kernel statistics are kept beside the JSON)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1 << 22)
    ap.add_argument("--ids", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sign-only", action="store_true", help="the 64-signer sign leg alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign", "sign_bench.json"))
    a = ap.parse_args()

    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()  # torch's HIP runtime opens the device before the library's (tests/conftest.py)
    from corda_amd import _lib, signable
    from corda_amd import batch as B
    from corda_amd.engine import Engine
    from oracle import ed25519_i2p as ed

    n = a.requests
    pre, suf = signable.template(1, 4)
    rng = np.random.default_rng(a.seed)
    ids = rng.integers(0, 256, (a.ids, 32), dtype=np.uint8)
    seeds = [hashlib.sha256(b"sign_bench signer %d" % k).digest() for k in range(64)]
    sb = B.SignRequestBuilder()
    sb.template(pre, suf)
    base = sb.build()
    reqs = {}
    for ns in (1, 64):
        r = np.zeros(n, dtype=B.SIGN_REQ_DTYPE)
        r["tx_idx"], r["signer"] = rng.integers(0, a.ids, n), rng.integers(0, ns, n)
        reqs[ns] = r

    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    d_ids, d_arena = up(ids), up(base.arena)
    d_reqs = {ns: up(r) for ns, r in reqs.items()}
    d_sigs = {ns: torch.zeros(64 * n, dtype=torch.uint8, device=dev) for ns in (1, 64)}
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    eng = Engine(0)
    pubs = eng.load_signers(seeds)

    def sign(ns):
        eng.sign_tx_ids_device(d_ids.data_ptr(), a.ids, d_reqs[ns].data_ptr(), n, base.tmpls, d_arena.data_ptr(),
                               base.arena.size, d_sigs[ns].data_ptr(), d_st.data_ptr(), stream=sp)

    # correctness first: a seeded sample of each sign call against the oracle
    with torch.cuda.stream(stream):
        for ns in (1, 64):
            sign(ns)
            torch.cuda.synchronize()
            assert not d_st.cpu().numpy().any(), "a request was not signed"
            got = d_sigs[ns].cpu().numpy().reshape(-1, 64)
            for j in np.random.default_rng(a.seed + ns).choice(n, 256, replace=False):
                q = reqs[ns][j]
                want = ed.sign(seeds[int(q["signer"])], pre + ids[int(q["tx_idx"])].tobytes() + suf)
                assert got[j].tobytes() == want, f"{ns} signers, request {j}: differs from the oracle"

    # the verify leg: the 64-signer signatures as the packed table + stream, in one arena
    keys = np.zeros(64, dtype=B.KEY_DTYPE)
    keys["off"], keys["len"], keys["scheme"], keys["fmt"] = 32 * np.arange(64), 32, B.EDDSA_ED25519_SHA512, B.KEY_RAW
    head = np.frombuffer(b"".join(pubs), dtype=np.uint8)
    tmpls = base.tmpls.copy()
    tmpls["prefix_off"] += head.size
    tmpls["suffix_off"] += head.size
    off = -(-(head.size + base.arena.size) // 16) * 16
    s12 = np.zeros(n, dtype=B.TXSIG12_DTYPE)
    s12["tx_idx"], s12["key_idx"], s12["sig_len"] = reqs[64]["tx_idx"], reqs[64]["signer"], 64
    d_varena = torch.zeros(off + 64 * n, dtype=torch.uint8, device=dev)
    d_varena[:head.size] = up(head)
    d_varena[head.size:head.size + base.arena.size] = d_arena
    d_varena[off:] = d_sigs[64]
    d_keys, d_s12 = up(keys), up(s12)
    d_vst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    eng.reserve(64, n)

    def verify():
        eng.verify_tx_signatures_packed_device(d_keys.data_ptr(), 64, d_ids.data_ptr(), a.ids, d_s12.data_ptr(), n, off,
                                               64 * n, tmpls, d_varena.data_ptr(), off + 64 * n, d_vst.data_ptr(),
                                               stream=sp)

    legs = {"sign_64": lambda: sign(64)} if a.sign_only else \
        {"sign_1": lambda: sign(1), "sign_64": lambda: sign(64), "verify": verify}
    if not a.sign_only:
        with torch.cuda.stream(stream):
            verify()
            torch.cuda.synchronize()
        assert not d_vst.cpu().numpy().any(), "a GPU signature does not verify on the GPU"
    ms = {k: [] for k in legs}
    with torch.cuda.stream(stream):
        for _ in range(a.repeats):
            for name, fn in legs.items():  # alternating: sign 1, sign 64, verify, sign 1, ...
                for _ in range(a.warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.steps):
                    fn()
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.steps)
    torch.cuda.synchronize()
    eng.close()
    out = {"lib": os.path.basename(_lib.LIB_PATH), "requests": n, "ids": a.ids, "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "template_bytes": len(pre) + 32 + len(suf), "d2h_bytes_per_signature": 64,
           "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "msigs_per_s": {}}
    for k, v in ms.items():
        r = [n / x / 1e3 for x in v]
        out["msigs_per_s"][k] = {"all": [round(x, 2) for x in r], "median": round(float(np.median(r)), 2),
                                 "min": round(min(r), 2), "max": round(max(r), 2)}
    if not a.sign_only:
        v = out["msigs_per_s"]["verify"]
        out["accept"] = bool(out["msigs_per_s"]["sign_64"]["median"] >= v["median"] - (v["max"] - v["min"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
