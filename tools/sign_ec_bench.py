"""The ECDSA signer's rate on one MI355X against two yardsticks on code it shares but does not change (run on
the GPU box): per curve (secp256k1, secp256r1) one cg_ec_sign_tx_ids_device call per step for 2^22 requests
over the real 269-byte SignableData and 2^20 ids, 64 signers of that curve, the nonces and every other
input resident in HBM; then, in the same process,
  (a) cg_verify_tx_signatures_packed_device over the signatures that call wrote: the gate,
  (b) cg_derive_keys_device for as many requests under 64 parents of the same curve: reported, no gate
      (its k_derive_ec_mul<C> and the signer's k_ec_sign_mul<C> run the same function over the same table).

Timed with device events on the caller's stream around `--steps` calls after `--warmup` warm-up calls, the
whole sequence (sign k1, verify k1, derive k1, sign r1, verify r1, derive r1) repeated `--repeats` times,
alternating, in one process. Before timing, 256 seeded signatures per curve are compared with the Python
oracle, every status is 0, and every signature verifies on the GPU. Writes one JSON object (--out, default
profiles/sign_ec/sign_ec_bench.json) and prints it:
  msigs_per_s: per leg, every repeat's rate, their median, min and max
  accept: per curve, median sign rate >= median verify rate - (max - min of the verify repeats)
The kernel shares come from a kernel trace of this tool run with --trace-legs --repeats 1 (the sign and
derive legs alone), in a run of its own; its kernel statistics are kept beside the JSON."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CURVES = {"k1": 2, "r1": 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1 << 22)
    ap.add_argument("--ids", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--trace-legs", action="store_true", help="the sign and derive legs alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign_ec", "sign_ec_bench.json"))
    a = ap.parse_args()

    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()  # torch's HIP runtime opens the device before the library's (tests/conftest.py)
    from corda_amd import _lib, signable
    from corda_amd import batch as B
    from corda_amd.engine import Engine
    from oracle import ecdsa_bc as bc

    n = a.requests
    rng = np.random.default_rng(a.seed)
    ids = rng.integers(0, 256, (a.ids, 32), dtype=np.uint8)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    d_ids = up(ids)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    eng = Engine(0)
    legs, checks = {}, {}
    keep = []  # device buffers stay alive

    for name, scheme in CURVES.items():
        order = bc.CURVES[scheme].n
        pre, suf = signable.template(1, scheme)
        sb = B.SignRequestBuilder()
        sb.template(pre, suf)
        base = sb.build()
        ds = [int.from_bytes(hashlib.sha256(b"sign_ec_bench %d %d" % (scheme, k)).digest(), "big") % (order - 1) + 1
              for k in range(64)]
        signers = [(scheme, d.to_bytes(32, "big")) for d in ds]
        reqs = np.zeros(n, dtype=B.SIGN_REQ_DTYPE)
        reqs["tx_idx"], reqs["signer"] = rng.integers(0, a.ids, n), rng.integers(0, 64, n)
        nonces = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        nonces[:, 0] &= 0x7F  # k < 2^255 < n on both curves: no refused candidate in a timed call
        nonces[:, 31] |= 1    # never zero
        d_reqs, d_arena, d_non = up(reqs), up(base.arena), up(nonces)
        d_sigs = torch.zeros(72 * n, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        keep += [d_reqs, d_arena, d_non, d_sigs, d_len, d_st]

        def sign(signers=signers, base=base, d_reqs=d_reqs, d_arena=d_arena, d_non=d_non, d_sigs=d_sigs, d_len=d_len,
                 d_st=d_st):
            eng.sign_ec_tx_ids_device(d_ids.data_ptr(), a.ids, d_reqs.data_ptr(), n, base.tmpls, d_arena.data_ptr(),
                                      base.arena.size, d_non.data_ptr(), d_sigs.data_ptr(), d_len.data_ptr(),
                                      d_st.data_ptr(), stream=sp)

        # correctness first: every status 0, a seeded sample against the oracle
        pubs, lst = eng.load_ec_signers(signers)
        assert not lst.any()
        with torch.cuda.stream(stream):
            sign()
            torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any(), f"{name}: a request was not signed"
        sigs = d_sigs.cpu().numpy().reshape(-1, 72)
        lens = d_len.cpu().numpy()
        for j in np.random.default_rng(a.seed + scheme).choice(n, 256, replace=False):
            q = reqs[j]
            msg = pre + ids[int(q["tx_idx"])].tobytes() + suf
            want = bc.der_encode_sig(*bc.sign(scheme, ds[int(q["signer"])], msg, int.from_bytes(nonces[j].tobytes(), "big")))
            assert sigs[j, :lens[j]].tobytes() == want and not sigs[j, lens[j]:].any(), f"{name}, request {j}: differs from the oracle"
        checks[name] = {"signed": int(n), "oracle_sample": 256, "der_len_min": int(lens.min()), "der_len_max": int(lens.max())}

        # (a) the verify leg: these signatures as the packed table + stream, in one arena
        keys = np.zeros(64, dtype=B.KEY_DTYPE)
        keys["off"], keys["len"], keys["scheme"], keys["fmt"] = 64 * np.arange(64), 64, scheme, B.KEY_RAW
        head = np.frombuffer(b"".join(pubs), dtype=np.uint8)
        tmpls = base.tmpls.copy()
        tmpls["prefix_off"] += head.size
        tmpls["suffix_off"] += head.size
        off = -(-(head.size + base.arena.size) // 16) * 16
        rl = (lens.astype(np.int64) + 3) & ~3
        sig_stream = sigs[np.arange(72)[None, :] < rl[:, None]]  # row-major: signature i at the 4-aligned end of i - 1
        assert sig_stream.size == int(rl.sum())
        s12 = np.zeros(n, dtype=B.TXSIG12_DTYPE)
        s12["tx_idx"], s12["key_idx"], s12["sig_len"] = reqs["tx_idx"], reqs["signer"], lens
        varena = np.zeros(off + sig_stream.size, dtype=np.uint8)
        varena[:head.size] = head
        varena[head.size:head.size + base.arena.size] = base.arena
        varena[off:] = sig_stream
        d_varena, d_keys, d_s12 = up(varena), up(keys), up(s12)
        d_vst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        keep += [d_varena, d_keys, d_s12, d_vst]
        eng.reserve(64, n)

        def verify(tmpls=tmpls, off=off, nbytes=sig_stream.size, d_varena=d_varena, d_keys=d_keys, d_s12=d_s12, d_vst=d_vst):
            eng.verify_tx_signatures_packed_device(d_keys.data_ptr(), 64, d_ids.data_ptr(), a.ids, d_s12.data_ptr(), n, off,
                                                   nbytes, tmpls, d_varena.data_ptr(), off + nbytes, d_vst.data_ptr(),
                                                   stream=sp)

        if not a.trace_legs:
            with torch.cuda.stream(stream):
                verify()
                torch.cuda.synchronize()
            assert not d_vst.cpu().numpy().any(), f"{name}: a GPU signature does not verify on the GPU"
            checks[name]["verified_on_gpu"] = int(n)

        # (b) the derive leg: n requests (32-byte seeds) under 64 parents of this curve
        db = B.DeriveRequestBuilder()
        for d in ds:
            db.parent(scheme, d.to_bytes(32, "big"))
        db.add_request(0, bytes(32))
        one = db.build()
        seeds_at = -(-one.arena.size // 4) * 4
        darena = np.zeros(seeds_at + 32 * n, dtype=np.uint8)
        darena[:one.arena.size] = one.arena
        darena[seeds_at:] = rng.integers(0, 256, 32 * n, dtype=np.uint8)
        dreqs = np.zeros(n, dtype=B.DERIVE_REQ_DTYPE)
        dreqs["seed_off"], dreqs["seed_len"], dreqs["parent"] = seeds_at + 32 * np.arange(n, dtype=np.uint64), 32, reqs["signer"]
        d_par, d_dreq, d_darena = up(one.parents), up(dreqs), up(darena)
        d_sec = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        d_pub = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
        d_dst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        keep += [d_par, d_dreq, d_darena, d_sec, d_pub, d_dst]

        def derive(n_par=len(one.parents), alen=darena.size, d_par=d_par, d_dreq=d_dreq, d_darena=d_darena, d_sec=d_sec,
                   d_pub=d_pub, d_dst=d_dst):
            eng.derive_keys_device(d_par.data_ptr(), n_par, d_dreq.data_ptr(), n, d_darena.data_ptr(), alen,
                                   d_sec.data_ptr(), d_pub.data_ptr(), d_dst.data_ptr(), stream=sp)

        legs[name] = {"signers": signers, "sign": sign, "verify": verify, "derive": derive}

    order = [(c, k) for c in CURVES for k in (("sign", "derive") if a.trace_legs else ("sign", "verify", "derive"))]
    ms = {f"{k}_{c}": [] for c, k in order}
    with torch.cuda.stream(stream):
        for _ in range(a.repeats):
            for c, k in order:
                if k == "sign":  # one signer set per context: this curve's
                    torch.cuda.synchronize()
                    eng.load_ec_signers(legs[c]["signers"])
                fn = legs[c][k]
                for _ in range(a.warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.steps):
                    fn()
                e1.record(stream)
                e1.synchronize()
                ms[f"{k}_{c}"].append(e0.elapsed_time(e1) / a.steps)
    torch.cuda.synchronize()
    info = eng.info()
    eng.close()
    out = {"lib": os.path.basename(_lib.LIB_PATH), "fixed_base_bits": info.get("fixed_base_bits"), "requests": n, "ids": a.ids,
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "signers_per_leg": 64, "checks": checks,
           "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "msigs_per_s": {}}
    for k, v in ms.items():
        r = [n / x / 1e3 for x in v]
        out["msigs_per_s"][k] = {"all": [round(x, 2) for x in r], "median": round(float(np.median(r)), 2),
                                 "min": round(min(r), 2), "max": round(max(r), 2)}
    if not a.trace_legs:
        out["accept"] = {}
        for c in CURVES:
            v, s = out["msigs_per_s"][f"verify_{c}"], out["msigs_per_s"][f"sign_{c}"]
            out["accept"][c] = bool(s["median"] >= v["median"] - (v["max"] - v["min"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
