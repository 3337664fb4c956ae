"""The RSA-PSS signer's rate on one MI355X against the host's: per modulus size (2048,
3072, 4096 bits) one cg_rsa_sign_tx_ids_device call per step over the real 269-byte SignableData, 64 signers
of that size, the salts and every other input resident in HBM. Timed with device events on the caller's
stream around `--steps` calls after `--warmup` warm-up calls, the three legs repeated `--repeats` times,
alternating, in one process. Before timing, per size: every status is 0, a seeded sample of signatures equals
hostverify.rsa_pss_sign (Python integers), and every signature is VALID on the same context's RSA verifier.

The yardstick is `openssl speed -multi 16 rsa2048 rsa3072 rsa4096` (sign/s), taken by this tool in the same
session with --openssl (16 processes, as DESIGN.md's RSA verify table). Writes one JSON object (--out,
default profiles/sign_rsa/rsa_sign_bench.json) and prints it:
  sigs_per_s: per size, every repeat's rate, their median, min and max
  openssl_sign_per_s, ratio, accept: per size, median sign rate >= OpenSSL's 16-process sign rate

The 64 keys per size come from the OpenSSL CLI, which takes minutes at 4096 bits and needs no GPU:
`--prepare-only --cache FILE` makes them once, a later run with the same `--cache` loads them.

  python tools/rsa_sign_bench.py --cache /tmp/rsa_sign_bench.json --prepare-only
  python tools/rsa_sign_bench.py --cache /tmp/rsa_sign_bench.json --openssl
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from corda_amd import hostverify  # noqa: E402

REQUESTS = {2048: 24576, 3072: 12288, 4096: 12288}  # whole rounds of the resident waves; tens of ms per call
PARTS = ("n", "e", "d", "p", "q", "dp", "dq", "qinv")


def gen_key(bits, d):
    key = os.path.join(d, "k.pem")
    subprocess.run(["openssl", "genpkey", "-algorithm", "RSA", "-pkeyopt", f"rsa_keygen_bits:{bits}", "-out", key],
                   check=True, capture_output=True)
    pkcs8 = subprocess.run(["openssl", "pkcs8", "-topk8", "-nocrypt", "-in", key, "-outform", "DER"], check=True,
                           capture_output=True).stdout
    spki = subprocess.run(["openssl", "pkey", "-in", key, "-pubout", "-outform", "DER"], check=True,
                          capture_output=True).stdout
    k = hostverify.rsa_decode_private_key(pkcs8)
    return dict({f: hex(k[f]) for f in PARTS}, spki=spki.hex())


def openssl_speed(seconds):
    """{bits: sign/s} of `openssl speed -multi 16`."""
    r = subprocess.run(["openssl", "speed", "-multi", "16", "-seconds", str(seconds), "rsa2048", "rsa3072", "rsa4096"],
                       check=True, capture_output=True, text=True)
    out = {}
    for m in re.finditer(r"^rsa\s+(\d+) bits\s+\S+\s+\S+\s+([\d.]+)\s+([\d.]+)", r.stdout, re.M):
        out[int(m.group(1))] = float(m.group(2))
    assert set(out) >= {2048, 3072, 4096}, r.stdout[-2000:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[2048, 3072, 4096])
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--requests", type=int, default=0, help="per call (default: per size, REQUESTS)")
    ap.add_argument("--ids", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cache", default="")
    ap.add_argument("--prepare-only", action="store_true")
    ap.add_argument("--openssl", action="store_true", help="take `openssl speed -multi 16` in this session: the gate")
    ap.add_argument("--openssl-seconds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign_rsa", "rsa_sign_bench.json"))
    a = ap.parse_args()

    cache = {}
    if a.cache and os.path.exists(a.cache):
        cache = json.load(open(a.cache))
    for bits in a.bits:
        tag = f"{bits}/{a.keys}"
        if tag not in cache:
            t0 = time.time()
            with tempfile.TemporaryDirectory() as d:
                cache[tag] = [gen_key(bits, d) for _ in range(a.keys)]
            print(f"# prepared {tag} in {time.time() - t0:.1f} s", file=sys.stderr)
            if a.cache:
                json.dump(cache, open(a.cache, "w"))
    if a.prepare_only:
        return 0

    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()  # torch's HIP runtime opens the device before the library's (tests/conftest.py)
    from corda_amd import _lib, signable
    from corda_amd import batch as B
    from corda_amd.engine import Engine, RsaSignerKey

    ossl = openssl_speed(a.openssl_seconds) if a.openssl else None
    rng = np.random.default_rng(a.seed)
    ids = rng.integers(0, 256, (a.ids, 32), dtype=np.uint8)
    up = lambda x: torch.from_numpy(np.array(x, copy=True).view(np.uint8)).to(dev)  # noqa: E731
    d_ids = up(ids)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    eng = Engine(0, rsa=True)
    pre, suf = signable.template(1, 1)
    sb = B.SignRequestBuilder()
    sb.template(pre, suf)
    base = sb.build()
    d_arena = up(np.concatenate([base.arena, np.zeros(-base.arena.size % 4, np.uint8)]))
    be = lambda v: v.to_bytes((v.bit_length() + 7) // 8, "big")  # noqa: E731
    legs, checks, keep = {}, {}, []

    for bits in a.bits:
        n = a.requests or REQUESTS.get(bits, 12288)
        keys = [{f: int(k[f], 16) for f in PARTS} for k in cache[f"{bits}/{a.keys}"]]
        spkis = [bytes.fromhex(k["spki"]) for k in cache[f"{bits}/{a.keys}"]]
        signers = [RsaSignerKey(be(k["n"]), k["e"], be(k["p"]), be(k["q"]), be(k["dp"]), be(k["dq"]), be(k["qinv"]))
                   for k in keys]
        reqs = np.zeros(n, dtype=B.SIGN_REQ_DTYPE)
        reqs["tx_idx"], reqs["signer"] = rng.integers(0, a.ids, n), rng.integers(0, len(keys), n)
        salts = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d_reqs, d_salts = up(reqs), up(salts)
        d_sigs = torch.zeros(512 * n, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(2 * n, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        keep += [d_reqs, d_salts, d_sigs, d_len, d_st]

        def sign(n=n, d_reqs=d_reqs, d_salts=d_salts, d_sigs=d_sigs, d_len=d_len, d_st=d_st):
            eng.sign_rsa_tx_ids_device(d_ids.data_ptr(), a.ids, d_reqs.data_ptr(), n, base.tmpls, d_arena.data_ptr(),
                                       base.arena.size, d_salts.data_ptr(), d_sigs.data_ptr(), d_len.data_ptr(),
                                       d_st.data_ptr(), stream=sp)

        # correctness first: every status 0, a seeded sample against the reference, every signature VALID
        assert not eng.load_rsa_signers(signers).any()
        with torch.cuda.stream(stream):
            sign()
            torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any(), f"{bits}: a request was not signed"
        k_bytes = (bits + 7) // 8
        sigs = d_sigs.cpu().numpy().reshape(-1, 512)
        assert (d_len.cpu().numpy().view(np.uint16) == k_bytes).all() and not sigs[:, k_bytes:].any()
        for j in np.random.default_rng(a.seed + bits).choice(n, a.sample, replace=False):
            q = reqs[j]
            k = keys[int(q["signer"])]
            want = hostverify.rsa_pss_sign(k["n"], k["d"], pre + ids[int(q["tx_idx"])].tobytes() + suf, salts[j].tobytes())
            assert sigs[j, :k_bytes].tobytes() == want, f"{bits} bits, request {j}: differs from the reference"
        # the verify batch: items over one arena [keys][signatures][messages]
        vkeys = np.zeros(len(keys), dtype=B.KEY_DTYPE)
        head = b"".join(spkis)
        vkeys["off"] = np.cumsum([0] + [len(s) for s in spkis[:-1]])
        vkeys["len"], vkeys["scheme"], vkeys["fmt"] = [len(s) for s in spkis], 1, B.KEY_SPKI
        msgs = np.empty((n, 269), dtype=np.uint8)
        assert len(pre) + 32 + len(suf) == 269
        msgs[:, :len(pre)] = np.frombuffer(pre, dtype=np.uint8)
        msgs[:, len(pre):len(pre) + 32] = ids[reqs["tx_idx"]]
        msgs[:, len(pre) + 32:] = np.frombuffer(suf, dtype=np.uint8)
        sig_at = -(-len(head) // 4) * 4
        msg_at = sig_at + k_bytes * n
        varena = np.zeros(msg_at + 269 * n + 8, dtype=np.uint8)
        varena[:len(head)] = np.frombuffer(head, dtype=np.uint8)
        varena[sig_at:msg_at] = sigs[:, :k_bytes].reshape(-1)
        varena[msg_at:msg_at + 269 * n] = msgs.reshape(-1)
        items = np.zeros(n, dtype=B.ITEM_DTYPE)
        items["sig_off"], items["sig_len"] = sig_at + k_bytes * np.arange(n, dtype=np.uint64), k_bytes
        items["msg_off"], items["msg_len"] = msg_at + 269 * np.arange(n, dtype=np.uint64), 269
        items["key_idx"] = reqs["signer"]
        v = eng.verify(B.Batch(vkeys, items, varena), B.MODE_DOVERIFY)
        assert (v == B.VALID).all(), f"{bits}: a GPU signature does not verify on the GPU"
        checks[bits] = {"signed": int(n), "reference_sample": int(a.sample), "verified_on_gpu": int(n)}
        legs[bits] = {"signers": signers, "sign": sign, "n": n}

    ms = {bits: [] for bits in a.bits}
    with torch.cuda.stream(stream):
        for _ in range(a.repeats):
            for bits in a.bits:
                torch.cuda.synchronize()
                eng.load_rsa_signers(legs[bits]["signers"])  # one signer set per context: this size's
                fn = legs[bits]["sign"]
                for _ in range(a.warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.steps):
                    fn()
                e1.record(stream)
                e1.synchronize()
                ms[bits].append(e0.elapsed_time(e1) / a.steps)
    torch.cuda.synchronize()
    eng.clear_rsa_signers()
    eng.close()
    out = {"lib": os.path.basename(_lib.LIB_PATH), "ids": a.ids, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "signers_per_leg": a.keys, "requests": {str(b): legs[b]["n"] for b in a.bits},
           "checks": {str(b): c for b, c in checks.items()},
           "ms_per_call": {str(b): [round(x, 3) for x in v] for b, v in ms.items()}, "sigs_per_s": {}}
    for bits, v in ms.items():
        r = [legs[bits]["n"] / x * 1e3 for x in v]
        out["sigs_per_s"][str(bits)] = {"all": [round(x) for x in r], "median": round(float(np.median(r))),
                                        "min": round(min(r)), "max": round(max(r))}
    if ossl:
        out["openssl_sign_per_s"] = {str(b): ossl[b] for b in a.bits if b in ossl}
        out["ratio"] = {str(b): round(out["sigs_per_s"][str(b)]["median"] / ossl[b], 2) for b in a.bits if b in ossl}
        out["accept"] = {str(b): bool(out["sigs_per_s"][str(b)]["median"] >= ossl[b]) for b in a.bits if b in ossl}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
