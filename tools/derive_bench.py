"""The key-derivation rate on one MI355X (run on the GPU box): cg_derive_keys_device for 2^22 requests with
32-byte seeds over 64 parents of one scheme, inputs resident in HBM, one leg per scheme (Ed25519,
secp256r1, secp256k1); and cg_sign_tx_ids_device (1 signer, the shape tools/sign_bench.py uses) on the
same warm context as the yardstick: a derivation runs the signer's fixed-base gather and batched encode,
fewer SHA-512 compressions and no scalar multiply-add.

Timed with device events on the caller's stream around `--steps` calls after `--warmup` warm-up calls,
the legs alternating, the sequence repeated `--repeats` times in one process. Before timing, 256 seeded
results of each derive leg are compared with tests/derive_ref.py. Writes one JSON object (--out, default
profiles/derive/derive_bench.json) and prints it:
  mkeys_per_s: per leg, every repeat's rate, their median, min and max
  accept: median Ed25519 derive rate >= median sign rate - (max - min of the sign repeats)
The two ECDSA legs have no comparable call: their rates are reported, no threshold. The share of a call
in each kernel comes from a kernel trace of this tool run with --leg NAME --repeats 1 in a run of its own."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = {"derive_ed25519": 4, "derive_secp256r1": 3, "derive_secp256k1": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1 << 22)
    ap.add_argument("--parents", type=int, default=64)
    ap.add_argument("--ids", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--leg", default=None, help="one leg alone (for a kernel trace): " + ", ".join(list(LEGS) + ["sign_1"]))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derive", "derive_bench.json"))
    a = ap.parse_args()

    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()  # torch's HIP runtime opens the device before the library's (tests/conftest.py)
    import derive_ref as R
    from corda_amd import _lib, signable
    from corda_amd import batch as B
    from corda_amd import derive as D
    from corda_amd.engine import Engine

    n = a.requests
    rng = np.random.default_rng(a.seed)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    eng = Engine(0)

    # per scheme: 64 parents' keyData, then n 32-byte seeds, in one arena
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sets = {}
    for name, scheme in LEGS.items():
        keys = [D.key_data(scheme, hashlib.sha256(b"derive_bench %d/%d" % (scheme, k)).digest()) for k in range(a.parents)]
        parents = np.zeros(a.parents, dtype=B.DERIVE_PARENT_DTYPE)
        off = 0
        for k, kd in enumerate(keys):
            parents[k]["key_off"], parents[k]["key_len"], parents[k]["scheme"] = off, len(kd), scheme
            off += len(kd)
        base = -(-off // 16) * 16
        arena = np.zeros(base + 32 * n, dtype=np.uint8)
        arena[:off] = np.frombuffer(b"".join(keys), dtype=np.uint8)
        arena[base:] = seeds.reshape(-1)
        reqs = np.zeros(n, dtype=B.DERIVE_REQ_DTYPE)
        reqs["seed_off"], reqs["seed_len"] = base + 32 * np.arange(n, dtype=np.uint64), 32
        reqs["parent"] = rng.integers(0, a.parents, n)
        sets[name] = dict(scheme=scheme, keys=keys, reqs=reqs, arena_len=arena.size, d_parents=up(parents),
                          d_reqs=up(reqs), d_arena=up(arena))
    d_secrets = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_pubs = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)

    def derive(name):
        s = sets[name]
        eng.derive_keys_device(s["d_parents"].data_ptr(), a.parents, s["d_reqs"].data_ptr(), n, s["d_arena"].data_ptr(),
                               s["arena_len"], d_secrets.data_ptr(), d_pubs.data_ptr(), d_st.data_ptr(), None, stream=sp)

    # the yardstick: the signer, 1 signer over the real SignableData template
    pre, suf = signable.template(1, 4)
    ids = rng.integers(0, 256, (a.ids, 32), dtype=np.uint8)
    sb = B.SignRequestBuilder()
    sb.template(pre, suf)
    sbase = sb.build()
    sreqs = np.zeros(n, dtype=B.SIGN_REQ_DTYPE)
    sreqs["tx_idx"] = rng.integers(0, a.ids, n)
    d_ids, d_sarena, d_sreqs = up(ids), up(sbase.arena), up(sreqs)
    d_sigs = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    d_sst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    eng.load_signers([hashlib.sha256(b"derive_bench signer").digest()])

    def sign():
        eng.sign_tx_ids_device(d_ids.data_ptr(), a.ids, d_sreqs.data_ptr(), n, sbase.tmpls, d_sarena.data_ptr(),
                               sbase.arena.size, d_sigs.data_ptr(), d_sst.data_ptr(), stream=sp)

    # correctness first: a seeded sample of each derive leg against derive_ref
    with torch.cuda.stream(stream):
        for name, s in sets.items():
            if a.leg and a.leg != name:  # a traced run holds the kernels of its leg alone
                continue
            derive(name)
            torch.cuda.synchronize()
            assert not d_st.cpu().numpy().any(), f"{name}: a request was not derived"
            secrets, pubs = d_secrets.cpu().numpy().reshape(-1, 32), d_pubs.cpu().numpy().reshape(-1, 64)
            for j in np.random.default_rng(a.seed + s["scheme"]).choice(n, 256, replace=False):
                want = R.derive(s["scheme"], s["keys"][int(s["reqs"]["parent"][j])], seeds[j].tobytes())
                assert (secrets[j].tobytes(), pubs[j].tobytes()) == want[:2], f"{name}, request {j}: differs from derive_ref"
        if not a.leg or a.leg == "sign_1":
            sign()
            torch.cuda.synchronize()
            assert not d_sst.cpu().numpy().any()

    legs = {name: (lambda name=name: derive(name)) for name in LEGS}
    legs["sign_1"] = sign
    if a.leg:
        legs = {a.leg: legs[a.leg]}
    ms = {k: [] for k in legs}
    with torch.cuda.stream(stream):
        for _ in range(a.repeats):
            for name, fn in legs.items():  # alternating
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
    out = {"lib": os.path.basename(_lib.LIB_PATH), "requests": n, "parents": a.parents, "seed_bytes": 32, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "mkeys_per_s": {}}
    for k, v in ms.items():
        r = [n / x / 1e3 for x in v]
        out["mkeys_per_s"][k] = {"all": [round(x, 2) for x in r], "median": round(float(np.median(r)), 2),
                                 "min": round(min(r), 2), "max": round(max(r), 2)}
    if not a.leg:
        s = out["mkeys_per_s"]["sign_1"]
        out["accept"] = bool(out["mkeys_per_s"]["derive_ed25519"]["median"] >= s["median"] - (s["max"] - s["min"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
