"""Child process of tests/test_gpu_derive.py (run with CG_TEST_DERIVE_FORCE_RETRIES=k set, which the
library reads at cg_open): one parent of each scheme, seeds of 0, 6 and 129 bytes, through
cg_derive_keys, and one ECDSA key pair through the Python mirror. Prints one JSON line: per request
(scheme, seed length, status, secret, pub, retries), and the mirror's key pair."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from corda_amd import batch as B  # noqa: E402
from corda_amd.crypto import Crypto, PrivateKey  # noqa: E402
from corda_amd.engine import Engine  # noqa: E402

PRIVATE = {2: bytes(range(1, 33)), 3: bytes(range(2, 34)), 4: bytes(range(3, 35))}
SEEDS = [b"", b"seed-1", bytes((5 * i + 1) & 255 for i in range(129))]


def main():
    b = B.DeriveRequestBuilder()
    rows = []
    for scheme in (2, 3, 4):
        p = b.parent(scheme, PRIVATE[scheme])
        for s in SEEDS:
            b.add_request(p, s)
            rows.append((scheme, len(s)))
    with Engine(0) as eng:
        secrets, pubs, st, tries = eng.derive_keys(b.build())
        Crypto.use_engine(eng)
        kp = Crypto.derive_key_pair(PrivateKey(3, PRIVATE[3]), b"seed-1")
    out = {"items": [{"scheme": sc, "seed_len": ln, "status": int(st[j]), "secret": secrets[j].tobytes().hex(),
                      "pub": pubs[j].tobytes().hex(), "retries": int(tries[j])} for j, (sc, ln) in enumerate(rows)],
           "mirror": {"secret": kp.private.encoded.hex(), "pub": kp.public.encoded.hex()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
