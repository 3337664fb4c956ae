"""Shared by the RSA-PSS signer's tests: the fixture tests/golden/rsa_sign.json (tests/golden/gen_rsa_sign.py)
and the reference, hostverify.rsa_pss_sign over Python integers."""
import json
import os

from corda_amd import hostverify
from corda_amd.engine import RsaSignerKey

HERE = os.path.dirname(os.path.abspath(__file__))
EMPTY, NOT_RUN, KEY_INVALID, UNSUPPORTED, SIGN_CHECK_FAILED = 5, 255, 3, 4, 10
SLOT = 512
PARTS = ("n", "e", "d", "p", "q", "dp", "dq", "qinv")
SIZES = ("rsa1024", "rsa1025", "rsa1032", "rsa2048e3", "rsa2048", "rsa3072", "rsa4096")  # the seven key sizes

_fx = None


def fixture():
    global _fx
    if _fx is None:
        with open(os.path.join(HERE, "golden", "rsa_sign.json")) as f:
            _fx = json.load(f)
    return _fx


def key(kid):
    """The fixture key's numbers as ints."""
    return {f: int(fixture()["keys"][kid][f], 16) for f in PARTS}


def be(v):
    return v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")


def signer_key(k):
    """A dict of ints (n, e, p, q, dp, dq, qinv) as Engine.load_rsa_signers takes it."""
    return RsaSignerKey(be(k["n"]), k["e"], be(k["p"]), be(k["q"]), be(k["dp"]), be(k["dq"]), be(k["qinv"]))


def refused():
    return [(r["id"], r["status"], {f: int(r[f], 16) for f in PARTS if f != "d"}) for r in fixture()["refused"]]


def records():
    return [dict(r, msg=bytes.fromhex(r["msg"]), salt=bytes.fromhex(r["salt"]), em=bytes.fromhex(r["em"]),
                 sig=bytes.fromhex(r["sig"])) for r in fixture()["records"]]


def sign(kid_or_key, msg, salt):
    k = key(kid_or_key) if isinstance(kid_or_key, str) else kid_or_key
    return hostverify.rsa_pss_sign(k["n"], k["d"], msg, salt)


def slot(sig):
    return bytes(sig) + bytes(SLOT - len(sig))
