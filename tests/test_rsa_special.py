"""CPU tests of tests/golden/rsa_special.json (tests/golden/gen_rsa_special.py): special-form prime
moduli whose key preparation reaches the carry ripple of rsa_resolve, and keys for every branch of
the exponent ladder. The restatement (corda_amd/hostverify.py) and the host build of rsa.h agree with
every `expect`; the lane model (tests/rsa_wave_model.py) proves that the key preparation of each
special-form key reaches the ripple below L and that a random key of the same size does not."""
import ctypes
import json
import math
import os
import random

import pytest

import rsa_wave_model as M
from corda_amd import hostverify
from test_rsa_host import Rec, lib  # noqa: F401  (the host build of rsa.h, tests/native/host_rsa.cpp)

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "rsa_special.json")))
KEYS, ITEMS = G["keys"], G["items"]
SPECIAL = [f"{t}{b}" for b in (1024, 1025, 2048, 2049, 4096) for t in ("m", "p")]
SHAPES = {"e1": 1, "e2": 2, "e4": 4, "e6": 6, "e80000001": 0x80000001, "effffffff": 0xFFFFFFFF, "e10001": 0x10001}


def test_fixture_holds_the_keys_and_items_it_should():
    assert list(KEYS) == SPECIAL + list(SHAPES)
    for kid, k in KEYS.items():
        n, bits = int(k["n"], 16), k["bits"]
        assert hostverify.rsa_decode_key(bytes.fromhex(k["spki"])) == (n, k["e"]) and n.bit_length() == bits and n % 2
        notes = [i["note"] for i in ITEMS if i["key"] == kid]
        assert notes[:4] == ["valid", "flip signature bit", "flip message bit", "s = n - 1"], kid
        valid = sum(1 for i in ITEMS if i["key"] == kid and i["expect"] == "VALID")
        if kid in SHAPES:
            assert k["e"] == SHAPES[kid] and bits == 2048 and len(notes) == 4 and valid >= 1
        else:
            c = k["c"]
            assert k["e"] == 65537 and math.gcd(65537, n - 1) == 1 and 0 < c < 1 << 20
            assert n == ((1 << bits) - c if kid[0] == "m" else (1 << (bits - 1)) + c)
            assert len(notes) == 12 and valid >= 9
            lens = {len(i["msg"]) // 2 for i in ITEMS if i["key"] == kid and i["expect"] == "VALID"}
            assert len(lens) >= 8
        if "d" in k:  # the modulus is prime: d inverts e modulo n - 1
            assert k["e"] * int(k["d"], 16) % (n - 1) == 1 and pow(3, n - 1, n) == 1
    assert os.path.getsize(os.path.join(HERE, "golden", "rsa_special.json")) < 1 << 20


def test_expect_is_the_restatement(lib):  # noqa: F811
    """hostverify.rsa_verify and the host build of rsa.h (hr_verify: also e = 1 and even e) give `expect`;
    hr_key_bits accepts every key; the scalar key preparation gives R^2 mod n."""
    for kid, k in KEYS.items():
        spki = bytes.fromhex(k["spki"])
        assert lib.hr_key_bits(spki, len(spki)) == k["bits"], kid
        rec = Rec()
        assert lib.hr_key_prepare(spki, len(spki), ctypes.byref(rec)) == 1, kid
        n = int(k["n"], 16)
        assert rec.e == k["e"] and rec.L == (k["bits"] + 31) // 32
        assert sum(int(rec.rr[i]) << (32 * i) for i in range(128)) == pow(2, 64 * rec.L, n), kid
    for i in ITEMS:
        k = KEYS[i["key"]]
        spki, sig, msg = bytes.fromhex(k["spki"]), bytes.fromhex(i["sig"]), bytes.fromhex(i["msg"])
        want = i["expect"] == "VALID"
        assert hostverify.rsa_verify((int(k["n"], 16), k["e"]), sig, msg) == want, (i["key"], i["note"])
        assert lib.hr_verify(spki, len(spki), sig, len(sig), msg, len(msg)) == (1 if want else 0), (i["key"], i["note"])


def test_special_keys_reach_the_ripple_in_the_key_preparation():
    """The model's wave-form key preparation ends at R^2 mod n and, for every special-form key, reaches
    generating lanes, propagating lanes that receive a carry and a chain of at least 8 of those, all
    below L; a random key of the same size reaches none. meta.keyprep records the measured counts."""
    rng = random.Random(0xC0DA)
    for kid in SPECIAL:
        n, bits = int(KEYS[kid]["n"], 16), KEYS[kid]["bits"]
        rr, ev = M.keyprep(n)
        assert rr == pow(2, 64 * ((bits + 31) // 32), n), kid
        row = ev.row(0)
        assert row["gen"] >= 1 and row["cprop"] >= 1 and row["chain"] >= 8, (kid, row)
        assert G["meta"]["keyprep"][kid] == {"gen": row["gen"], "cprop": row["cprop"], "chain": row["chain"]}, kid
        if kid[0] == "m":  # once per size
            r = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
            rr, ev = M.keyprep(r)
            row = ev.row(0)
            assert rr == pow(2, 64 * ((bits + 31) // 32), r)
            assert row["gen"] == 0 and row["cprop"] == 0 and row["chain"] == 0, (bits, row)
