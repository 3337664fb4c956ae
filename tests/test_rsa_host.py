"""CPU tests of corda_amd/csrc/rsa.h (the code the RSA kernels run for the key decode, the Montgomery
constants and the EMSA-PSS check) through tests/native/host_rsa.cpp, against Python integers and the
BC 1.57 restatement (corda_amd/hostverify.py), over every key and item of tests/golden/rsa.json and
tests/golden/rsa_gpu.json."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess

import pytest

from corda_amd import hostverify

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "host_rsa.cpp")
HDRS = [os.path.join(HERE, "..", "corda_amd", "csrc", h) for h in ("rsa.h", "sha2.h", "fe25519.h")]
SO = os.path.join(HERE, "native", "libhostrsatest.so")
MAX_LIMBS = 128


class Rec(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("ok", "bits", "L", "k", "em_bits", "block_len", "e", "n0inv")] + \
               [("n", ctypes.c_uint32 * MAX_LIMBS), ("rr", ctypes.c_uint32 * MAX_LIMBS)]


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HDRS)


@pytest.fixture(scope="module")
def lib():
    if _stale(SO):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.hr_rec_bytes.restype = ctypes.c_uint32
    L.hr_key_prepare.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(Rec)]
    L.hr_key_bits.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    L.hr_key_bits.restype = ctypes.c_uint32
    L.hr_modexp.argtypes = [ctypes.POINTER(Rec), ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    L.hr_pss_check.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    L.hr_verify.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p,
                            ctypes.c_uint32]
    assert L.hr_rec_bytes() == ctypes.sizeof(Rec) == 32 + 8 * MAX_LIMBS
    return L


def _load():
    """(keys {id: dict}, items [(key id, key_fmt, spki, sig, msg, expect, note)]) of both fixtures."""
    g = json.load(open(os.path.join(HERE, "golden", "rsa_gpu.json")))
    keys = dict(g["keys"])
    items = [(i["key"], i["key_fmt"], bytes.fromhex(keys[i["key"]]["spki"]), bytes.fromhex(i["sig"]),
              bytes.fromhex(i["msg"]), i["expect"], i["note"]) for i in g["items"]]
    old = json.load(open(os.path.join(HERE, "golden", "rsa.json")))
    for i in old["items"]:
        kid = "rsa.json/%d" % i["bits"]
        keys.setdefault(kid, {"spki": i["key"], "bits": i["bits"], "accepted": True})
        items.append((kid, i["key_fmt"], bytes.fromhex(i["key"]), bytes.fromhex(i["sig"]), bytes.fromhex(i["msg"]),
                      i["expect"], i["note"]))
    return keys, items


KEYS, ITEMS = _load()


def _limbs(arr, count):
    return sum(int(arr[i]) << (32 * i) for i in range(count))


def test_fixture_covers_the_sizes_and_cases():
    bits = {k["bits"] for k in KEYS.values() if k["accepted"]}
    assert {1024, 1025, 1032, 2048, 3072, 4096} <= bits
    assert any(k.get("e") == 3 for k in KEYS.values())
    declined = {kid for kid, k in KEYS.items() if not k["accepted"]}
    assert {"rsa1016", "rsa4104", "even_n", "big_e", "nonminimal_len", "trailing", "negative_n", "p256_oid",
            "fmt_raw", "garbage"} <= declined
    notes = {n for *_, n in ITEMS}
    for want in ("valid", "flip message bit", "flip signature bit", "sig_len = k + 1 with a leading 0x00",
                 "valid signature with its leading 0x00 stripped", "s = 0", "s = 1", "s = n - 1", "s = n",
                 "s = 2^(8k) - 1", "wrong trailer", "nonzero padding byte", "missing 0x01", "20-byte salt",
                 "message of 1 bytes", "message of 55 bytes", "message of 56 bytes", "message of 64 bytes",
                 "message of 700 bytes", "empty signature", "a signature made by another key"):
        assert want in notes, want
    # the masked top bit: the restatement accepts what OpenSSL rejects, both recorded
    g = json.load(open(os.path.join(HERE, "golden", "rsa_gpu.json")))
    top = [i for i in g["items"] if i["note"].startswith("top masked bit")]
    assert len(top) >= 4 and all(i["expect"] == "VALID" and i["openssl"] == "reject" for i in top)
    # `expect` is the restatement's verdict on the stored bytes
    for kid, fmt, spki, sig, msg, expect, note in ITEMS:
        try:
            got = "VALID" if hostverify.rsa_verify(hostverify.rsa_decode_key(spki), sig, msg) else "INVALID"
        except hostverify.InvalidKeySpecException:
            got = "HOST_EXCEPTION"
        assert got == expect, (kid, note)


def test_key_decode_and_montgomery_constants(lib):
    """Every fixture key: accepted exactly when the fixture says so; n, L, k, emBits, block_len, e,
    -n^-1 mod 2^32 and R^2 mod n equal Python's."""
    for kid, k in KEYS.items():
        spki = bytes.fromhex(k["spki"])
        rec = Rec()
        ok = lib.hr_key_prepare(spki, len(spki), ctypes.byref(rec))
        # (fmt_raw is a good encoding: the fmt is the kernel's check, not the decode's)
        want_ok = k["accepted"] or kid == "fmt_raw"
        assert bool(ok) == want_ok, kid
        assert lib.hr_key_bits(spki, len(spki)) == (rec.bits if ok else 0), kid
        if not ok:
            continue
        n, e = hostverify.rsa_decode_key(spki)
        bits = n.bit_length()
        assert rec.bits == bits == k["bits"] or kid == "fmt_raw"
        L = (bits + 31) // 32
        assert (rec.L, rec.k, rec.em_bits, rec.block_len, rec.e) == (L, (bits + 7) // 8, bits - 1, (bits + 6) // 8, e)
        assert _limbs(rec.n, MAX_LIMBS) == n, kid
        assert (n * ((1 << 32) - rec.n0inv)) % (1 << 32) == 1, kid  # n0inv = -n^-1 mod 2^32
        assert _limbs(rec.rr, MAX_LIMBS) == pow(2, 64 * L, n), kid


def test_scalar_modexp_equals_pow(lib):
    recs = {}
    seen = set()
    for kid, fmt, spki, sig, msg, expect, note in ITEMS:
        if not KEYS[kid]["accepted"]:
            continue
        if kid not in recs:
            recs[kid] = Rec()
            assert lib.hr_key_prepare(spki, len(spki), ctypes.byref(recs[kid]))
        rec = recs[kid]
        # a few signatures per key (a scalar 4096-bit modexp is slow): the first three and every s = ... case
        if sum(1 for s in seen if s[0] == kid) >= 3 and not note.startswith("s = "):
            continue
        seen.add((kid, note))
        n, e = hostverify.rsa_decode_key(spki)
        out = ctypes.create_string_buffer(4 * rec.L)
        rc = lib.hr_modexp(ctypes.byref(rec), sig, len(sig), out)
        s = int.from_bytes(sig, "big")
        if len(sig) > rec.k or s >= n:
            assert rc == -1, (kid, note)
        else:
            assert rc == 0 and int.from_bytes(out.raw, "big") == pow(s, e, n), (kid, note)


def test_emsa_pss_equals_restatement(lib):
    """rsa_pss_check over EM = s^e mod n (Python pow) for every item the restatement takes that far."""
    ran = 0
    for kid, fmt, spki, sig, msg, expect, note in ITEMS:
        if expect == "HOST_EXCEPTION":
            continue
        n, e = hostverify.rsa_decode_key(spki)
        bits = n.bit_length()
        block_len = (bits + 6) // 8
        s = int.from_bytes(sig, "big")
        if len(sig) > (bits + 7) // 8 or s >= n:
            continue
        m = pow(s, e, n)
        if m.bit_length() > 8 * block_len:
            continue
        em = m.to_bytes(block_len, "big")
        got = lib.hr_pss_check(em, block_len, bits - 1, hashlib.sha256(msg).digest())
        assert got == (1 if expect == "VALID" else 0), (kid, note)
        ran += 1
    assert ran > 150


def _vectors():
    out = []
    for kid, fmt, spki, sig, msg, expect, note in ITEMS:
        if KEYS[kid]["accepted"] or kid == "fmt_raw":
            want = 1 if expect == "VALID" else 0
        else:
            want = -1
        out.append((spki, sig, msg, want, kid, note))
    return out


def test_whole_verification_equals_restatement(lib):
    """Decode + scalar modexp + fit + EMSA-PSS, as the kernels chain them, for every fixture item."""
    for spki, sig, msg, want, kid, note in _vectors():
        assert lib.hr_verify(spki, len(spki), sig, len(sig), msg, len(msg)) == want, (kid, note)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same vectors through a stand-alone program built with AddressSanitizer + UBSan and run
    directly: no out-of-bounds read in the decode (truncated and garbage keys), no undefined shift."""
    exe = str(tmp_path / "host_rsa_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DHOST_RSA_MAIN", "-o", exe, SRC])
    vec = tmp_path / "vectors.bin"
    good = bytes.fromhex(KEYS["rsa1024"]["spki"])
    with open(vec, "wb") as f:
        for spki, sig, msg, want, kid, note in _vectors():
            if KEYS[kid].get("bits", 0) > 2048 and not note.startswith(("valid", "s = n")):
                continue  # keep the instrumented run short
            f.write(struct.pack("<IIIi", len(spki), len(sig), len(msg), want) + spki + sig + msg)
        for cut in list(range(0, 40)) + [len(good) - 5, len(good) - 1]:  # every truncation of the header
            f.write(struct.pack("<IIIi", cut, 1, 1, -1) + good[:cut] + b"\x01" + b"m")
    r = subprocess.run([exe, str(vec)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 mismatches" in r.stdout
