"""CPU tests of the RSA-PSS signer: the fixture tests/golden/rsa_sign.json against the reference
(hostverify.rsa_pss_sign / rsa_verify, Python integers); the HIP-free EMSA-PSS encode of corda_amd/csrc/rsa.h
through the stand-alone program tests/native/host_rsa_sign.cpp, plain and under the address and
undefined-behaviour sanitizers, against every fixture `em`; the C ABI's declarations; the Python mirror
through a fake engine (the PKCS#8 parse, one random(32) per signature, the refusals); and the test-only device
library's Makefile."""
import ctypes
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import hostsignrsa as H
from corda_amd import _lib, hostverify, signable
from corda_amd import batch as B
from corda_amd import crypto as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "host_rsa_sign.cpp")
HDR = open(_lib.HEADER_PATH).read()


# ---------------------------------------------------------------- the fixture
def test_fixture_covers_the_sizes_cases_and_equals_the_reference():
    fx = H.fixture()
    keys = fx["keys"]
    assert [keys[k]["bits"] for k in H.SIZES] == [1024, 1025, 1032, 2048, 2048, 3072, 4096]
    assert H.key("rsa2048e3")["e"] == 3
    k1025 = H.key("rsa1025")
    assert k1025["p"].bit_length() != k1025["q"].bit_length() and (1025 + 6) // 8 == (1025 + 7) // 8 - 1
    for kid in ("rsa1024", "rsa3072"):  # both orders of the primes
        a, b = H.key(kid), H.key(kid + "_swapped")
        assert (a["p"], a["q"]) == (b["q"], b["p"]) and (a["p"] > a["q"]) != (b["p"] > b["q"])
    for kid in keys:
        k = H.key(kid)
        assert k["p"] * k["q"] == k["n"] and k["dp"] == k["d"] % (k["p"] - 1) and k["dq"] == k["d"] % (k["q"] - 1)
        assert k["qinv"] * k["q"] % k["p"] == 1
    recs = H.records()
    assert {len(r["msg"]) for r in recs} == {1, 55, 56, 64, 270, 700}
    assert {bytes(32), b"\xff" * 32} < {r["salt"] for r in recs}
    for kid in keys:
        mine = [r for r in recs if r["key"] == kid]
        assert len(mine) == 6 and len({r["salt"] for r in mine}) >= 3
    for r in recs:
        k = H.key(r["key"])
        assert r["sig"] == hostverify.rsa_pss_sign(k["n"], k["d"], r["msg"], r["salt"])
        assert int.from_bytes(r["sig"], "big") == pow(int.from_bytes(r["em"], "big"), k["d"], k["n"])
        assert hostverify.rsa_verify((k["n"], k["e"]), r["sig"], r["msg"])
    assert [(i, s) for i, s, _ in H.refused()] == [("dp_plus_2", 3), ("n_plus_2", 3), ("even_p", 3), ("e_zero", 3),
                                                   ("n_1016_bits", 4)]
    assert os.path.getsize(os.path.join(HERE, "golden", "rsa_sign.json")) < 256 * 1024


# ---------------------------------------------------------------- rsa.h's encode on the host
def _vectors(path, corrupt=False):
    with open(path, "wb") as f:
        for j, r in enumerate(H.records()):
            em = bytearray(r["em"])
            if corrupt and j == 7:
                em[5] ^= 1
            f.write(struct.pack("<I", H.fixture()["keys"][r["key"]]["bits"]) + hashlib.sha256(r["msg"]).digest() +
                    r["salt"] + bytes(em))


@pytest.mark.parametrize("san", [False, True])
def test_emsa_pss_encode_equals_every_fixture_em(san, tmp_path):
    """san: built with AddressSanitizer + UBSan and run directly: no byte outside the exactly-sized EM buffer is
    touched (block_len = k - 1 at 1025 bits), no undefined shift."""
    exe = str(tmp_path / "host_rsa_sign")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if san else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", *flags, "-o", exe, SRC])
    vec = str(tmp_path / "vectors.bin")
    _vectors(vec)
    r = subprocess.run([exe, vec], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "54 vectors, 0 mismatches" in r.stdout
    if not san:  # the program does report a wrong byte
        _vectors(vec, corrupt=True)
        r = subprocess.run([exe, vec], capture_output=True, text=True)
        assert r.returncode == 1 and "54 vectors, 1 mismatches" in r.stdout


# ---------------------------------------------------------------- the C ABI
def test_header_block_and_declarations():
    assert re.search(r"#define CG_SIGN_CHECK_FAILED 10\b", HDR) and re.search(r"#define CG_RSA_SIG_MAX 512\b", HDR)
    assert B.SIGN_CHECK_FAILED == H.SIGN_CHECK_FAILED == 10 and "#define CG_ABI_VERSION 2" in HDR
    assert "} cg_rsa_signer;     /* 52 bytes */" in HDR
    from corda_amd.engine import RSA_SIGNER_DTYPE
    m = re.search(r"typedef struct cg_rsa_signer \{(.*?)\} cg_rsa_signer;", HDR, re.S)
    fields = re.findall(r"\b(\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert tuple(fields) == RSA_SIGNER_DTYPE.names and RSA_SIGNER_DTYPE.itemsize == 52
    block = HDR[HDR.index("---- RSA-PSS signing"):HDR.index("---- Key derivation")]
    for cite in ("Crypto.kt:395-402", "Crypto.kt:415-422", "PSSSigner", "RSABlindedEngine", "[recalled]", "linding",
                 "Not constant-time", "window digit", "conditional subtraction", "CG_SIGN_CHECK_FAILED"):
        assert cite in block, cite
    assert "RSA-PSS signing stays on the" not in HDR
    for fn, n_args in (("cg_rsa_signers_load", 6), ("cg_rsa_signers_clear", 1), ("cg_rsa_sign_tx_ids", 13),
                       ("cg_rsa_sign_tx_ids_device", 14), ("cg_rsa_sign_batch", 9), ("cg_pool_rsa_signers_load", 6),
                       ("cg_pool_rsa_signers_clear", 1), ("cg_pool_rsa_sign_tx_ids", 14)):
        m = re.search(r"\bint %s\(([^;]*)\);" % fn, HDR)
        assert m and len(m.group(1).split(",")) == n_args, fn


def test_symbols_exported_and_null_ctx_is_an_argument_error():
    lb = _lib.lib()
    for name in ("cg_rsa_signers_load", "cg_rsa_signers_clear", "cg_rsa_sign_tx_ids", "cg_rsa_sign_tx_ids_device",
                 "cg_rsa_sign_batch", "cg_pool_rsa_signers_load", "cg_pool_rsa_signers_clear", "cg_pool_rsa_sign_tx_ids"):
        assert name in _lib.declared_symbols() and hasattr(lb, name), name
    assert lb.cg_abi_version() == 2
    buf = np.zeros(1024, dtype=np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lb.cg_rsa_signers_load(None, p, 1, p, 64, p) == -1
    assert lb.cg_rsa_signers_clear(None) == -1
    assert lb.cg_rsa_sign_tx_ids(None, p, 1, p, 1, None, 0, None, 0, p, p, p, p) == -1
    assert lb.cg_rsa_sign_tx_ids_device(None, p, 1, p, 1, None, 0, None, 0, p, p, p, p, None) == -1
    assert lb.cg_rsa_sign_batch(None, p, 1, p, 8, p, p, p, p) == -1
    assert lb.cg_pool_rsa_signers_load(None, p, 1, p, 64, p) == -1
    assert lb.cg_pool_rsa_signers_clear(None) == -1
    assert lb.cg_pool_rsa_sign_tx_ids(None, p, 1, p, 1, None, 0, None, 0, p, p, p, p, None) == -1
    assert (buf == 0).all() and "NULL" in _lib.last_error()


def test_sources_are_built_once_and_listed():
    mk = open(os.path.join(ROOT, "corda_amd", "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "rsa_sign_wave.h" in hdrs and "build/sign_rsa.o" in mk
    for var in ("VARIANT_SRCS", "DERIVE_SRCS", "SIGN_EC_SRCS"):  # radix-independent: not a variant source
        assert "sign_rsa" not in re.search(rf"^{var}\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^resources:.*\n.*\bsign_rsa\b", mk, re.M)
    # the test-only device library: the product's flags, rebuilt when a header it instantiates changes
    tmk = open(os.path.join(HERE, "native_rsa_sign", "Makefile")).read()
    flags = lambda text: re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, re.M).group(1).split()  # noqa: E731
    assert flags(tmk) == flags(mk)
    assert re.search(r"^\$\(OUT\):.*rsa_sign_wave_gpu\.hip.*rsa_sign_wave\.h.*rsa_wave\.h", tmk, re.M)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '_make("tests/native_rsa_sign"' in entry


# ---------------------------------------------------------------- the mirror, through a fake engine
class _FakeEngine:
    """An engine stand-in that signs with the reference: the mirror's parse, key-pair check and draws without
    a GPU."""

    def __init__(self):
        self.keys, self.loads, self.calls, self.salt_arrays = [], 0, [], []

    def load_rsa_signers(self, keys):
        self.keys, self.loads = [tuple(int.from_bytes(bytes(v), "big") if f != "e" else v
                                       for f, v in zip(k._fields, k)) for k in keys], self.loads + 1
        return np.array([0 if p * q == n else H.KEY_INVALID for n, e, p, q, dp, dq, qinv in self.keys], dtype=np.uint8)

    def clear_rsa_signers(self):
        self.keys = []

    def _sign(self, signer_msgs, salts):
        n = len(signer_msgs)
        assert isinstance(salts, np.ndarray) and salts.dtype == np.uint8 and salts.size == 32 * n
        self.calls.append(n)
        self.salt_arrays.append(salts)
        sigs, ln, st = np.zeros((n, 512), dtype=np.uint8), np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint8)
        for j, (i, m) in enumerate(signer_msgs):
            nn, e, p, q, dp, dq, qinv = self.keys[i]
            d = pow(e, -1, (p - 1) * (q - 1))
            sig = hostverify.rsa_pss_sign(nn, d, m, salts[32 * j:32 * j + 32].tobytes())
            sigs[j, :len(sig)], ln[j] = np.frombuffer(sig, dtype=np.uint8), len(sig)
        salts[:] = 0  # as Engine.sign_rsa does with the array the C ABI read
        return sigs, ln, st

    def sign_rsa(self, signer_msgs, salts):
        return self._sign(signer_msgs, salts)

    def sign_rsa_tx_ids(self, sr, salts):
        msgs = []
        for q in sr.reqs:
            t = sr.tmpls[int(q["tmpl"])]
            pre = bytes(sr.arena[int(t["prefix_off"]):int(t["prefix_off"]) + int(t["prefix_len"])])
            suf = bytes(sr.arena[int(t["suffix_off"]):int(t["suffix_off"]) + int(t["suffix_len"])])
            i = int(q["tx_idx"])
            msgs.append((int(q["signer"]), pre + bytes(sr.ids[32 * i:32 * i + 32]) + suf))
        return self._sign(msgs, salts)


class _Draws:
    def __init__(self, draws):
        self.draws, self.used = list(draws), 0

    def __call__(self, nbytes):
        assert nbytes == 32
        self.used += 1
        return self.draws[self.used - 1]


def _pair(kid):
    k = H.fixture()["keys"][kid]
    return C.KeyPair(C.PublicKey(C.RSA_SHA256, bytes.fromhex(k["spki"]), B.KEY_SPKI),
                     C.PrivateKey(C.RSA_SHA256, bytes.fromhex(k["pkcs8"])))


def test_pkcs8_parse_gives_the_fixture_numbers():
    for kid in H.SIZES:
        got = hostverify.rsa_decode_private_key(bytes.fromhex(H.fixture()["keys"][kid]["pkcs8"]))
        assert got == H.key(kid), kid
    with pytest.raises(hostverify.InvalidKeySpecException):
        hostverify.rsa_decode_private_key(bytes.fromhex(H.fixture()["keys"]["rsa1024"]["pkcs8"])[:-1])
    with pytest.raises(hostverify.InvalidKeySpecException):
        hostverify.rsa_decode_private_key(bytes.fromhex(H.fixture()["keys"]["rsa1024"]["spki"]))


def test_mirror_without_random_still_refuses_rsa_keys():
    cr = C._Crypto()
    cr.use_engine(_FakeEngine())
    pair = _pair("rsa1024")
    with pytest.raises(C.UnsupportedOperationException):
        cr.do_sign(pair.private, b"data")
    with pytest.raises(C.UnsupportedOperationException):
        cr.sign_all(pair, [bytes(32)], (1, 1))
    with pytest.raises(C.UnsupportedOperationException):
        cr.do_sign_tx(pair, C.SignableData(bytes(32), 1, 1))
    with pytest.raises(Exception, match="Signing of an empty array is not permitted!"):
        cr.do_sign(pair.private, b"", random=lambda n: bytes(n))  # doSign's order: the empty check first


def test_mirror_draws_one_salt_per_signature_and_never_redraws():
    cr, fake = C._Crypto(), _FakeEngine()
    cr.use_engine(fake)
    r = next(x for x in H.records() if x["key"] == "rsa2048" and len(x["msg"]) == 270)
    draws = _Draws([r["salt"], b"\x01" * 32])
    assert cr.do_sign(_pair("rsa2048").private, r["msg"], random=draws) == r["sig"]
    assert draws.used == 1 and fake.calls == [1] and fake.loads == 1
    assert all((a == 0).all() for a in fake.salt_arrays)  # the arrays handed down come back zeroed
    # transaction ids: one draw each, in request order; the second key joins the loaded set
    pair = _pair("rsa1025")
    ids = [hashlib.sha256(bytes([k])).digest() for k in range(4)]
    salts = [hashlib.sha256(b"salt %d" % j).digest() for j in range(4)]
    draws = _Draws(salts + [b"\x02" * 32])
    out = cr.sign_all(pair, ids, (1, 1), random=draws)
    pre, suf = signable.template(1, 1)
    assert draws.used == 4 and fake.calls == [1, 4] and fake.loads == 2
    for ts, i, s in zip(out, ids, salts):
        assert ts.bytes == H.sign("rsa1025", pre + i + suf, s) and len(ts.bytes) == 129
        assert ts.by == pair.public and (ts.platform_version, ts.scheme_number_id) == (1, 1)
    one = cr.do_sign_tx(pair, C.SignableData(ids[0], 1, 1), random=_Draws([salts[0]]))
    assert one.bytes == out[0].bytes and fake.loads == 2
    cr.forget_signers()
    assert fake.keys == []


def test_mirror_refusals():
    cr, fake = C._Crypto(), _FakeEngine()
    cr.use_engine(fake)
    rnd = lambda n: bytes(n)  # noqa: E731
    big_e = C.PrivateKey(C.RSA_SHA256, bytes.fromhex(H.fixture()["pkcs8_big_e"]))
    assert hostverify.rsa_decode_private_key(big_e.encoded)["e"] == (1 << 32) + 1
    with pytest.raises(C.UnsupportedOperationException, match="2\\^32"):
        cr.do_sign(big_e, b"data", random=rnd)
    # a key without CRT parts (BC writes zeros for them)
    from corda_amd import der
    k = H.key("rsa1024")
    body = der.tlv(0x30, b"".join(der.integer(v) for v in (0, k["n"], k["e"], k["d"], 0, 0, 0, 0, 0)))
    alg = der.tlv(0x30, hostverify.RSA_OID + der.tlv(0x05, b""))
    no_crt = C.PrivateKey(C.RSA_SHA256, der.tlv(0x30, der.integer(0) + alg + der.tlv(0x04, body)))
    with pytest.raises(C.UnsupportedOperationException, match="CRT"):
        cr.do_sign(no_crt, b"data", random=rnd)
    with pytest.raises(C.InvalidKeySpecException):
        cr.do_sign(C.PrivateKey(C.RSA_SHA256, b"\x30\x00"), b"data", random=rnd)
    assert fake.loads == 0  # refused before anything is loaded
    # the key-pair check: the public key must be (n, e) of the private key
    a, b = _pair("rsa1024"), _pair("rsa1032")
    with pytest.raises(C.IllegalArgumentException, match="not the private key's"):
        cr.sign_all(C.KeyPair(b.public, a.private), [bytes(32)], (1, 1), random=rnd)
    with pytest.raises(C.IllegalArgumentException, match="is not aligned with the key type"):
        cr.sign_all(C.KeyPair(C.PublicKey(4, bytes(32)), a.private), [bytes(32)], (1, 1), random=rnd)
    with pytest.raises(ValueError, match="32 bytes"):
        cr.do_sign(a.private, b"data", random=lambda n: b"short")
