"""Key derivation on the CPU: the fixture against derive_ref, the host build of the lane code
(tests/native/host_derive.cpp, corda_amd/csrc/derive.h) at all three radixes with FE_BOUNDS_CHECK, the
same as a stand-alone program under the address and undefined-behaviour sanitizers, the host
restatement the Python mirror finishes CG_DERIVE_HOST items with, the request packer and the ABI."""
import ctypes
import hashlib
import hmac
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import derive_ref as R
import hostderive as H
from corda_amd import _lib
from corda_amd import batch as B
from corda_amd import derive as D
from oracle import ecdsa_bc, ed25519_i2p as ed

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
RADIX = pytest.mark.parametrize("bw", H.RADIXES)
KEYS = [bytes([7]), bytes([0, 0x80]), bytes(range(1, 31)), bytes(range(32)), bytes([0]) + bytes(range(200, 232)),
        bytes(range(127)), bytes(range(128))]
SEED_LENS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 32, 111, 112, 127, 128, 129, 239, 240, 300]


def seed_bytes(n):
    return bytes((7 * i + 3) & 255 for i in range(n))


@pytest.fixture(scope="module")
def fx():
    return H.fixture()


# ---------------------------------------------------------------- the fixture and the references
def test_fixture_shape_and_reference(fx):
    ps, rs = fx["parents"], fx["records"]
    assert len(ps) == 14 and len(rs) == 280
    assert sorted({len(bytes.fromhex(p["key_data"])) for p in ps if p["scheme"] != R.ED}) == [1, 2, 30, 33]
    for p in ps:
        private = bytes.fromhex(p["private"])
        want = R.key_data_ed(private) if p["scheme"] == R.ED else R.key_data_ec(int.from_bytes(private, "big"))
        assert bytes.fromhex(p["key_data"]) == want == D.key_data(p["scheme"], private)
    lens = {len(bytes.fromhex(r["seed"])) for r in rs}
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8, 32, 111, 112, 127, 128, 129, 239, 240, 4096} <= lens
    for r in rs[::7]:
        p = ps[r["parent"]]
        secret, pub, tries = R.derive(p["scheme"], bytes.fromhex(p["key_data"]), bytes.fromhex(r["seed"]))
        assert (secret.hex(), pub.hex(), tries) == (r["secret"], r["pub"], r["retries"])


def test_host_restatement_equals_the_reference():
    for scheme in (R.K1, R.R1):
        n = ecdsa_bc.CURVES[scheme].n
        for d in (0, 1, 2, n - 1, n, 2 ** 255, sum(1 << (4 * i) for i in range(63)), sum(1 << (4 * i) for i in range(64))):
            assert D.accepts(scheme, d) == R.accepts(scheme, d)
        key = R.key_data_ec(n - 7)
        for force in (0, 1, 6):
            assert D.derive_ecdsa(scheme, key, b"seed-1", force) == R.derive(scheme, key, b"seed-1", force)
    with pytest.raises(ValueError):
        D.key_data(1, bytes(32))
    # its own point arithmetic on the table-edge scalars and the accept cases
    for scheme in (R.K1, R.R1):
        c = ecdsa_bc.CURVES[scheme]
        for _, d in H.crafted_scalars(22, c.n) + H.crafted_scalars(26, c.n):
            assert D.public_point(scheme, d) == ecdsa_bc.ec_mul(c, d, c.G)
        assert D.public_point(scheme, c.n) is None and D.public_point(scheme, 0) is None
        for d, ok in accept_cases(scheme):
            assert D.accepts(scheme, d) == ok


def test_request_builder_forms_key_data_and_wipes():
    b = B.DeriveRequestBuilder()
    d = 2 ** 255 + 5
    p0 = b.parent(R.R1, d.to_bytes(32, "big"))
    p1 = b.parent(R.ED, ed.entropy_seed(20))
    b.add_request(p0, b"seed-1")
    b.add_request(p1, b"")
    dr = b.build()
    assert dr.parents.dtype.itemsize == 16 and dr.reqs.dtype.itemsize == 16 and dr.n == 2
    k0 = dr.arena[int(dr.parents["key_off"][0]):][:int(dr.parents["key_len"][0])].tobytes()
    k1 = dr.arena[int(dr.parents["key_off"][1]):][:int(dr.parents["key_len"][1])].tobytes()
    assert k0 == b"\x00" + d.to_bytes(32, "big") and k1 == R.key_data_ed(ed.entropy_seed(20))
    assert list(dr.reqs["seed_len"]) == [6, 0] and list(dr.reqs["parent"]) == [0, 1]
    dr.wipe()
    assert not dr.arena.any()


# ---------------------------------------------------------------- the lane code, host build
@needs_gxx
@RADIX
def test_hmac_lanes_against_hmac(bw):
    for key in KEYS:
        for n in SEED_LENS:
            msg = seed_bytes(n)
            want = hmac.new(key, msg, hashlib.sha512).digest()
            for phase in range(4):
                assert H.hmac512(bw, key, msg, phase) == want, (len(key), n, phase)
    # the rehashed forms: the SHA-256 of short and multi-block seeds, then a digest of a digest
    for n in (0, 6, 55, 56, 64, 129):
        msg = seed_bytes(n)
        s1 = hashlib.sha256(msg).digest()
        s2 = hashlib.sha256(s1).digest()
        for phase in range(4):
            assert H.hmac512_rehashed(bw, KEYS[3], msg, phase) == (hmac.new(KEYS[3], s1, hashlib.sha512).digest(),
                                                                  hmac.new(KEYS[3], s2, hashlib.sha512).digest())


def accept_cases(scheme):
    """(d, accepted). sum of 2^(4i) over k terms: 3d xor d has one bit per term, so its weight is k."""
    n = ecdsa_bc.CURVES[scheme].n
    w63, w64 = sum(1 << (4 * i) for i in range(63)), sum(1 << (4 * i) for i in range(64))
    assert (R.naf_weight(w63), R.naf_weight(w64), R.naf_weight(2 ** 255)) == (63, 64, 1) and w64 < n
    return [(0, False), (1, False), (2, False), (n - 1, R.naf_weight(n - 1) >= 64), (n, False), (n + 1, False),
            (2 ** 256 - 1, False), (2 ** 255, False), (w63, False), (w64, True)]


@needs_gxx
@RADIX
@pytest.mark.parametrize("scheme", [R.K1, R.R1])
def test_accept_rule(bw, scheme):
    for d, ok in accept_cases(scheme):
        assert R.accepts(scheme, d) == ok, hex(d)
        assert H.accept(bw, scheme, d) == ok, hex(d)


@needs_gxx
@RADIX
@pytest.mark.parametrize("scheme", [R.K1, R.R1])
def test_d_times_g_at_the_table_edges(bw, scheme):
    c = ecdsa_bc.CURVES[scheme]
    rows = H.g_digits(bw)
    half = 1 << (bw - 1)
    seen_zero, seen_last, seen_carry = set(), set(), False
    for note, d in H.crafted_scalars(bw, c.n):
        xy, digits = H.ec_fixed_base(bw, scheme, d)
        q = ecdsa_bc.ec_mul(c, d, c.G)
        assert xy == q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"), note
        assert digits == H.recode(d, bw), note
        seen_zero |= {u for u, e in enumerate(digits) if e == 0}
        seen_last |= {u for u, e in enumerate(digits) if e == -half}
        raw = [(d >> (bw * t)) & ((1 << bw) - 1) for t in range(rows)]
        seen_carry = seen_carry or all(r >= half for r in raw[:rows - 1])
    assert {0, rows // 2, rows - 1} <= seen_zero
    assert set(range(rows - 1)) <= seen_last and seen_carry
    assert H.ec_fixed_base(bw, scheme, 0)[0] is None and H.ec_fixed_base(bw, scheme, c.n)[0] is None  # infinity


def refused_mac(scheme, kind):
    n = ecdsa_bc.CURVES[scheme].n
    d = {0: 1, 1: n, 2: 2 ** 255, 3: 0, 4: n + 5}[kind % 5]
    return d.to_bytes(32, "big") + bytes([kind]) * 32


def good_mac(tag):
    d = int.from_bytes(hashlib.sha256(b"good %d" % tag).digest(), "big") >> 1
    assert R.accepts(R.K1, d) and R.accepts(R.R1, d)
    return d.to_bytes(32, "big") + bytes(32)


@needs_gxx
@RADIX
@pytest.mark.parametrize("scheme", [R.K1, R.R1])
def test_retry_lane_with_injected_macs(bw, scheme):
    """Attempts 0 .. k - 1 refused by their own d (each kind of refusal), attempt k accepted: k rehashes,
    up to the cap; with every attempt refused, CG_DERIVE_HOST after exactly MAX_RETRIES rehashes."""
    for k in range(R.MAX_RETRIES + 2):
        macs = [refused_mac(scheme, a) if a < k else good_mac(a) for a in range(R.MAX_RETRIES + 1)]
        st, d, tries, calls = H.derive_attempts(bw, scheme, macs)
        if k <= R.MAX_RETRIES:
            assert (st, d, tries, calls) == (0, macs[k][:32], k, k), k
        else:
            assert (st, tries, calls) == (R.DERIVE_HOST, R.MAX_RETRIES, R.MAX_RETRIES)
    # the hook refuses attempts whatever their d
    macs = [good_mac(a) for a in range(R.MAX_RETRIES + 1)]
    for force in range(R.MAX_RETRIES + 2):
        st, d, tries, calls = H.derive_attempts(bw, scheme, macs, force)
        want = (0, macs[force][:32], force, force) if force <= R.MAX_RETRIES else \
            (R.DERIVE_HOST, macs[-1][:32], R.MAX_RETRIES, R.MAX_RETRIES)
        assert (st, d, tries, calls) == want, force


@needs_gxx
@RADIX
def test_item_lanes_against_the_reference(bw, fx):
    ps = fx["parents"]
    for r in fx["records"][::11]:
        p = ps[r["parent"]]
        key, seed = bytes.fromhex(p["key_data"]), bytes.fromhex(r["seed"])
        for phase in (0, 3):
            if p["scheme"] == R.ED:
                assert H.derive_ed(bw, key, seed, phase) == (bytes.fromhex(r["secret"]), bytes.fromhex(r["pub"])[:32])
            else:
                assert H.derive_ec(bw, p["scheme"], key, seed, 0, phase) == \
                    (0, bytes.fromhex(r["secret"]), bytes.fromhex(r["pub"]), 0)
    for scheme in (R.K1, R.R1):
        key = R.key_data_ec(ecdsa_bc.CURVES[scheme].n - 11)
        for force in (1, 2, R.MAX_RETRIES, R.MAX_RETRIES + 1):
            for n in (0, 6, 129):
                assert H.derive_ec(bw, scheme, key, seed_bytes(n), force, 1) == \
                    R.device_expect(scheme, key, seed_bytes(n), force), (scheme, force, n)
    for e in (20, 70, 80):
        assert H.ed_public(bw, ed.entropy_seed(e)) == ed.public_from_seed(ed.entropy_seed(e))


@needs_gxx
@RADIX
def test_sanitized_stand_alone_program(bw, fx, tmp_path):
    """The same lane code as a program with its own main under the address and undefined-behaviour
    sanitizers, run directly: every arena is an exact-size heap block, so a load past the rounded end of
    a seed or key is reported."""
    exe = H.sanitized_main(bw)
    ps, lines = fx["parents"], []
    hx = lambda b: b.hex() if b else "-"  # noqa: E731
    for r in fx["records"][::5]:
        p = ps[r["parent"]]
        lines.append(f"H {p['key_data']} {hx(bytes.fromhex(r['seed']))} {r['mac']}")
        lines.append(f"D {p['scheme']} 0 {p['key_data']} {hx(bytes.fromhex(r['seed']))} 0 {r['secret']} {r['pub']} 0")
    for scheme in (R.K1, R.R1):
        c = ecdsa_bc.CURVES[scheme]
        for d, _ in accept_cases(scheme):
            lines.append(f"A {scheme} {d.to_bytes(32, 'big').hex()} {int(R.accepts(scheme, d))}")
        for _, d in H.crafted_scalars(bw, c.n):
            q = ecdsa_bc.ec_mul(c, d, c.G)
            lines.append(f"G {scheme} {d.to_bytes(32, 'big').hex()} {(q[0].to_bytes(32, 'big') + q[1].to_bytes(32, 'big')).hex()}")
        key = R.key_data_ec(c.n - 11)
        for force in (1, R.MAX_RETRIES, R.MAX_RETRIES + 1):
            for n in (0, 6, 129):
                st, secret, pub, tries = R.device_expect(scheme, key, seed_bytes(n), force)
                lines.append(f"D {scheme} {force} {key.hex()} {hx(seed_bytes(n))} {st} {secret.hex()} {pub.hex()} {tries}")
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()[-2000:]
    assert out.stdout.decode().strip() == f"{len(lines)} cases, 0 mismatches"


# ---------------------------------------------------------------- the ABI
def test_abi_structs_symbols_and_loud_failure():
    src = open(_lib.HEADER_PATH).read()
    assert "} cg_derive_parent;  /* 16 bytes */" in src and "} cg_derive_req;      /* 16 bytes */" in src
    assert [B.DERIVE_PARENT_DTYPE.fields[f][1] for f in ("key_off", "key_len", "scheme", "pad")] == [0, 8, 10, 11]
    assert [B.DERIVE_REQ_DTYPE.fields[f][1] for f in ("seed_off", "seed_len", "parent")] == [0, 8, 12]
    for name, code in (("CG_DERIVE_HOST", B.DERIVE_HOST), ("CG_DERIVE_BAD_PARENT", B.DERIVE_BAD_PARENT),
                       ("CG_KEY_REJECTED", B.KEY_REJECTED)):
        assert re.search(rf"\b{name} = {code}\b", src), name
    assert re.search(r"#define CG_DERIVE_MAX_RETRIES 4\b", src) and B.DERIVE_MAX_RETRIES == R.MAX_RETRIES == 4
    assert (R.DERIVE_HOST, R.BAD_PARENT, R.KEY_REJECTED) == (B.DERIVE_HOST, B.DERIVE_BAD_PARENT, B.KEY_REJECTED)
    L = _lib.lib()
    for name in ("cg_derive_keys", "cg_derive_keys_device", "cg_public_keys", "cg_public_keys_device",
                 "cg_pool_derive_keys", "cg_pool_public_keys"):
        assert name in _lib.declared_symbols() and hasattr(L, name), name
    one = np.zeros(64, np.uint8)
    p = one.ctypes.data_as(ctypes.c_void_p)
    assert L.cg_derive_keys(None, p, 1, p, 1, p, 8, p, p, p, None) == -1
    assert L.cg_public_keys(None, 4, p, 1, p, p) == -1
    assert L.cg_pool_derive_keys(None, p, 1, p, 1, p, 8, p, p, p, None, None) == -1
    assert b"ctx is NULL" in L.cg_last_error() or b"pool is NULL" in L.cg_last_error()


def test_kotlin_binding_derives_through_both_handles():
    """CryptoBatch.deriveAll / publicKeys (not compiled here: no JDK): natives that take (ctx, pool, ...),
    called inside withHandles with both, the direct buffers that held key bytes zeroed, every other case
    left to Crypto.deriveKeyPair on the JVM. tests/test_jvm_binding.py type-checks the JNI functions."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kt = open(os.path.join(root, "jvm/src/main/kotlin/net/corda/core/crypto/CryptoBatch.kt")).read()
    jni = open(os.path.join(root, "jvm/jni/cordagpu_jni.c")).read()
    for ext in ("nativeDeriveKeys", "nativePublicKeys"):
        decl = re.search(rf"external fun {ext}\((.*?)\): Int", kt, re.S).group(1)
        assert decl.replace(" ", "").startswith("ctx:Long,pool:Long,"), ext
        assert re.search(rf"withHandles {{ c, p ->\s*{ext}\(c, p,", kt), ext
    for fn in ("cg_derive_keys", "cg_pool_derive_keys", "cg_public_keys", "cg_pool_public_keys"):
        assert fn + "(" in jni, fn
    body = kt[kt.index("fun deriveAll("):kt.index("fun publicKeys(")]
    assert "fun deriveAll(privateKey: PrivateKey, seeds: List<ByteArray>): List<KeyPair>" in body
    assert "wipe(arena); wipe(secrets); keyData.fill(0)" in body and "finally" in body
    assert "Crypto.deriveKeyPair(privateKey, seed)" in body and "else onJvm(seed)" in body
    assert "wipe(secrets)" in kt[kt.index("fun publicKeys("):]
    for name, code in (("CG_DERIVE_HOST", 6), ("CG_DERIVE_BAD_PARENT", 7), ("CG_KEY_REJECTED", 8)):
        assert f"const val {name} = {code}" in kt


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="CPU-only behaviour")
def test_without_a_gpu_the_mirror_fails_loudly():
    from corda_amd.crypto import Crypto, PrivateKey
    from corda_amd.engine import Engine
    with pytest.raises(_lib.EngineUnavailable):
        Engine(0).derive_keys(B.DeriveRequestBuilder().build())
    if Crypto._engine is None:
        with pytest.raises(_lib.EngineUnavailable):
            Crypto.derive_key_pair(PrivateKey(R.ED, bytes(32)), b"seed-1")
