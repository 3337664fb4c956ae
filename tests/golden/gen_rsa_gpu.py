"""Generates tests/golden/rsa_gpu.json: RSA_SHA256 (SHA256WITHRSAANDMGF1) fixtures for the GPU path
(Engine(rsa=True), corda_amd/csrc/verify_rsa.hip, rsa.h). Keys come from the OpenSSL CLI at the bit
lengths where the kernel takes another path (1024 the minimum, 1025: block_len = k - 1, 1032: a bit
length that is no multiple of 32, 2048 with e = 3, 3072, 4096 the maximum), plus the keys the device
decode must decline (1016 and 4104 bits, and malformed / out-of-range encodings of a good key).
Signatures and crafted encodings are made with hostverify.rsa_pss_sign's arithmetic and the test-only
private exponents. Every item carries `expect`, the BC 1.57 restatement's outcome
(hostverify.rsa_verify: VALID / INVALID, or HOST_EXCEPTION when the key does not decode there), and
`openssl`, OpenSSL's own PSS verdict where OpenSSL can be asked (a key it can load).

Layout: {"keys": {id: {spki, bits, accepted, n, e, d, note}}, "items": [{key, key_fmt, sig, msg,
note, expect, openssl}]}: the keys are stored once.

usage: python tests/golden/gen_rsa_gpu.py  (needs the openssl CLI)
"""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from corda_amd import der, hostverify  # noqa: E402

PSS = ["-sigopt", "rsa_padding_mode:pss", "-sigopt", "rsa_pss_saltlen:32", "-sigopt", "rsa_mgf1_md:sha256"]
RSA_ALG = der.oid("1.2.840.113549.1.1.1")
NULL = der.tlv(0x05, b"")


def sh(*args, data=None):
    return subprocess.run(args, input=data, capture_output=True, check=True).stdout


def ossl_verify(pub_der, msg, sig, d):
    kp, mp, sp = (os.path.join(d, n) for n in ("k.der", "m.bin", "s.bin"))
    open(kp, "wb").write(pub_der)
    open(mp, "wb").write(msg)
    open(sp, "wb").write(sig)
    r = subprocess.run(["openssl", "dgst", "-sha256", "-keyform", "DER", "-verify", kp] + PSS +
                       ["-signature", sp, mp], capture_output=True)
    if b"unable to load" in r.stderr or b"Could not read" in r.stderr or b"Could not find" in r.stderr:
        return "n/a"
    return "accept" if r.returncode == 0 else "reject"


def gen_key(bits, e, d):
    """(spki, n, e, d) of a fresh key whose modulus has exactly `bits` bits."""
    for _ in range(64):
        key = os.path.join(d, "k.pem")
        sh("openssl", "genpkey", "-algorithm", "RSA", "-pkeyopt", f"rsa_keygen_bits:{bits}", "-pkeyopt",
           f"rsa_keygen_pubexp:{e}", "-out", key)
        pub = sh("openssl", "pkey", "-in", key, "-pubout", "-outform", "DER")
        txt = sh("openssl", "pkey", "-in", key, "-text", "-noout").decode()

        def field(name, nxt):
            body = txt.split(name + ":")[1].split(nxt)[0]
            return int("".join(body.split()).replace(":", ""), 16)
        n = field("modulus", "publicExponent")
        dd = field("privateExponent", "prime1")
        if n.bit_length() == bits:
            assert hostverify.rsa_decode_key(pub) == (n, e)
            return pub, n, e, dd
    raise RuntimeError(f"no {bits}-bit modulus from openssl")


def rsa_spki(n, e, params=NULL, alg=RSA_ALG):
    return der.spki(alg, params, der.tlv(0x30, der.integer(n) + der.integer(e)))


def em_encode(n, msg, salt, trailer=0xBC, pad_byte=None, marker=0x01, top_bit=False):
    """EMSA-PSS-ENCODE with MGF1-SHA256 for modulus n (hostverify.rsa_pss_sign), with faults."""
    em_bits = n.bit_length() - 1
    block_len = (em_bits + 7) // 8
    mh = hashlib.sha256(bytes(8) + hashlib.sha256(bytes(msg)).digest() + bytes(salt)).digest()
    db = bytearray(block_len - len(salt) - 32 - 2) + bytes([marker]) + bytes(salt)
    if pad_byte is not None:
        db[pad_byte] = 0x5A
    masked = bytearray(a ^ b for a, b in zip(db, hostverify.mgf1_sha256(mh, len(db))))
    masked[0] &= 0xFF >> (8 * block_len - em_bits)
    if top_bit:
        masked[0] |= 0x80  # a bit above emBits (8 * block_len > em_bits)
    return bytes(masked) + mh + bytes([trailer])


def sign_em(em, n, d):
    return pow(int.from_bytes(em, "big"), d, n).to_bytes((n.bit_length() + 7) // 8, "big")


def v15(n, d, msg):
    k = (n.bit_length() + 7) // 8
    di = bytes.fromhex("3031300d060960864801650304020105000420") + hashlib.sha256(msg).digest()
    em = b"\x00\x01" + b"\xff" * (k - 3 - len(di)) + b"\x00" + di
    return sign_em(em, n, d)


def main():
    rng = random.Random(0x25A6)
    rb = lambda ln: bytes(rng.randrange(256) for _ in range(ln))  # noqa: E731
    keys, items = {}, []
    with tempfile.TemporaryDirectory() as d:
        def add(key, sig, msg, note, key_fmt=1):
            k = keys[key]
            spki = bytes.fromhex(k["spki"])
            try:
                exp = "VALID" if hostverify.rsa_verify(hostverify.rsa_decode_key(spki), sig, msg) else "INVALID"
            except hostverify.InvalidKeySpecException:
                exp = "HOST_EXCEPTION"
            items.append({"key": key, "key_fmt": key_fmt, "sig": sig.hex(), "msg": msg.hex(), "note": note,
                          "expect": exp, "openssl": ossl_verify(spki, msg, sig, d)})
            return exp

        good = []
        for bits, e in ((1024, 65537), (1025, 65537), (1032, 65537), (2048, 3), (3072, 65537), (4096, 65537)):
            pub, n, e, dd = gen_key(bits, e, d)
            kid = f"rsa{bits}" + ("e3" if e == 3 else "")
            keys[kid] = {"spki": pub.hex(), "bits": bits, "accepted": True, "n": hex(n), "e": e, "d": hex(dd),
                         "note": "test-only key, generated for this fixture"}
            good.append(kid)
        firsts = {}
        for kid in good:
            k = keys[kid]
            n, dd, bits = int(k["n"], 16), int(k["d"], 16), k["bits"]
            kk = (bits + 7) // 8
            sign = lambda m, **kw: sign_em(em_encode(n, m, kw.pop("salt", None) or rb(32), **kw), n, dd)  # noqa: E731
            msg = rb(270)
            sig = sign(msg)
            firsts[kid] = (sig, msg)
            assert add(kid, sig, msg, "valid") == "VALID"
            m2 = bytearray(msg)
            m2[rng.randrange(len(m2))] ^= 1 << rng.randrange(8)
            add(kid, sig, bytes(m2), "flip message bit")
            s2 = bytearray(sig)
            s2[rng.randrange(1, len(s2))] ^= 1 << rng.randrange(8)
            add(kid, bytes(s2), msg, "flip signature bit")
            add(kid, v15(n, dd, msg), msg, "PKCS#1 v1.5 signature of the same message")
            assert add(kid, b"\x00" + sig, msg, "sig_len = k + 1 with a leading 0x00") == "INVALID"
            for _ in range(20000):  # a valid signature that starts with 0x00, given without that byte
                m3 = rb(40)
                s3 = sign(m3)
                if s3[0] == 0:
                    break
            else:
                raise RuntimeError("no signature with a leading zero byte")
            assert add(kid, s3[1:], m3, "valid signature with its leading 0x00 stripped") == "VALID"
            assert add(kid, s3, m3, "the same signature with its leading 0x00") == "VALID"
            for name, v in (("s = 0", 0), ("s = 1", 1), ("s = n - 1", n - 1), ("s = n", n),
                            ("s = 2^(8k) - 1", (1 << (8 * kk)) - 1)):
                add(kid, v.to_bytes(kk, "big"), msg, name)
            add(kid, sign(msg, trailer=0xCC), msg, "wrong trailer")
            add(kid, sign(msg, pad_byte=3), msg, "nonzero padding byte")
            add(kid, sign(msg, marker=0x00), msg, "missing 0x01")
            add(kid, sign(msg, marker=0x02), msg, "0x02 in place of 0x01")
            add(kid, sign(msg, salt=rb(20)), msg, "20-byte salt")
            if (bits - 1) % 8:  # 8 * block_len > em_bits: a masked bit exists
                for _ in range(4000):
                    m4 = rb(33)
                    em = em_encode(n, m4, rb(32), top_bit=True)
                    if int.from_bytes(em, "big") < n:
                        break
                else:
                    raise RuntimeError("no encoded message with the masked bit set below n")
                exp = add(kid, sign_em(em, n, dd), m4, "top masked bit of EM set, EM < n (BC 1.57: masked; OpenSSL rejects)")
                assert exp == "VALID" and items[-1]["openssl"] == "reject"
            for ln in (1, 55, 56, 64, 700):
                m5 = rb(ln)
                assert add(kid, sign(m5), m5, f"message of {ln} bytes") == "VALID"
            add(kid, b"", msg, "empty signature")
            add(kid, sign(b""), b"", "empty message, valid signature over it")
        for i, kid in enumerate(good):  # another key's valid signature
            sig, msg = firsts[good[(i + 1) % len(good)]]
            add(kid, sig, msg, "a signature made by another key")

        # ---- keys the device decode declines (items keep CG_UNSUPPORTED under the flag)
        def declined(kid, spki, note, src, n=None, dd=None, key_fmt=1):
            keys[kid] = {"spki": spki.hex(), "bits": 0, "accepted": False, "note": note}
            if n is not None:
                msg = rb(100)
                sig = sign_em(em_encode(n, msg, rb(32)), n, dd)
            else:
                sig, msg = firsts[src]
            add(kid, sig, msg, "declined key: " + note, key_fmt)

        for bits in (1016, 4104):
            pub, n, e, dd = gen_key(bits, 65537, d)
            declined(f"rsa{bits}", pub, f"{bits}-bit modulus (outside 1024..4096)", None, n, dd)
        base = keys["rsa2048e3"]
        n, e = int(base["n"], 16), base["e"]
        good_spki = bytes.fromhex(base["spki"])
        declined("even_n", rsa_spki(n - 1, e), "even modulus", "rsa2048e3")
        declined("big_e", rsa_spki(n, (1 << 32) + 1), "e >= 2^32", "rsa2048e3")
        assert good_spki[:2] == b"\x30\x82"
        declined("nonminimal_len", b"\x30\x83\x00" + good_spki[2:], "non-minimal length byte (0x83 0x00 ..)", "rsa2048e3")
        declined("trailing", good_spki + b"\x00", "one trailing byte", "rsa2048e3")
        nb = n.to_bytes(256, "big")
        assert nb[0] & 0x80
        neg = der.spki(RSA_ALG, NULL, der.tlv(0x30, der.tlv(0x02, nb) + der.integer(e)))
        declined("negative_n", neg, "modulus INTEGER without its leading 0x00 (negative)", "rsa2048e3")
        p256 = der.tlv(0x30, der.oid("1.2.840.10045.2.1") + der.oid("1.2.840.10045.3.1.7"))
        declined("p256_oid", der.tlv(0x30, p256 + der.bit_string(der.tlv(0x30, der.integer(n) + der.integer(e)))),
                 "id-ecPublicKey / P-256 AlgorithmIdentifier around RSA bytes", "rsa2048e3")
        ub = bytearray(good_spki)  # SEQUENCE hdr (4) + AlgorithmIdentifier (15), then 03 82 LL LL 00
        assert ub[19] == 0x03 and ub[20] == 0x82 and ub[23] == 0x00
        ub[23] = 0x01
        declined("unused_bits", bytes(ub), "BIT STRING with 1 unused bit", "rsa2048e3")
        declined("fmt_raw", good_spki, "a good key handed over with fmt != SPKI", "rsa2048e3", key_fmt=0)
        declined("garbage", b"\x30" * 300, "300 bytes of 0x30", "rsa2048e3")
        # parameters absent: accepted, as hostverify.rsa_decode_key accepts it
        keys["rsa2048e3_noparams"] = dict(base, spki=rsa_spki(n, e, params=b"").hex(),
                                          note="the 2048-bit key with the AlgorithmIdentifier parameters absent")
        sig, msg = firsts["rsa2048e3"]
        assert add("rsa2048e3_noparams", sig, msg, "valid, parameters absent") == "VALID"

    meta = {"generator": "tests/golden/gen_rsa_gpu.py", "openssl": sh("openssl", "version").decode().strip(),
            "note": "expect = BC 1.57 PSSSigner restatement (hostverify.py), whatever the mode; a DOVERIFY caller "
                    "gets EMPTY for an empty signature or message. openssl = OpenSSL's PSS verdict (n/a: it cannot "
                    "load the key). keys[*].accepted: the device decode's rule (include/cordagpu.h)."}
    with open(os.path.join(HERE, "rsa_gpu.json"), "w") as f:
        json.dump({"meta": meta, "keys": keys, "items": items}, f, indent=0)
    print(len(keys), "keys,", len(items), "items")


if __name__ == "__main__":
    main()
