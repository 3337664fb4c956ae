"""Generates tests/golden/rsa_sign.json: RSA_SHA256 (SHA256WITHRSAANDMGF1) signing fixtures for the GPU signer
(corda_amd/csrc/sign_rsa.hip, rsa_sign_wave.h, rsa.h). Fresh test-only keys with all CRT parts come from
the OpenSSL CLI at the bit lengths where the kernels take another path: 1024 (the minimum), 1025 (unequal
prime lengths, block_len = k - 1), 1032 (no multiple of 32), 2048 with e = 3, 2048, 3072 and 4096 (the
maximum); and copies of the 1024- and 3072-bit keys with p and q exchanged and dP, dQ, qInv recomputed,
so that both orders of the primes (p > q and p < q) are signed with whatever order OpenSSL wrote.

Each record is (key, message, salt) -> `em` (the encoded message) and `sig`, computed with
hostverify.rsa_pss_sign's arithmetic (Python integers). Messages have 1, 55, 56, 64, 270 and 700 bytes;
salts are random, all zero and all 0xFF. Every record is accepted by `openssl dgst -verify` with PSS, salt
length 32 and MGF1-SHA256, and by hostverify.rsa_verify, when it is generated.

`refused`: keys the load must refuse (dP + 2, n + 2, an even p, a 1016-bit n, e = 0), and `pkcs8_big_e`, a
PKCS#8 private key whose public exponent is 2^32 + 1 (the Python mirror's refusal; the C ABI's e is 32 bits).

Layout: {"keys": {id: {pkcs8, spki, bits, n, e, d, p, q, dp, dq, qinv}}, "records": [{key, msg, salt, em,
sig}], "refused": [{id, status, n, e, p, q, dp, dq, qinv}], "pkcs8_big_e": hex}. Numbers are hex strings.

usage: python tests/golden/gen_rsa_sign.py  (needs the openssl CLI)
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
from corda_amd import hostverify  # noqa: E402

PSS = ["-sigopt", "rsa_padding_mode:pss", "-sigopt", "rsa_pss_saltlen:32", "-sigopt", "rsa_mgf1_md:sha256"]
KEY_INVALID, UNSUPPORTED = 3, 4  # CG_KEY_INVALID, CG_UNSUPPORTED (include/cordagpu.h)
PARTS = ("n", "e", "d", "p", "q", "dp", "dq", "qinv")


def sh(*args):
    return subprocess.run(args, capture_output=True, check=True).stdout


def ossl_accepts(pub_der, msg, sig, d):
    kp, mp, sp = (os.path.join(d, n) for n in ("pub.der", "m.bin", "s.bin"))
    for path, data in ((kp, pub_der), (mp, msg), (sp, sig)):
        with open(path, "wb") as f:
            f.write(data)
    r = subprocess.run(["openssl", "dgst", "-sha256", "-keyform", "DER", "-verify", kp] + PSS + ["-signature", sp, mp],
                       capture_output=True)
    return r.returncode == 0


def gen_key(bits, e, d):
    """(pkcs8, spki, parts) of a fresh key whose modulus has exactly `bits` bits."""
    for _ in range(64):
        key = os.path.join(d, "k.pem")
        sh("openssl", "genpkey", "-algorithm", "RSA", "-pkeyopt", f"rsa_keygen_bits:{bits}", "-pkeyopt",
           f"rsa_keygen_pubexp:{e}", "-out", key)
        pkcs8 = sh("openssl", "pkcs8", "-topk8", "-nocrypt", "-in", key, "-outform", "DER")
        spki = sh("openssl", "pkey", "-in", key, "-pubout", "-outform", "DER")
        k = hostverify.rsa_decode_private_key(pkcs8)
        if k["n"].bit_length() == bits:
            assert k["p"] * k["q"] == k["n"] and k["e"] == e and k["qinv"] * k["q"] % k["p"] == 1
            return pkcs8, spki, k
    raise RuntimeError(f"no {bits}-bit modulus from openssl")


def swapped(k):
    p, q = k["q"], k["p"]
    return dict(k, p=p, q=q, dp=k["d"] % (p - 1), dq=k["d"] % (q - 1), qinv=pow(q, -1, p))


def em_encode(n, msg, salt):
    em_bits = n.bit_length() - 1
    block_len = (em_bits + 7) // 8
    mh = hashlib.sha256(bytes(8) + hashlib.sha256(msg).digest() + salt).digest()
    db = bytes(block_len - 32 - 32 - 2) + b"\x01" + salt
    masked = bytearray(a ^ b for a, b in zip(db, hostverify.mgf1_sha256(mh, len(db))))
    masked[0] &= 0xFF >> (8 * block_len - em_bits)
    return bytes(masked) + mh + b"\xbc"


def main():
    rng = random.Random(0x516E)
    rb = lambda ln: bytes(rng.randrange(256) for _ in range(ln))  # noqa: E731
    keys, records, refused = {}, [], []
    with tempfile.TemporaryDirectory() as d:
        for bits, e in ((1024, 65537), (1025, 65537), (1032, 65537), (2048, 3), (2048, 65537), (3072, 65537),
                        (4096, 65537)):
            pkcs8, spki, k = gen_key(bits, e, d)
            kid = f"rsa{bits}" + ("e3" if e == 3 else "")
            keys[kid] = dict({"pkcs8": pkcs8.hex(), "spki": spki.hex(), "bits": bits}, **{f: hex(k[f]) for f in PARTS})
        for kid in ("rsa1024", "rsa3072"):
            k = swapped({f: int(keys[kid][f], 16) for f in PARTS})
            keys[kid + "_swapped"] = dict(keys[kid], **{f: hex(k[f]) for f in PARTS})
        assert int(keys["rsa1025"]["p"], 16).bit_length() != int(keys["rsa1025"]["q"], 16).bit_length()
        for ki, (kid, k) in enumerate(keys.items()):
            n, dd = int(k["n"], 16), int(k["d"], 16)
            for mi, ln in enumerate((1, 55, 56, 64, 270, 700)):
                msg = rb(ln)
                salt = (rb(32), bytes(32), b"\xff" * 32)[(ki + mi) % 3]
                em = em_encode(n, msg, salt)
                sig = hostverify.rsa_pss_sign(n, dd, msg, salt)
                assert sig == pow(int.from_bytes(em, "big"), dd, n).to_bytes((n.bit_length() + 7) // 8, "big")
                assert hostverify.rsa_verify((n, int(k["e"], 16)), sig, msg)
                assert ossl_accepts(bytes.fromhex(k["spki"]), msg, sig, d)
                records.append({"key": kid, "msg": msg.hex(), "salt": salt.hex(), "em": em.hex(), "sig": sig.hex()})

        base = {f: int(keys["rsa2048"][f], 16) for f in PARTS}

        def refuse(rid, status, **change):
            k = dict(base, **change)
            refused.append(dict({"id": rid, "status": status}, **{f: hex(k[f]) for f in PARTS if f != "d"}))

        refuse("dp_plus_2", KEY_INVALID, dp=base["dp"] + 2)          # the self-test
        refuse("n_plus_2", KEY_INVALID, n=base["n"] + 2)             # p q != n: the self-test
        refuse("even_p", KEY_INVALID, p=base["p"] + 1)
        refuse("e_zero", KEY_INVALID, e=0)
        _, _, small = gen_key(1016, 65537, d)
        refused.append(dict({"id": "n_1016_bits", "status": UNSUPPORTED}, **{f: hex(small[f]) for f in PARTS if f != "d"}))
        big_e, _, kb = gen_key(2048, (1 << 32) + 1, d)
        assert kb["e"] == (1 << 32) + 1

    meta = {"generator": "tests/golden/gen_rsa_sign.py", "openssl": sh("openssl", "version").decode().strip(),
            "note": "test-only keys, generated for this fixture. sig = EM^d mod n as k bytes; every record was accepted "
                    "by `openssl dgst -verify` (PSS, salt length 32, MGF1-SHA256) and hostverify.rsa_verify."}
    with open(os.path.join(HERE, "rsa_sign.json"), "w") as f:
        json.dump({"meta": meta, "keys": keys, "records": records, "refused": refused, "pkcs8_big_e": big_e.hex()}, f,
                  indent=0)
    print(len(keys), "keys,", len(records), "records,", len(refused), "refused")


if __name__ == "__main__":
    main()
