"""Generates tests/golden/rsa_special.json: RSA_SHA256 keys that no key generator makes, chosen so
that valid signatures reach code of the RSA kernels (corda_amd/csrc/verify_rsa.hip, rsa_wave.h)
that ordinary keys leave alone. Pure Python and seeded: a second run reproduces the file byte for
byte (tests/test_rsa_special.py checks the keys and the recorded counts).

Special-form prime moduli, e = 65537, 1024 / 1025 / 2048 / 2049 / 4096 bits, n = 2^B - c and
n = 2^(B-1) + c with the smallest c that makes n prime with gcd(e, n - 1) = 1. R mod n is then a
small number (or close to a power of two), every value the key preparation squares is a sparse
multiple of a power of two, and the products have long runs of zero limbs: each run is a generate
followed by a chain of propagating lanes in rsa_resolve. A prime modulus can be signed for with
d = e^-1 mod (n - 1), and a valid signature verifies only if R^2 mod n came out right, so these
items witness the carry ripple inside k_rsa_keyprep. meta.keyprep records, per key, what the lane
model (tests/rsa_wave_model.py) counts over the key preparation.

Exponent-shape keys, 2048 bits: e = 1 (any odd n above EM: the signature is EM), e = 2, 4, 6 (s chosen,
n = s^e - EM retried until odd with exactly 2048 bits; n need not be prime), and prime n for
e = 0x80000001, 0xffffffff, 0x10001: the branches of the exponent ladder (no product, the final
product with one, a set bit in the middle, every bit set).

Per key: a valid signature, the same with one signature bit flipped, the same with one message bit
flipped, s = n - 1; the special-form keys add 8 valid signatures over messages of other lengths.
`expect` is hostverify.rsa_verify's verdict. Layout as rsa_gpu.json: the keys stored once.

usage: python tests/golden/gen_rsa_special.py
"""
import json
import math
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import rsa_wave_model  # noqa: E402
from corda_amd import der, hostverify  # noqa: E402

RSA_ALG = der.oid("1.2.840.113549.1.1.1")
NULL = der.tlv(0x05, b"")
SPECIAL_BITS = (1024, 1025, 2048, 2049, 4096)
MSG_LENGTHS = (1, 31, 55, 56, 64, 119, 300, 700)


def _small_primes(limit):
    sieve = bytearray([1]) * limit
    sieve[0:2] = b"\x00\x00"
    for i in range(2, int(limit ** 0.5) + 1):
        if sieve[i]:
            sieve[i * i::i] = bytearray(len(sieve[i * i::i]))
    return [i for i in range(limit) if sieve[i]]


SMALL = _small_primes(20000)


def is_prime(n):
    """Trial division, then Miller-Rabin to the first 16 primes as bases."""
    for p in SMALL:
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in SMALL[:16]:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def special_prime(bits, form, e):
    """(n, c): the smallest c with n prime and gcd(e, n - 1) = 1."""
    c = 1
    while True:
        n = (1 << bits) - c if form == "2^B-c" else (1 << (bits - 1)) + c
        if math.gcd(e, n - 1) == 1 and is_prime(n):
            assert n.bit_length() == bits
            return n, c
        c += 2


def random_prime(bits, e, rng):
    while True:
        n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if math.gcd(e, n - 1) == 1 and is_prime(n):
            return n


def iroot(x, k):
    """floor(x^(1/k))"""
    lo, hi = 0, 1 << (x.bit_length() // k + 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** k <= x:
            lo = mid
        else:
            hi = mid - 1
    return lo


def rsa_spki(n, e):
    return der.spki(RSA_ALG, NULL, der.tlv(0x30, der.integer(n) + der.integer(e)))


def main():
    rng = random.Random(0x5BEC1A1)
    rb = lambda ln: bytes(rng.randrange(256) for _ in range(ln))  # noqa: E731
    keys, items, keyprep = {}, [], {}

    def add_key(kid, n, e, note, d=None, **more):
        spki = rsa_spki(n, e)
        assert hostverify.rsa_decode_key(spki) == (n, e)
        keys[kid] = dict({"spki": spki.hex(), "bits": n.bit_length(), "accepted": True, "n": hex(n), "e": e,
                          "note": note}, **more)
        if d is not None:
            keys[kid]["d"] = hex(d)

    def add(kid, sig, msg, note):
        k = keys[kid]
        ok = hostverify.rsa_verify((int(k["n"], 16), k["e"]), sig, msg)
        items.append({"key": kid, "key_fmt": 1, "sig": sig.hex(), "msg": msg.hex(), "note": note,
                      "expect": "VALID" if ok else "INVALID"})
        return ok

    def four(kid, sig, msg):
        n = int(keys[kid]["n"], 16)
        assert add(kid, sig, msg, "valid"), kid
        s2 = bytearray(sig)
        s2[rng.randrange(1, len(s2))] ^= 1 << rng.randrange(8)
        add(kid, bytes(s2), msg, "flip signature bit")
        m2 = bytearray(msg)
        m2[rng.randrange(len(m2))] ^= 1 << rng.randrange(8)
        add(kid, sig, bytes(m2), "flip message bit")
        add(kid, (n - 1).to_bytes((n.bit_length() + 7) // 8, "big"), msg, "s = n - 1")

    # ---- special-form prime moduli
    for bits in SPECIAL_BITS:
        for form, tag in (("2^B-c", "m"), ("2^(B-1)+c", "p")):
            e = 65537
            n, c = special_prime(bits, form, e)
            d = pow(e, -1, n - 1)
            kid = f"{tag}{bits}"
            add_key(kid, n, e, f"prime n = {form}, B = {bits}, c = {c}; test-only, d = e^-1 mod (n - 1)", d, form=form, c=c)
            rr, ev = rsa_wave_model.keyprep(n)
            assert rr == pow(2, 64 * ((bits + 31) // 32), n)
            row = ev.row(0)
            keyprep[kid] = {"gen": row["gen"], "cprop": row["cprop"], "chain": row["chain"]}
            msg = rb(270)
            four(kid, hostverify.rsa_pss_sign(n, d, msg, rb(32)), msg)
            for ln in MSG_LENGTHS:
                m = rb(ln)
                assert add(kid, hostverify.rsa_pss_sign(n, d, m, rb(32)), m, f"valid, message of {ln} bytes")

    # ---- exponent shapes at 2048 bits
    bits = 2048
    n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    add_key("e1", n, 1, "e = 1: the signature is the encoded message itself; any odd n above it")
    msg = rb(270)
    four("e1", hostverify.rsa_pss_sign(n, 1, msg, rb(32)), msg)
    for e in (2, 4, 6):
        msg, salt = rb(270), rb(32)
        em = int.from_bytes(hostverify.rsa_pss_sign((1 << bits) - 1, 1, msg, salt), "big")  # EM for a 2048-bit n
        lo, hi = iroot((1 << (bits - 1)) + em, e) + 1, iroot((1 << bits) - 1 + em, e)
        while True:
            s = rng.randrange(lo, hi + 1)
            n = s ** e - em
            if n % 2 == 1 and n.bit_length() == bits and s < n:
                break
        assert pow(s, e, n) == em
        add_key(f"e{e}", n, e, f"e = {e}: n = s^e - EM for a chosen s (n need not be prime)")
        four(f"e{e}", s.to_bytes(bits // 8, "big"), msg)
    for e in (0x80000001, 0xFFFFFFFF, 0x10001):
        n = random_prime(bits, e, rng)
        d = pow(e, -1, n - 1)
        add_key(f"e{e:x}", n, e, f"e = {e:#x}, prime n; test-only, d = e^-1 mod (n - 1)", d)
        msg = rb(270)
        four(f"e{e:x}", hostverify.rsa_pss_sign(n, d, msg, rb(32)), msg)

    for kid in keys:
        assert any(i["key"] == kid and i["expect"] == "VALID" for i in items), kid
    meta = {"generator": "tests/golden/gen_rsa_special.py",
            "note": "expect = BC 1.57 PSSSigner restatement (hostverify.py). keyprep: per special-form key, what "
                    "tests/rsa_wave_model.py counts over the wave form of the key preparation, in lanes below L: "
                    "generating lanes, propagating lanes that receive a carry, the longest chain of those.",
            "keyprep": keyprep}
    with open(os.path.join(HERE, "rsa_special.json"), "w") as f:
        json.dump({"meta": meta, "keys": keys, "items": items}, f, indent=0)
    print(len(keys), "keys,", len(items), "items")
    for kid, row in keyprep.items():
        print(kid, row)


if __name__ == "__main__":
    main()
