"""Host side of Crypto.deriveKeyPair (core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:646-771):
``key_data`` forms the HMAC key the reference's deriveHMAC takes from a private key, and
``derive_ecdsa`` restates deriveKeyPairECDSA for the items the device hands back with
CG_DERIVE_HOST (more than CG_DERIVE_MAX_RETRIES rehashes: about 2^-160 per item on secp256r1). It is
not a fallback for a missing kernel: every other item is derived on the GPU or fails loudly.
"""
import hashlib
import hmac

from .batch import ECDSA_SECP256K1_SHA256, ECDSA_SECP256R1_SHA256, EDDSA_ED25519_SHA512

# (p, a, gx, gy, n) of secp256k1 / secp256r1
_CURVES = {
    ECDSA_SECP256K1_SHA256: (
        2 ** 256 - 2 ** 32 - 977, 0,
        0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
        0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8,
        0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141),
    ECDSA_SECP256R1_SHA256: (
        2 ** 256 - 2 ** 224 + 2 ** 192 + 2 ** 96 - 1, -3,
        0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
        0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5,
        0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551),
}


def key_data(scheme, encoded):
    """deriveHMAC's keyData: a BC EC private key's d.toByteArray() (``encoded`` is the 32-byte
    big-endian d: minimal two's complement, a leading 00 when the top bit of the first magnitude byte is
    set), an EdDSA key's geta() (``encoded`` is the 32-byte seed: the clamped h[0..32) of SHA-512(seed))."""
    encoded = bytes(encoded)
    if scheme == EDDSA_ED25519_SHA512:
        a = bytearray(hashlib.sha512(encoded).digest()[:32])
        a[0] &= 248
        a[31] = (a[31] & 63) | 64
        return bytes(a)
    if scheme in _CURVES:
        d = int.from_bytes(encoded, "big")
        return d.to_bytes((d.bit_length() + 8) // 8, "big")
    raise ValueError(f"scheme {scheme} has no deterministic key derivation")


def accepts(scheme, d):
    """deriveKeyPairECDSA's accept rule: 2 <= d < n and WNafUtil.getNafWeight(d) >= n.bitLength() >>> 2."""
    n = _CURVES[scheme][4]
    return 2 <= d < n and bin((3 * d) ^ d).count("1") >= n.bit_length() >> 2


def _add(p, a, P, Q):
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = (3 * P[0] * P[0] + a) * pow(2 * P[1], -1, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return x, (lam * (P[0] - x) - P[1]) % p


def public_point(scheme, d):
    """d G as (x, y), or None for the point at infinity."""
    p, a, gx, gy, _ = _CURVES[scheme]
    R, Q = None, (gx, gy)
    while d:
        if d & 1:
            R = _add(p, a, R, Q)
        Q = _add(p, a, Q, Q)
        d >>= 1
    return R


def derive_ecdsa(scheme, key, seed, force_retries=0):
    """deriveKeyPairECDSA: (d as 32 big-endian bytes, X || Y, rehashes made). ``force_retries`` refuses
    the first that many attempts, as CG_TEST_DERIVE_FORCE_RETRIES makes the device do."""
    seed, tries = bytes(seed), 0
    while True:
        d = int.from_bytes(hmac.new(bytes(key), seed, hashlib.sha512).digest()[:32], "big")
        if tries >= force_retries and accepts(scheme, d):
            q = public_point(scheme, d)
            if q is not None:
                return d.to_bytes(32, "big"), q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"), tries
        seed = hashlib.sha256(seed).digest()
        tries += 1
