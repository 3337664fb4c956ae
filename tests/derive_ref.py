"""Python restatement of Crypto.deriveKeyPair (core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:
646-771), the yardstick of the key-derivation tests. Built from hmac, hashlib and the oracles only
(oracle.ecdsa_bc.public_point / ec_mul, oracle.ed25519_i2p.secret_expand / public_from_seed); nothing of
corda_amd is used.

  deriveHMAC           mac = HMAC-SHA512(key = keyData, msg = seed); keyData is d.toByteArray() of a BC EC
                       private key, geta() of an EdDSA key (key_data_ec / key_data_ed)
  deriveKeyPairEdDSA   child seed = mac[0..32), public = encode(a B)
  deriveKeyPairECDSA   d = BigInteger(1, mac[0..32)); refused when d < 2, getNafWeight(d) <
                       n.bitLength() >>> 2, d >= n or d G is infinity; a refusal derives again with
                       seed := SHA-256(seed)
``force_retries=k`` refuses the first k ECDSA attempts whatever their d (the library's test hook
CG_TEST_DERIVE_FORCE_RETRIES does the same on the device). ``derive`` reports the number of rehashes.
"""
import hashlib
import hmac
import json
import os

from oracle import ecdsa_bc, ed25519_i2p

K1, R1, ED = 2, 3, 4  # Corda schemeNumberIDs
MAX_RETRIES = 4       # CG_DERIVE_MAX_RETRIES
# status bytes (include/cordagpu.h)
OK, UNSUPPORTED, DERIVE_HOST, BAD_PARENT, KEY_REJECTED, NOT_RUN = 0, 4, 6, 7, 8, 255


def key_data_ec(d):
    """BigInteger.toByteArray(): minimal two's complement, big-endian."""
    return d.to_bytes((d.bit_length() + 8) // 8, "big")


def key_data_ed(seed):
    """EdDSAPrivateKey.geta(): the clamped h[0..32) of SHA-512(seed)."""
    a, _ = ed25519_i2p.secret_expand(seed)
    return a.to_bytes(32, "little")


def mac_of(key, seed):
    return hmac.new(key, seed, hashlib.sha512).digest()


def naf_weight(d):
    """WNafUtil.getNafWeight: bitCount(3d xor d)."""
    return 0 if d == 0 else bin((3 * d) ^ d).count("1")


def accepts(scheme, d):
    n = ecdsa_bc.CURVES[scheme].n
    return not (d < 2 or naf_weight(d) < (n.bit_length() >> 2) or d >= n)


def ec_public(scheme, d):
    """X || Y big-endian of d G, or None at infinity."""
    q = ecdsa_bc.public_point(scheme, d)
    return None if q is None else q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")


def derive(scheme, key, seed, force_retries=0):
    """(secret 32 bytes, public 64 bytes, rehashes). Ed25519: the child seed, Abyte then 32 zero bytes;
    ECDSA: d and X || Y big-endian."""
    if scheme == ED:
        child = mac_of(key, seed)[:32]
        return child, ed25519_i2p.public_from_seed(child) + bytes(32), 0
    assert scheme in (K1, R1)
    tries = 0
    while True:
        d = int.from_bytes(mac_of(key, seed)[:32], "big")
        if tries >= force_retries and accepts(scheme, d):
            pub = ec_public(scheme, d)
            if pub is not None:
                return d.to_bytes(32, "big"), pub, tries
        seed = hashlib.sha256(seed).digest()
        tries += 1


def device_expect(scheme, key, seed, force_retries=0):
    """What cg_derive_keys writes for a well-formed request: (status, secret, public, rehashes). More
    than MAX_RETRIES rehashes: CG_DERIVE_HOST, zero bytes, MAX_RETRIES rehashes made."""
    secret, pub, tries = derive(scheme, key, seed, force_retries)
    if tries > MAX_RETRIES:
        return DERIVE_HOST, bytes(32), bytes(64), MAX_RETRIES
    return OK, secret, pub, tries


def public_key(scheme, secret):
    """cg_public_keys: (status, public 64 bytes)."""
    if scheme == ED:
        return OK, ed25519_i2p.public_from_seed(secret) + bytes(32)
    d = int.from_bytes(secret, "big")
    if not accepts(scheme, d):
        return KEY_REJECTED, bytes(64)
    return OK, ec_public(scheme, d)


def load_fixture():
    """tests/golden/derive_keys.json with every record's seed (hex), note, mac and retries (0) filled in."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derive_keys.json")) as f:
        doc = json.load(f)
    for r in doc["records"]:
        s = doc["seeds"][r["seed"]]
        key = bytes.fromhex(doc["parents"][r["parent"]]["key_data"])
        r.update(seed=s["hex"], note=s["note"], mac=mac_of(key, bytes.fromhex(s["hex"])).hex(), retries=0)
        assert r["mac"][:64] == r["secret"]
    return doc
