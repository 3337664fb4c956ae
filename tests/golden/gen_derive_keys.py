"""Generates tests/golden/derive_keys.json: Crypto.deriveKeyPair vectors (Crypto.kt:646-771) for the GPU
key derivation (cg_derive_keys) and its host lane code.

Each record is (parent index, seed index, secret, pub); each parent is (scheme, private key, keyData),
each seed (note, bytes), listed once. The mac is not stored: secret is mac[0..32) for every scheme, and no
record takes a rehash. The expected bytes come from tests/derive_ref.py (hmac, hashlib and the oracles).
One record per line keeps the file small.
Every record's MAC is cross-checked here against the `openssl` binary (dgst -sha512 -mac HMAC), and
every public key against it too: the public half `openssl pkey -pubout` gives for the PKCS#8 (Ed25519)
or SEC1 (ECDSA) encoding of the child private key. The generator asserts that the two sources agree on
every record.

  parents  ECDSA, both curves: d with the top bit set (33-byte keyData with a leading 00), d = 0x80
           (keyData 00 80), d = 1 (1 byte), d below 2^240 (30 bytes); Ed25519: the keys of
           Crypto.deriveEdDSAKeyPairFromEntropy(20 / 70 / 80) and of the RFC 8032 7.1 seeds
  seeds    "seed-1" and "seed-2" (CryptoUtilsTest.kt:665,690); lengths 0, 1, 32, 4096; the inner hash's
           padding boundaries 111, 112, 127, 128, 129, 239, 240; lengths 2 .. 8, so that with 1 every
           byte phase of the last word and of the last 16-byte load occurs
No record takes the retry path: a seed whose mac is refused is a 2^32-try search. The retry path is held
by the library's test hook and the host lane tests (tests/test_derive_host.py).

usage: python tests/golden/gen_derive_keys.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import derive_ref as R  # noqa: E402
from oracle import ecdsa_bc, ed25519_i2p as ed  # noqa: E402

OUT = os.path.join(HERE, "derive_keys.json")
PKCS8_HEAD = bytes.fromhex("302e020100300506032b657004220420")
EC_OID = {R.R1: bytes.fromhex("06082a8648ce3d030107"), R.K1: bytes.fromhex("06052b8104000a")}
RFC_SEEDS = ["9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
             "4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
             "c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7"]
SEED_LENS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 32, 111, 112, 127, 128, 129, 239, 240, 4096]


def stretch(label, n):
    """n deterministic bytes from a label."""
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha256(label.encode() + c.to_bytes(4, "big")).digest()
        c += 1
    return out[:n]


def openssl(args, data=None):
    return subprocess.run(["openssl"] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout


def openssl_hmac(key, msg, tmp):
    path = os.path.join(tmp, "msg")
    with open(path, "wb") as f:
        f.write(msg)
    out = openssl(["dgst", "-sha512", "-mac", "HMAC", "-macopt", "hexkey:" + key.hex(), "-binary", path])
    assert len(out) == 64
    return out


def openssl_public(scheme, secret):
    """The public half OpenSSL computes for the child private key: Abyte, or X || Y."""
    if scheme == R.ED:
        der = openssl(["pkey", "-inform", "DER", "-pubout", "-outform", "DER"], PKCS8_HEAD + secret)
        return der[-32:] + bytes(32)
    body = b"\x02\x01\x01\x04\x20" + secret + b"\xa0" + bytes([len(EC_OID[scheme])]) + EC_OID[scheme]
    der = openssl(["ec", "-inform", "DER", "-pubout", "-outform", "DER", "-conv_form", "uncompressed"],
                  b"\x30" + bytes([len(body)]) + body)
    assert der[-65] == 4
    return der[-64:]


def parents():
    out = []
    for scheme in (R.R1, R.K1):
        n = ecdsa_bc.CURVES[scheme].n
        top = int.from_bytes(stretch("parent top bit", 32), "big") | (1 << 255)
        top &= ~(1 << 254)  # below n on both curves
        low = (int.from_bytes(stretch("parent below 2^240", 30), "big") | (1 << 238)) & ~(1 << 239)
        for note, d in (("d with the top bit set: 33-byte keyData", top), ("d = 0x80: keyData 00 80", 0x80),
                        ("d = 1: 1-byte keyData", 1), ("d below 2^240: 30-byte keyData", low)):
            assert 0 < d < n
            key = R.key_data_ec(d)
            out.append({"scheme": scheme, "note": note, "private": d.to_bytes(32, "big").hex(), "key_data": key.hex()})
    assert [len(bytes.fromhex(p["key_data"])) for p in out[:4]] == [33, 2, 1, 30]
    for e in (20, 70, 80):
        seed = ed.entropy_seed(e)
        out.append({"scheme": R.ED, "note": f"deriveKeyPairFromEntropy({e})", "private": seed.hex(),
                    "key_data": R.key_data_ed(seed).hex()})
    for k, s in enumerate(RFC_SEEDS):
        seed = bytes.fromhex(s)
        out.append({"scheme": R.ED, "note": f"RFC 8032 7.1 TEST {k + 1}", "private": seed.hex(),
                    "key_data": R.key_data_ed(seed).hex()})
    return out


def seeds():
    out = [("seed-1 (CryptoUtilsTest.kt:665)", b"seed-1"), ("seed-2 (CryptoUtilsTest.kt:690)", b"seed-2")]
    out += [(f"{n} bytes", stretch(f"seed {n}", n)) for n in SEED_LENS]
    return out


def main():
    ps, sd, records = parents(), seeds(), []
    with tempfile.TemporaryDirectory() as tmp:
        for pi, p in enumerate(ps):
            key, scheme = bytes.fromhex(p["key_data"]), p["scheme"]
            for si, (note, seed) in enumerate(sd):
                mac = R.mac_of(key, seed)
                assert mac == openssl_hmac(key, seed, tmp), (pi, note)
                secret, pub, tries = R.derive(scheme, key, seed)
                assert tries == 0 and secret == mac[:32]
                assert pub == openssl_public(scheme, secret), (pi, note)
                records.append({"parent": pi, "seed": si, "secret": secret.hex(), "pub": pub.hex()})
    note = ("Crypto.deriveKeyPair vectors: tests/derive_ref.py, every mac and public key cross-checked against "
            "the openssl binary (" + openssl(["version"]).decode().strip() + "); pub is Abyte || 0^32 (Ed25519) "
            "or X || Y big-endian (ECDSA), secret the child seed or d big-endian = mac[0..32)")
    rows = lambda xs: ",\n".join(json.dumps(x) for x in xs)  # noqa: E731
    with open(OUT, "w") as f:
        f.write('{"note": %s,\n"parents": [\n%s\n],\n"seeds": [\n%s\n],\n"records": [\n%s\n]}\n' % (
            json.dumps(note), rows(ps), rows([{"note": n, "hex": s.hex()} for n, s in sd]), rows(records)))
    print(f"{len(ps)} parents, {len(sd)} seeds, {len(records)} records -> {OUT}")


if __name__ == "__main__":
    main()
