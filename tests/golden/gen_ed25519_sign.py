"""Generates tests/golden/ed25519_sign.json: Ed25519 signing vectors for the GPU signer
(cg_sign_batch / cg_sign_tx_ids) and its host lane code.

Each record is (seed, pub = Abyte, message or (prefix, id, suffix), sig, status) with a note. The
signatures come from oracle.ed25519_i2p.sign (RFC 8032's deterministic signature, what i2p 0.2.0
EdDSAEngine.engineSign computes) and every one is cross-checked here against OpenSSL
(`pkeyutl -sign -rawin` over a PKCS#8 DER of 302e020100300506032b657004220420 || seed); the RFC 8032
section 7.1 vectors are checked against the RFC's own bytes as well. The generator asserts that the
sources agree on all of them.

  RFC 8032 7.1   TEST 2 and 3; TEST 1 (the empty message) as the CG_EMPTY case: status EMPTY, 64 zero
                 bytes; TEST 1's seed with a 1-byte message
  entropy keys   Crypto.deriveEdDSAKeyPairFromEntropy(n), n = 20 (DUMMY_NOTARY_KEY), 70, 80
  messages       the lengths where 32 + len or 64 + len crosses a SHA-512 padding boundary
                 ((n + 17 + 127) >> 7), odd ones covering every byte phase of the last word, and 4096
  splices        the real SignableData template (prefix 234, suffix 3), and prefix lengths 0, 1, 2, 3, 45,
                 81, 233 with suffix lengths 0 and 3: the id straddles a 128-byte block in one hash or
                 the other, at every alignment mod 4

usage: python tests/golden/gen_ed25519_sign.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from corda_amd import signable  # noqa: E402
from oracle import ed25519_i2p as ed  # noqa: E402

OUT = os.path.join(HERE, "ed25519_sign.json")
PKCS8_HEAD = bytes.fromhex("302e020100300506032b657004220420")
MSG_LENS = [1, 47, 48, 79, 80, 111, 112, 127, 128, 129, 175, 176, 207, 208, 303, 304, 335, 336, 4096]
PREFIX_LENS = [0, 1, 2, 3, 45, 81, 233]
SUFFIX_LENS = [0, 3]
ENTROPY = [20, 70, 80]
EMPTY = 5  # CG_EMPTY (include/cordagpu.h)

RFC = [  # (name, seed, pub, msg, sig)
    ("TEST 1", "9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
     "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a", "",
     "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46b"
     "d25bf5f0595bbe24655141438e7a100b"),
    ("TEST 2", "4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
     "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c", "72",
     "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da085ac1e43e15996e458f3613d0f11d8c"
     "387b2eaeb4302aeeb00d291612bb0c00"),
    ("TEST 3", "c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7",
     "fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025", "af82",
     "6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac18ff9b538d16f290ae67f760984dc659"
     "4a7c15e9716ed28dc027beceea1ec40a"),
]


def stretch(label, n):
    """n deterministic bytes from a label."""
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha512(label.encode() + c.to_bytes(4, "little")).digest()
        c += 1
    return out[:n]


def openssl_sign(tmp, seed, msg):
    key, m, sig = (os.path.join(tmp, f) for f in ("key.der", "msg.bin", "sig.bin"))
    with open(key, "wb") as f:
        f.write(PKCS8_HEAD + seed)
    with open(m, "wb") as f:
        f.write(msg)
    subprocess.check_call(["openssl", "pkeyutl", "-sign", "-rawin", "-inkey", key, "-keyform", "DER", "-in", m,
                           "-out", sig])
    with open(sig, "rb") as f:
        return f.read()


def main():
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        def signed(seed, msg):
            sig = ed.sign(seed, msg)
            assert openssl_sign(tmp, seed, msg) == sig, "OpenSSL and the Python oracle disagree"
            assert ed.verify(ed.PublicKey(ed.public_from_seed(seed)), msg, sig)
            return sig

        def msg_rec(note, seed, msg):
            recs.append({"note": note, "seed": seed.hex(), "pub": ed.public_from_seed(seed).hex(), "msg": msg.hex(),
                         "sig": signed(seed, msg).hex(), "status": 0})

        def tmpl_rec(note, seed, prefix, tx_id, suffix):
            recs.append({"note": note, "seed": seed.hex(), "pub": ed.public_from_seed(seed).hex(),
                         "prefix": prefix.hex(), "id": tx_id.hex(), "suffix": suffix.hex(),
                         "sig": signed(seed, prefix + tx_id + suffix).hex(), "status": 0})

        for name, seed, pub, msg, sig in RFC:
            seed, msg = bytes.fromhex(seed), bytes.fromhex(msg)
            assert ed.public_from_seed(seed).hex() == pub and ed.sign(seed, msg).hex() == sig, name
            if msg:
                msg_rec(f"RFC 8032 7.1 {name}", seed, msg)
                assert recs[-1]["sig"] == sig
            else:  # Crypto.kt:398: "Signing of an empty array is not permitted!"
                recs.append({"note": f"RFC 8032 7.1 {name}: the empty message, CG_EMPTY", "seed": seed.hex(), "pub": pub,
                             "msg": "", "sig": "00" * 64, "status": EMPTY})
        msg_rec("RFC 8032 7.1 TEST 1's seed, 1-byte message", bytes.fromhex(RFC[0][1]), b"\x5a")

        seeds = [(n, ed.entropy_seed(n)) for n in ENTROPY]
        for ln in MSG_LENS:
            for n, seed in seeds:
                msg_rec(f"entropy {n}, {ln}-byte message", seed, stretch(f"msg {n} {ln}", ln))
        pre, suf = signable.template(1, 4)
        assert (len(pre), len(suf)) == (234, 3)
        for n, seed in seeds:
            for j in range(4):
                tmpl_rec(f"entropy {n}, SignableData(id {j}, SignatureMetadata(1, 4))", seed, pre,
                         stretch(f"id {n} {j}", 32), suf)
        for pl in PREFIX_LENS:
            for sl in SUFFIX_LENS:
                for n, seed in seeds:
                    for j in range(3):
                        tmpl_rec(f"entropy {n}, prefix {pl} suffix {sl}, id {j}", seed, stretch(f"pre {pl} {sl}", pl),
                                 stretch(f"id {n} {pl} {sl} {j}", 32), stretch(f"suf {pl} {sl}", sl))
    with open(OUT, "w") as f:
        json.dump({"records": recs}, f, indent=0)
        f.write("\n")
    print(f"{len(recs)} records, {os.path.getsize(OUT)} bytes -> {OUT}")


if __name__ == "__main__":
    main()
