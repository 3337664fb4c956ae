"""Generates tests/golden/ecdsa_sign.json: ECDSA signing vectors (BC 1.57 SHA256withECDSA with the nonce
given: DSABase.engineSign -> ECDSASigner.generateSignature -> StdDSAEncoder.encode) for the GPU signer
(cg_ec_sign_batch / cg_ec_sign_tx_ids) and its host lane code.

The signatures come from oracle.ecdsa_bc.sign + der_encode_sig. Every signed record is verified here by
the `openssl` binary (dgst -sha256 -verify over the key's SubjectPublicKeyInfo DER) and by
oracle.ecdsa_bc.verify; the generator asserts both.

Layout: "keys" (per scheme: d, X || Y), "records" (one per line; d is the scheme's key unless the record
carries its own; "msg" for Crypto.doSign(privateKey, clearData), "prefix"/"id"/"suffix" for the
SignableData splice; "k" the 32-byte candidate; "status" and "sig", the DER bytes, empty when the item is
not signed), and "edges" (per scheme: [k, digest] over the one message "edge_msg", k in hex without
leading zeros, digest = the first 12 bytes of SHA-256(sig): the G-table edge scalars are many; a test
compares digests, and shows the oracle's full bytes for an edge whose digest differs).

Per curve:
  messages   lengths 1 .. 5 (every byte phase of the last word), and the SHA-256 padding boundaries
             55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129
  splices    the real SignableData template (prefix 234, suffix 3); prefix lengths 0, 1, 2, 3, 45, 81, 233
             (suffix 3): the id straddles a 64-byte block at every alignment mod 4
  crafted k  1, 2, n - 2, n - 1
  edges      tests/scalar_edges.py ec_u1_targets at radix 2^26, 2^24 and 2^22, as k
  refused k  0, n, n + 1, 2^256 - 1: CG_NONCE_REJECTED
  s = 0      d = -e r^-1 mod n for a chosen message and k: CG_NONCE_REJECTED
  DER        r and s with the top bit set (33-byte INTEGER) and clear, and one r and one s of at most 31
             bytes (a short search over k, and over a message counter)
  empty      the empty message: CG_EMPTY

usage: python tests/golden/gen_ecdsa_sign.py
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
import scalar_edges  # noqa: E402
from corda_amd import signable  # noqa: E402
from oracle import ecdsa_bc as bc  # noqa: E402

OUT = os.path.join(HERE, "ecdsa_sign.json")
SCHEMES = (2, 3)
MSG_LENS = [1, 2, 3, 4, 5, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129]
PREFIX_LENS = [0, 1, 2, 3, 45, 81, 233]
EMPTY, NONCE_REJECTED = 5, 9  # CG_EMPTY, CG_NONCE_REJECTED (include/cordagpu.h)
EDGE_MSG = b"G-table edge scalars"


def stretch(label, n):
    """n deterministic bytes from a label."""
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha256(label.encode() + c.to_bytes(4, "big")).digest()
        c += 1
    return out[:n]


def key_of(scheme):
    d = int.from_bytes(stretch(f"ecdsa sign key {scheme}", 32), "big") % (bc.CURVES[scheme].n - 1) + 1
    return d


def openssl_verify(tmp, scheme, Q, msg, sig):
    pub, m, s = (os.path.join(tmp, f) for f in ("pub.der", "msg.bin", "sig.bin"))
    with open(pub, "wb") as f:
        f.write(bc.spki_prefix(scheme, 65) + b"\x04" + bc.raw_key(Q))
    with open(m, "wb") as f:
        f.write(msg)
    with open(s, "wb") as f:
        f.write(sig)
    r = subprocess.run(["openssl", "dgst", "-sha256", "-verify", pub, "-keyform", "DER", "-signature", s, m],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return r.returncode == 0 and b"Verified OK" in r.stdout


def int_len(v):
    return len(bc.der_encode_int(v)) - 2


def main():
    keys, recs, edges, shapes = {}, [], {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        def signed(scheme, d, msg, k):
            r, s = bc.sign(scheme, d, msg, k)
            sig = bc.der_encode_sig(r, s)
            Q = bc.public_point(scheme, d)
            assert bc.verify(scheme, Q, msg, sig) and openssl_verify(tmp, scheme, Q, msg, sig), (scheme, k)
            assert 8 <= len(sig) <= 72
            shapes.setdefault(scheme, set()).update({("r", int_len(r)), ("s", int_len(s))})
            return sig

        for scheme in SCHEMES:
            c = bc.CURVES[scheme]
            n, d = c.n, key_of(scheme)
            keys[str(scheme)] = {"d": d.to_bytes(32, "big").hex(), "pub": bc.raw_key(bc.public_point(scheme, d)).hex()}

            def nonce(label):
                return int.from_bytes(stretch(f"k {scheme} {label}", 32), "big") % (n - 1) + 1

            def rec(note, k, status=0, sig=b"", d_own=None, **where):
                r = {"scheme": scheme, "note": note}
                if d_own is not None:
                    r["d"] = d_own.to_bytes(32, "big").hex()
                r.update({a: b.hex() for a, b in where.items()})
                r.update({"k": k.to_bytes(32, "big").hex(), "status": status, "sig": sig.hex()})
                recs.append(r)

            for ln in MSG_LENS:
                msg, k = stretch(f"msg {scheme} {ln}", ln), nonce(f"msg {ln}")
                rec(f"{ln}-byte message", k, sig=signed(scheme, d, msg, k), msg=msg)
            pre, suf = signable.template(1, scheme)
            assert (len(pre), len(suf)) == (234, 3)
            for j in range(3):
                tx, k = stretch(f"id {scheme} {j}", 32), nonce(f"tx {j}")
                rec(f"SignableData(id {j}, SignatureMetadata(1, {scheme}))", k, sig=signed(scheme, d, pre + tx + suf, k),
                    prefix=pre, id=tx, suffix=suf)
            for pl in PREFIX_LENS:
                p, sx, tx, k = stretch(f"pre {pl}", pl), stretch(f"suf {pl}", 3), stretch(f"id {scheme} {pl}", 32), nonce(f"pl {pl}")
                rec(f"prefix {pl} suffix 3", k, sig=signed(scheme, d, p + tx + sx, k), prefix=p, id=tx, suffix=sx)
            msg = stretch(f"crafted {scheme}", 40)
            for note, k in (("k = 1", 1), ("k = 2", 2), ("k = n - 2", n - 2), ("k = n - 1", n - 1)):
                rec(note, k, sig=signed(scheme, d, msg, k), msg=msg)
            for note, k in (("k = 0", 0), ("k = n", n), ("k = n + 1", n + 1), ("k = 2^256 - 1", 2 ** 256 - 1)):
                rec(note + ": refused", k, status=NONCE_REJECTED, msg=msg)
            # s = 0: d = -e r^-1 mod n
            k = nonce("s = 0")
            e = int.from_bytes(hashlib.sha256(msg).digest(), "big")
            r0 = bc.ec_mul(c, k, c.G)[0] % n
            d0 = (-e * pow(r0, n - 2, n)) % n
            assert 0 < d0 < n and (e + r0 * d0) % n == 0
            rec("s = 0 (d = -e / r): refused", k, status=NONCE_REJECTED, d_own=d0, msg=msg)
            # a short r: walk k = 1, 2, ... by additions
            R, k = c.G, 1
            while (R[0] % n).bit_length() > 247:
                R, k = bc.ec_add(c, R, c.G), k + 1
            rec(f"r of {int_len(R[0] % n)} bytes", k, sig=signed(scheme, d, msg, k), msg=msg)
            # a short s: a message counter under one k
            k = nonce("short s")
            rk, kinv, ctr = bc.ec_mul(c, k, c.G)[0] % n, pow(k, n - 2, n), 0
            while True:
                m2 = b"short s %d" % ctr
                s = kinv * (int.from_bytes(hashlib.sha256(m2).digest(), "big") + rk * d) % n
                if 0 < s.bit_length() <= 247:
                    break
                ctr += 1
            rec(f"s of {int_len(s)} bytes", k, sig=signed(scheme, d, m2, k), msg=m2)
            rec("the empty message: CG_EMPTY", nonce("empty"), status=EMPTY, msg=b"")
            got = shapes[scheme]
            assert {("r", 33), ("s", 33), ("r", 32), ("s", 32)} <= got, got
            assert any(a == "r" and ln <= 31 for a, ln in got) and any(a == "s" and ln <= 31 for a, ln in got)
            # the G table's edges, as k
            seen, rows = set(), []
            for w in scalar_edges.WIDE_RADIXES:
                for _, k in scalar_edges.ec_u1_targets(scheme, w):
                    if k in seen:
                        continue
                    seen.add(k)
                    rows.append(["%x" % k, hashlib.sha256(signed(scheme, d, EDGE_MSG, k)).digest()[:12].hex()])
            edges[str(scheme)] = rows
    note = ("ECDSA signing vectors (BC 1.57 SHA256withECDSA, k given): oracle.ecdsa_bc.sign + der_encode_sig, every "
            "signed record verified by oracle.ecdsa_bc.verify and by the openssl binary ("
            + subprocess.run(["openssl", "version"], stdout=subprocess.PIPE).stdout.decode().strip() + ")")
    rows = lambda xs: ",\n".join(json.dumps(x, separators=(",", ":")) for x in xs)  # noqa: E731
    with open(OUT, "w") as f:
        f.write('{"note": %s,\n"keys": %s,\n"edge_msg": %s,\n"records": [\n%s\n],\n"edges": {\n%s\n}}\n' % (
            json.dumps(note), json.dumps(keys), json.dumps(EDGE_MSG.hex()), rows(recs),
            ",\n".join('"%s": [\n%s\n]' % (s, rows(edges[s])) for s in edges)))
    print(f"{len(recs)} records, {sum(len(v) for v in edges.values())} edges, {os.path.getsize(OUT)} bytes -> {OUT}")


if __name__ == "__main__":
    main()
