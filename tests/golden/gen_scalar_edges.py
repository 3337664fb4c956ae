"""Generates tests/golden/scalar_edges.json: signatures whose ladder scalars are chosen exactly
(tests/scalar_edges.py lists them: the first, last and group-boundary entries of every table row,
the recoding carries, the top of the range), where every other fixture's scalars are random.

  Ed25519   the identity key 01 00 .. 00 (y = 1, x = 0): [h](-A) vanishes, so (R = encode([S mod L] B),
            S) verifies for every message; S is the B-ladder scalar itself. Also S in [L, 2^256): the
            verdict is whatever the i2p restatement says.
  ECDSA     a key solved from the target t. With k' fixed, r = x(k' G) mod n and e = SHA-256(msg):
              u1 = t:  s = e / t,  d = (k' - t) e / (r t)
              u2 = t:  s = r / t,  u1 = e / s,  d = (k' - u1) / t
            and Q = d G, so u1 G + u2 Q = k' G. Each item has its own key.

Items use the golden item schema (golden_io.sig_batch loads them). `class` is ed_s / ed_s_above_l /
ec_u1 / ec_u2, `note` names radix, row and pattern (tests/scalar_edges.py); a scalar that several
lists name is one item with the notes joined by "; ". Each list keeps N_RANDOM seeded random
controls. The file stores the items that are not only a per-row target (`in_fixture`), with `expect`
/ `expect_isvalid` from the Python oracle (oracle.corda.verify_item); the per-row items, three
quarters of the list at 330 to 410 bytes of JSON each, are made on demand by `all_items`, VALID as
constructed, and the tests hold them against both oracles. The eight small-order Ed25519 keys are
not included.

usage: python tests/golden/gen_scalar_edges.py
"""
import hashlib
import json
import os
import re
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import scalar_edges as SE  # noqa: E402
from oracle import corda, ecdsa_bc, ed25519_i2p as ed  # noqa: E402

N_RANDOM = 4  # seeded random controls per list
K_NONCE = {2: 0x5CA1AB1E0DDBA11C0FFEE0123456789ABCDEF02468ACE13579BDF0FEDCBA9877,
           3: 0x0DDBA11C0FFEE5CA1AB1E0FEDCBA98765432100123456789ABCDEF13579BDF02}


def specs():
    """The ordered, deduplicated (class, scheme, target, note) list of every item."""
    raw = []
    for w in SE.WIDE_RADIXES + (10,):
        raw += [("ed_s", 4, s, n) for n, s in SE.ed_s_targets(w, n_random=N_RANDOM)]
    raw += [("ed_s_above_l", 4, s, n) for n, s in SE.ed_s_above_l()]
    for scheme in (3, 2):
        for w in SE.WIDE_RADIXES + (10,):
            raw += [("ec_u1", scheme, t, n) for n, t in SE.ec_u1_targets(scheme, w, n_random=N_RANDOM)]
        for w in (6, 8):
            raw += [("ec_u2", scheme, t, n) for n, t in SE.ec_u2_targets(scheme, w, n_random=N_RANDOM)]
    out, at = [], {}
    for cls, scheme, t, note in raw:
        k = (cls if cls != "ed_s_above_l" else "ed_s", scheme, t)
        if k in at:
            out[at[k]]["note"] += "; " + note
        else:
            at[k] = len(out)
            out.append({"class": cls, "scheme": scheme, "target": t, "note": note})
    return out


def in_fixture(spec):
    """What scalar_edges.json stores: the items that are not only a per-row target ("w26 r3 h": one
    digit of one row). The per-row items are made by make_item when a test asks for them
    (all_items)."""
    return any(re.match(r"w\d+ r\d+ ", n) is None for n in spec["note"].split("; "))


_POW2 = {}


def _ec_mul_g(c, k):
    """k G as ecdsa_bc.ec_mul gives it (affine), 0 < k < n: the sum of the stored 2^i G over k's bits
    in Jacobian coordinates, one inversion."""
    if c.name not in _POW2:
        pts = [c.G]
        for _ in range(255):
            pts.append(ecdsa_bc.ec_add(c, pts[-1], pts[-1]))
        _POW2[c.name] = pts
    p, acc = c.p, None
    for i, (gx, gy) in enumerate(_POW2[c.name]):
        if not (k >> i) & 1:
            continue
        if acc is None:
            acc = (gx, gy, 1)
            continue
        X, Y, Z = acc
        zz = Z * Z % p
        h, r = (gx * zz - X) % p, (gy * zz * Z - Y) % p
        assert h != 0  # the running sum is below 2^i, and k < n: never +-2^i G
        hh = h * h % p
        v = X * hh % p
        X3 = (r * r - hh * h - 2 * v) % p
        acc = (X3, (r * (v - X3) - Y * hh * h) % p, h * Z % p)
    X, Y, Z = acc
    zi = pow(Z, p - 2, p)
    return X * zi * zi % p, Y * zi * zi * zi % p


def _ed_mul_b(k):
    """k B (extended), k < 2^253: the sum of the stored 2^i B over k's bits."""
    if "ed" not in _POW2:
        pts = [ed.B]
        for _ in range(252):
            pts.append(ed._dbl(pts[-1]))
        _POW2["ed"] = pts
    acc = ed.IDENT
    for i, pt in enumerate(_POW2["ed"]):
        if (k >> i) & 1:
            acc = ed._add(acc, pt)
    return acc


_R = {}


def _r_of(scheme):
    if scheme not in _R:
        c = ecdsa_bc.CURVES[scheme]
        _R[scheme] = ecdsa_bc.ec_mul(c, K_NONCE[scheme], c.G)[0] % c.n
    return _R[scheme]


def make_item(spec, index, oracle=True):
    """The item of specs()[index] (deterministic). oracle: `expect` from oracle.corda.verify_item
    (the fixture); else VALID as constructed, for the caller to hold against an oracle."""
    cls, scheme, t = spec["class"], spec["scheme"], spec["target"]
    msg = b"edge %05d" % index
    if scheme == 4:
        r_pt = ed.encode_point(ed._to_affine(_ed_mul_b(t % SE.L)))
        key, sig = SE.ED_IDENTITY_KEY, r_pt + t.to_bytes(32, "little")
    else:
        c = ecdsa_bc.CURVES[scheme]
        n, kp, r = c.n, K_NONCE[scheme], _r_of(scheme)
        e = int.from_bytes(hashlib.sha256(msg).digest(), "big") % n
        inv = lambda x: pow(x, n - 2, n)  # noqa: E731
        if cls == "ec_u1":
            s = e * inv(t) % n
            d = (kp - t) * e * inv(r * t) % n
        else:
            s = r * inv(t) % n
            d = (kp - e * inv(s)) * inv(t) % n
        assert s != 0 and d > 1
        w = inv(s)
        assert (e * w % n if cls == "ec_u1" else r * w % n) == t
        key, sig = ecdsa_bc.raw_key(_ec_mul_g(c, d)), ecdsa_bc.der_encode_sig(r, s)
    if oracle:
        st = corda.STATUS_NAMES[corda.verify_item(scheme, corda.KEY_RAW, key, sig, msg, corda.MODE_ISVALID)]
        assert st == "VALID" or cls == "ed_s_above_l", (spec, st)
    else:
        assert cls != "ed_s_above_l"
        st = "VALID"
    return {"class": cls, "note": spec["note"], "scheme": scheme, "key_fmt": corda.KEY_RAW, "key": key.hex(),
            "sig": sig.hex(), "msg": msg.hex(), "expect": st, "expect_isvalid": st}


_ALL = None


def all_items():
    """Every item of specs(), in order: the stored ones from scalar_edges.json, the per-row
    ones made here (a few seconds, once per process)."""
    global _ALL
    if _ALL is None:
        with open(os.path.join(HERE, "scalar_edges.json")) as f:
            stored = iter(json.load(f)["items"])
        _ALL = [next(stored) if in_fixture(sp) else make_item(sp, i, oracle=False) for i, sp in enumerate(specs())]
        assert next(stored, None) is None
    return _ALL


def _job(i):
    return make_item(_SPECS[i], i)


_SPECS = None


def main():
    global _SPECS
    _SPECS = specs()
    keep = [i for i, sp in enumerate(_SPECS) if in_fixture(sp)]
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        items = list(ex.map(_job, keep, chunksize=16))
    meta = {"generator": "tests/golden/gen_scalar_edges.py",
            "note": "crafted ladder scalars (tests/scalar_edges.py); expect = oracle.corda.verify_item; the per-row "
                    "items are not stored (gen_scalar_edges.all_items makes them)"}
    path = os.path.join(HERE, "scalar_edges.json")
    with open(path, "w") as f:
        f.write('{"meta": %s,\n"items": [\n' % json.dumps(meta))
        f.write(",\n".join(json.dumps(it, separators=(",", ":")) for it in items))
        f.write("\n]}\n")
    by = {}
    for it in items:
        by[it["class"], it["scheme"]] = by.get((it["class"], it["scheme"]), 0) + 1
    print(len(items), "of", len(_SPECS), "items stored,", os.path.getsize(path), "bytes;", by)


if __name__ == "__main__":
    main()
