"""Generates tests/golden/ec_exceptional.json: valid ECDSA signatures whose fixed-base additions are
doublings or cancellations (tests/ec_exceptional.py lists the (t1, v) pairs), and ordinary
signatures that are false positives of the wide ladder's limb-0 filter (ec9.h ec9_maybe_zero).

  crafted   e = SHA-256(msg) is fixed by the message; u1 = t1 and the accumulator v G after the Q
            part are chosen:
              k' = v + t1,  r = x(k' G) mod n,  s = e / t1,  u2 = r / s,  d = v / u2,  Q = d G
            so u2 Q = v G and u1 G + u2 Q = k' G: VALID, and the Q part ends exactly at v G.
            neg@last has k' = 0 (INVALID); its r is the x of a fixed multiple of G.
  filter    one key d per curve and one nonce k' (so r is fixed), msg_i = b"filter %07d" % i,
            s_i = (e_i + r d) / k': ordinary VALID signatures. The host build's t_ec_filter_search
            (tests/native/host_kernels.cpp, compiled here at -O2 without the bounds checks) runs
            the 32 Q-part additions of the wide ladder on u2_i = r / s_i over the key's table and
            counts jac_madd9's entries into the exact path; the first FILTER_KEEP hits per curve
            among FILTER_BUDGET candidates are kept. `meta.filter` records what was tried and
            found; `specs` reads the kept candidates from there (the search is not repeated).

Items use the golden item schema with `class`, `note` and `expect` / `expect_isvalid` from the
Python oracle (oracle.corda.verify_item). One key per crafted item.

usage: python tests/golden/gen_ec_exceptional.py
"""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ec_exceptional as EX  # noqa: E402
import scalar_edges as SE  # noqa: E402
from gen_scalar_edges import K_NONCE, _ec_mul_g  # noqa: E402
from oracle import corda, ecdsa_bc  # noqa: E402

PATH = os.path.join(HERE, "ec_exceptional.json")
FILTER_KEEP = 4
FILTER_BUDGET = {3: 1000000, 2: 2000}  # candidates per curve (r1: ~2^22 / 32 per hit expected)
FILTER_CHUNK = 31250
FILTER_ROUND = 16 * FILTER_CHUNK  # candidates between two looks at the hit count
_frng = random.Random(0xF117E2)
FILTER_D = {s: _frng.randrange(2, SE.N[s] - 1) for s in (3, 2)}
FILTER_K = {s: _frng.randrange(2, SE.N[s] - 1) for s in (3, 2)}


def _e(msg, n):
    return int.from_bytes(hashlib.sha256(msg).digest(), "big") % n


def _inv(x, n):
    return pow(x, n - 2, n)


def stored_filter_hits():
    """{scheme: [candidate, ...]} as the committed fixture's meta records them."""
    with open(PATH) as f:
        meta = json.load(f)["meta"]
    return {int(s): list(v["hits"]) for s, v in meta["filter"].items()}


def specs(filter_hits=None):
    """The ordered list of every item: ec_exceptional.specs(), then the filter items."""
    out = [dict(sp, **{"class": sp["kind"]}) for sp in EX.specs()]
    hits = stored_filter_hits() if filter_hits is None else filter_hits
    for scheme in (3, 2):
        cls = "r1_filter" if scheme == 3 else "k1_filter"
        out += [{"class": cls, "kind": "filter", "scheme": scheme, "w": 26, "note": f"{cls} candidate {i}", "cand": i}
                for i in hits.get(scheme, [])]
    return out


_FIXED = {}


def _filter_fixed(scheme):
    if scheme not in _FIXED:
        c = ecdsa_bc.CURVES[scheme]
        r = _ec_mul_g(c, FILTER_K[scheme])[0] % c.n
        assert r != 0
        _FIXED[scheme] = (r, ecdsa_bc.raw_key(_ec_mul_g(c, FILTER_D[scheme])))
    return _FIXED[scheme]


def filter_sig(scheme, i):
    """(msg, r, s, u2) of filter candidate i."""
    n = SE.N[scheme]
    r, _ = _filter_fixed(scheme)
    msg = b"filter %07d" % i
    s = (_e(msg, n) + r * FILTER_D[scheme]) * _inv(FILTER_K[scheme], n) % n
    assert s != 0
    return msg, r, s, r * _inv(s, n) % n


def make_item(spec, index, oracle=True):
    """The item of specs()[index] (deterministic), with every identity of its construction asserted."""
    scheme = spec["scheme"]
    c = ecdsa_bc.CURVES[scheme]
    n = c.n
    if spec["kind"] == "filter":
        msg, r, s, _ = filter_sig(scheme, spec["cand"])
        key = _filter_fixed(scheme)[1]
        want = "VALID"
    else:
        w, t1, v = spec["w"], spec["t1"], spec["v"]
        d_g = SE.ec_g_digits(w)
        g = SE.recode(t1, w, d_g)
        assert sum(x << (w * i) for i, x in enumerate(g)) == t1 and 0 < t1 < n and 0 < v < n
        zero = [i for i, x in enumerate(g) if x == 0]
        assert zero == ([2] if spec["kind"] == "neg gap" else [])
        acc = v  # the walk over the rows: which additions meet +-(the accumulator)
        hit = []
        for m, x in enumerate(g):
            step = x << (w * m)
            if x != 0 and acc in (step % n, -step % n):
                hit.append(m)
            acc = (acc + step) % n
        assert hit == spec["rows"], (spec["note"], hit)
        if spec["kind"] == "dbl neg":
            assert (g[1], g[2]) == (-(1 << (w - 1)), 1)
        msg = b"exc %05d" % index
        e = _e(msg, n)
        kp = (v + t1) % n
        assert (kp == 0) == (spec["kind"] == "neg last")
        r = (_ec_mul_g(c, kp)[0] if kp else ecdsa_bc.ec_mul(c, K_NONCE[scheme], c.G)[0]) % n
        s = e * _inv(t1, n) % n
        u2 = r * _inv(s, n) % n
        d = v * _inv(u2, n) % n
        assert r != 0 and s != 0 and d not in (0, 1, n - 1)
        assert e * _inv(s, n) % n == t1 and (t1 + u2 * d) % n == kp
        key = ecdsa_bc.raw_key(_ec_mul_g(c, d))
        want = "INVALID" if kp == 0 else "VALID"
    sig = ecdsa_bc.der_encode_sig(r, s)
    if oracle:
        st = corda.STATUS_NAMES[corda.verify_item(scheme, corda.KEY_RAW, key, sig, msg, corda.MODE_ISVALID)]
        assert st == want, (spec["note"], st)
    return {"class": spec["class"], "note": spec["note"], "scheme": scheme, "key_fmt": corda.KEY_RAW, "key": key.hex(),
            "sig": sig.hex(), "msg": msg.hex(), "expect": want, "expect_isvalid": want}


# ---------------------------------------------------------------- the filter search
SEARCH_SO = os.path.join(os.path.dirname(HERE), "native", "libhostkernels_search.so")


def build_search_so():
    """The host build at -O2 with the counters and without the bounds checks (the search alone; the
    kept items go through the bounds-checked build in tests/test_ec_exceptional.py)."""
    src = os.path.join(os.path.dirname(HERE), "native", "host_kernels.cpp")
    tmp = f"{SEARCH_SO}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DFE_OP_COUNT", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, SEARCH_SO)


def search_counts(lib, scheme, cands):
    """jac_madd9's exact-path entries over the Q part of each candidate's wide ladder."""
    lib.t_ec_filter_search.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    u2 = np.frombuffer(b"".join(filter_sig(scheme, i)[3].to_bytes(32, "little") for i in cands), dtype="<u4").copy()
    key = np.frombuffer(_filter_fixed(scheme)[1], dtype=np.uint8).copy()
    out = np.zeros(len(cands), np.uint8)
    st = lib.t_ec_filter_search(scheme, key.ctypes.data, u2.ctypes.data, len(cands), out.ctypes.data)
    assert st == 0, st
    return out


def _search_chunk(job):
    scheme, lo, hi = job
    out = search_counts(ctypes.CDLL(SEARCH_SO), scheme, range(lo, hi))
    return [lo + int(j) for j in np.flatnonzero(out)]


def search(scheme, ex):
    """(candidates tried, every hit among them): whole chunks in order, until FILTER_KEEP hits or the
    budget."""
    hits, tried = [], 0
    while tried < FILTER_BUDGET[scheme] and len(hits) < FILTER_KEEP:
        jobs = [(scheme, lo, min(lo + FILTER_CHUNK, FILTER_BUDGET[scheme]))
                for lo in range(tried, min(tried + FILTER_ROUND, FILTER_BUDGET[scheme]), FILTER_CHUNK)]
        for part in ex.map(_search_chunk, jobs):
            hits += part
        tried = jobs[-1][2]
    return tried, sorted(hits)


def _job(i):
    return make_item(_SPECS[i], i)


_SPECS = None


def main():
    global _SPECS
    build_search_so()
    meta_filter, hits = {}, {}
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        for scheme in (3, 2):
            tried, found = search(scheme, ex)
            hits[scheme] = found[:FILTER_KEEP]
            meta_filter[str(scheme)] = {"tried": tried, "found": len(found), "hits": hits[scheme]}
            print("scheme", scheme, "tried", tried, "hits", found)
        _SPECS = specs(hits)
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as ex:  # forked after _SPECS is set
        items = list(ex.map(_job, range(len(_SPECS)), chunksize=4))
    meta = {"generator": "tests/golden/gen_ec_exceptional.py",
            "note": "ECDSA items whose fixed-base additions are doublings / cancellations (tests/ec_exceptional.py), "
                    "and false positives of ec9.h's limb-0 filter; expect = oracle.corda.verify_item",
            "filter": meta_filter}
    with open(PATH, "w") as f:
        f.write('{"meta": %s,\n"items": [\n' % json.dumps(meta))
        f.write(",\n".join(json.dumps(it, separators=(",", ":")) for it in items))
        f.write("\n]}\n")
    by = {}
    for it in items:
        by[it["class"], it["scheme"]] = by.get((it["class"], it["scheme"]), 0) + 1
    print(len(items), "items,", os.path.getsize(PATH), "bytes;", by)


if __name__ == "__main__":
    main()
