"""ctypes access to the host build of the ECDSA signer's lane code (tests/native/host_sign_ec.cpp), one
shared library per fixed-base radix (-DED_WIDE_BW=-DEC_WIDE_GW=26 / 24 / 22), built the way tests/hostsign.py
builds host_sign.cpp; the stand-alone sanitizer build of the same source (-DSIGN_EC_MAIN); and the
fixture tests/golden/ecdsa_sign.json as uniform records."""
import ctypes
import hashlib
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "host_sign_ec.cpp")
CSRC = os.path.join(HERE, "..", "corda_amd", "csrc")
FIXTURE = os.path.join(HERE, "golden", "ecdsa_sign.json")
RADIXES = (26, 24, 22)
CURVE = {2: 0, 3: 1}  # scheme -> CG_CURVE_K1 / CG_CURVE_R1
SLOT = 72
EMPTY, NOT_RUN, NONCE_REJECTED, KEY_INVALID, UNSUPPORTED = 5, 255, 9, 3, 4


def _stale(out):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return t < os.path.getmtime(SRC) or t < max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)
                                               if f.endswith(".h"))


def _build(out, flags):
    if _stale(out):
        tmp = f"{out}.{os.getpid()}.tmp"  # build aside and rename: parallel test workers never load a partial file
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DFE_BOUNDS_CHECK", *flags, "-o", tmp, SRC])
        os.replace(tmp, out)
    return out


_libs = {}


def lib(bw):
    if bw not in _libs:
        so = _build(os.path.join(HERE, "native", f"libhostsignec_bw{bw}.so"),
                    [f"-DED_WIDE_BW={bw}", f"-DEC_WIDE_GW={bw}", "-fPIC", "-shared"])
        lb = ctypes.CDLL(so)
        vp, cp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        lb.t_x_mod_n.argtypes = [i32, cp, cp]
        lb.t_der.argtypes = [cp, cp, cp]
        lb.t_der.restype = u32
        lb.t_signer_load.argtypes = [i32, cp, cp]
        lb.t_sign_arena.argtypes = [i32, cp, cp, u64, u32, cp, cp, vp, vp]
        lb.t_sign_splice.argtypes = [i32, cp, cp, u32, cp, cp, u32, cp, cp, vp]
        assert lb.t_wide_bw() == bw
        _libs[bw] = lb
    return _libs[bw]


def sanitized_main(bw):
    """The stand-alone program over a case file, built with the address and undefined-behaviour sanitizers."""
    return _build(os.path.join(HERE, "native", f"host_sign_ec_main_bw{bw}_asan"),
                  [f"-DED_WIDE_BW={bw}", f"-DEC_WIDE_GW={bw}", "-DSIGN_EC_MAIN", "-fsanitize=address,undefined",
                   "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def sign_arena(bw, scheme, d, msg, k, phase=0, digits=None):
    """(status, length, the 72-byte slot) of the arena-form lane."""
    out, ln = ctypes.create_string_buffer(SLOT), ctypes.c_uint32(0)
    st = lib(bw).t_sign_arena(CURVE[scheme], d, msg if msg else b"\0", len(msg), phase, k, out, ctypes.byref(ln),
                              digits)
    return st, ln.value, out.raw


def sign_splice(bw, scheme, d, prefix, tx_id, suffix, k):
    out, ln = ctypes.create_string_buffer(SLOT), ctypes.c_uint32(0)
    st = lib(bw).t_sign_splice(CURVE[scheme], d, prefix, len(prefix), tx_id, suffix, len(suffix), k, out,
                               ctypes.byref(ln))
    return st, ln.value, out.raw


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with open(FIXTURE) as f:
            _fixture = json.load(f)
    return _fixture


def key(scheme):
    """(d, X || Y) of the fixture's key of `scheme`."""
    k = fixture()["keys"][str(scheme)]
    return bytes.fromhex(k["d"]), bytes.fromhex(k["pub"])


def records():
    """The fixture's full records: dicts with scheme, note, d, k, status, sig (the DER bytes, b"" when the
    item is not signed) and either msg or prefix / id / suffix, all as bytes."""
    out = []
    for r in fixture()["records"]:
        q = {"scheme": r["scheme"], "note": r["note"], "status": r["status"],
             "d": bytes.fromhex(r["d"]) if "d" in r else key(r["scheme"])[0]}
        for f in ("k", "sig", "msg", "prefix", "id", "suffix"):
            if f in r:
                q[f] = bytes.fromhex(r[f])
        out.append(q)
    return out


def edges():
    """The G-table edge records: (scheme, k as 32 bytes, digest); the message is edge_msg(), the key key(scheme)."""
    return [(int(s), int(k, 16).to_bytes(32, "big"), bytes.fromhex(h)) for s, rows in fixture()["edges"].items()
            for k, h in rows]


def edge_msg():
    return bytes.fromhex(fixture()["edge_msg"])


def digest(sig):
    return hashlib.sha256(sig).digest()[:12]


def record_message(r):
    return r["msg"] if "msg" in r else r["prefix"] + r["id"] + r["suffix"]


def slot(sig):
    return sig + bytes(SLOT - len(sig))
