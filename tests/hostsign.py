"""ctypes access to the host build of the Ed25519 signer's lane code (tests/native/host_sign.cpp), one
shared library per fixed-base radix (-DED_WIDE_BW=26 / 24 / 22), built the way tests/hostk.py builds
host_kernels.cpp; and the stand-alone sanitizer build of the same source (-DSIGN_MAIN)."""
import ctypes
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "host_sign.cpp")
CSRC = os.path.join(HERE, "..", "corda_amd", "csrc")
FIXTURE = os.path.join(HERE, "golden", "ed25519_sign.json")
RADIXES = (26, 24, 22)
L = 2 ** 252 + 27742317777372353535851937790883648493


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
        so = _build(os.path.join(HERE, "native", f"libhostsign_bw{bw}.so"), [f"-DED_WIDE_BW={bw}", "-fPIC", "-shared"])
        lb = ctypes.CDLL(so)
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        lb.t_sc_muladd.argtypes = [vp, vp, vp, vp]
        lb.t_fixed_base.argtypes = [vp, vp, vp]
        lb.t_sha512_prefix_arena.argtypes = [i32, vp, ctypes.c_char_p, u64, u32, vp]
        lb.t_sha512_prefix_splice.argtypes = [i32, vp, ctypes.c_char_p, u32, ctypes.c_char_p, ctypes.c_char_p, u32, vp]
        lb.t_signer_expand.argtypes = [vp, vp]
        lb.t_sign_arena.argtypes = [vp, ctypes.c_char_p, u64, u32, vp]
        lb.t_sign_splice.argtypes = [vp, ctypes.c_char_p, u32, ctypes.c_char_p, ctypes.c_char_p, u32, vp]
        assert lb.t_wide_bw() == bw
        _libs[bw] = lb
    return _libs[bw]


def sanitized_main(bw):
    """The stand-alone program over a case file, built with the address and undefined-behaviour sanitizers."""
    return _build(os.path.join(HERE, "native", f"host_sign_main_bw{bw}_asan"),
                  [f"-DED_WIDE_BW={bw}", "-DSIGN_MAIN", "-fsanitize=address,undefined",
                   "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def words(b):
    return np.frombuffer(bytes(b), dtype="<u4").copy()


def scalar_words(x):
    return words(int(x).to_bytes(32, "little"))


def records():
    with open(FIXTURE) as f:
        return json.load(f)["records"]


def record_message(r):
    return bytes.fromhex(r["msg"]) if "msg" in r else \
        bytes.fromhex(r["prefix"]) + bytes.fromhex(r["id"]) + bytes.fromhex(r["suffix"])


def n_digits(bw):
    return (253 + bw - 1) // bw


def recode(s, bw):
    """sc_recode_wb's signed radix-2^bw digits of s < 2^253."""
    out, carry = [], 0
    for t in range(n_digits(bw)):
        e = ((s >> (t * bw)) & ((1 << bw) - 1)) + carry
        carry = (e + (1 << (bw - 1))) >> bw
        out.append(e - (carry << bw))
    assert carry == 0 and sum(d << (bw * t) for t, d in enumerate(out)) == s
    return out


def crafted_scalars(bw):
    """(note, scalar) for the fixed-base table's edges at radix 2^bw: the small scalars, the order's
    neighbours, every raw digit 2^(bw-1) (a carry out of every row), every recoded digit below the top
    -2^(bw-1) (the last entry of every row), and a zero digit in the first, a middle and the last row."""
    d, half = n_digits(bw), 1 << (bw - 1)
    top_bits = 253 - bw * (d - 1)
    out = [("0", 0), ("1", 1), ("2", 2), ("L - 1", L - 1), ("2^252", 2 ** 252)]
    # every raw digit 2^(bw-1) (the top one as far as 2^253 allows): each recodes to -2^(bw-1) or its
    # neighbour and carries into the next row
    top = min(half, (1 << top_bits) - 1)
    out.append(("every raw digit 2^(bw-1)", sum(half << (bw * t) for t in range(d - 1)) + (top << (bw * (d - 1)))))
    # every recoded digit below the top is -2^(bw-1): raw digit 0 = 2^(bw-1), the others 2^(bw-1) - 1
    s = half + sum((half - 1) << (bw * t) for t in range(1, d - 1))
    assert recode(s, bw) == [-half] * (d - 1) + [1]
    out.append(("every digit below the top -2^(bw-1)", s))
    base = sum((3 + t) << (bw * t) for t in range(d))
    for name, row in (("first", 0), ("middle", d // 2), ("last", d - 1)):
        z = base - ((3 + row) << (bw * row))
        assert recode(z, bw)[row] == 0 and all(x != 0 for t, x in enumerate(recode(z, bw)) if t != row)
        out.append((f"zero digit in the {name} row", z))
    for _, v in out:
        assert 0 <= v < 2 ** 253
    return out
