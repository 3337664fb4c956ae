"""ctypes access to the host build of the key-derivation lane code (tests/native/host_derive.cpp), one
shared library per fixed-base radix (-DED_WIDE_BW = -DEC_WIDE_GW = 26 / 24 / 22), built on demand the
way tests/hostsign.py builds host_sign.cpp; and the stand-alone sanitizer build of the same source
(-DDERIVE_MAIN)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "host_derive.cpp")
CSRC = os.path.join(HERE, "..", "corda_amd", "csrc")
RADIXES = (26, 24, 22)
CURVE_OF = {2: 0, 3: 1}  # scheme -> CG_CURVE_K1 / CG_CURVE_R1


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


def _radix(bw):
    return [f"-DED_WIDE_BW={bw}", f"-DEC_WIDE_GW={bw}"]


_libs = {}


def lib(bw):
    if bw not in _libs:
        so = _build(os.path.join(HERE, "native", f"libhostderive_bw{bw}.so"), _radix(bw) + ["-fPIC", "-shared"])
        lb = ctypes.CDLL(so)
        cp, u64, u32, i32 = ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        lb.t_hmac512.argtypes = [cp, u32, cp, u64, u32, cp]
        lb.t_hmac512.restype = None
        lb.t_hmac512_rehashed.argtypes = [cp, u32, cp, u64, u32, cp]
        lb.t_hmac512_rehashed.restype = None
        lb.t_accept.argtypes = [i32, cp]
        lb.t_ec_fixed_base.argtypes = [i32, cp, cp, ctypes.POINTER(ctypes.c_int32)]
        lb.t_derive_ec.argtypes = [i32, u32, cp, u32, cp, u64, u32, cp, cp, ctypes.POINTER(u32)]
        lb.t_derive_attempts.argtypes = [i32, u32, cp, cp, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        lb.t_derive_ed.argtypes = [cp, u32, cp, u64, u32, cp, cp]
        lb.t_derive_ed.restype = None
        lb.t_ed_public.argtypes = [cp, cp]
        lb.t_ed_public.restype = None
        assert lb.t_wide_bw() == bw
        _libs[bw] = lb
    return _libs[bw]


def sanitized_main(bw):
    """The stand-alone program over a case file, built with the address and undefined-behaviour sanitizers."""
    return _build(os.path.join(HERE, "native", f"host_derive_main_bw{bw}_asan"),
                  _radix(bw) + ["-DDERIVE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                "-fno-omit-frame-pointer"])


def hmac512(bw, key, msg, phase=0):
    out = ctypes.create_string_buffer(64)
    lib(bw).t_hmac512(key, len(key), msg, len(msg), phase, out)
    return out.raw


def hmac512_rehashed(bw, key, msg, phase=0):
    out = ctypes.create_string_buffer(128)
    lib(bw).t_hmac512_rehashed(key, len(key), msg, len(msg), phase, out)
    return out.raw[:64], out.raw[64:]


def accept(bw, scheme, d):
    return bool(lib(bw).t_accept(CURVE_OF[scheme], d.to_bytes(32, "big")))


def g_digits(bw):
    return lib(bw).t_g_digits()


def ec_fixed_base(bw, scheme, d):
    """(X || Y or None at infinity, the signed table digits)."""
    xy = ctypes.create_string_buffer(64)
    dg = (ctypes.c_int32 * g_digits(bw))()
    ok = lib(bw).t_ec_fixed_base(CURVE_OF[scheme], d.to_bytes(32, "big"), xy, dg)
    return (xy.raw if ok else None), list(dg)


def derive_ec(bw, scheme, key, seed, force=0, phase=0):
    """(status, secret, X || Y, rehashes) of one ECDSA item's lane."""
    sec, xy, tries = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64), ctypes.c_uint32(0)
    st = lib(bw).t_derive_ec(CURVE_OF[scheme], force, key, len(key), seed, len(seed), phase, sec, xy, ctypes.byref(tries))
    return st, sec.raw, xy.raw, tries.value


def derive_attempts(bw, scheme, macs, force=0):
    """ec_derive_attempts over injected macs: (status, d bytes of the last attempt, rehashes, rehash calls)."""
    assert len(macs) == 5 and all(len(m) == 64 for m in macs)
    d, tries, calls = ctypes.create_string_buffer(32), ctypes.c_uint32(0), ctypes.c_uint32(0)
    st = lib(bw).t_derive_attempts(CURVE_OF[scheme], force, b"".join(macs), d, ctypes.byref(tries), ctypes.byref(calls))
    return st, d.raw, tries.value, calls.value


def derive_ed(bw, key, seed, phase=0):
    sec, pub = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    lib(bw).t_derive_ed(key, len(key), seed, len(seed), phase, sec, pub)
    return sec.raw, pub.raw


def ed_public(bw, seed):
    pub = ctypes.create_string_buffer(32)
    lib(bw).t_ed_public(seed, pub)
    return pub.raw


def fixture():
    import derive_ref
    return derive_ref.load_fixture()


def recode(d, bw):
    """ec_recode_wide's signed radix-2^bw digits of d < 2^256 (every digit recentred)."""
    n = (257 + bw - 1) // bw
    out, carry = [], 0
    for t in range(n):
        e = ((d >> (t * bw)) & ((1 << bw) - 1)) + carry
        carry = (e + (1 << (bw - 1))) >> bw
        out.append(e - (carry << bw))
    assert carry == 0 and sum(x << (bw * t) for t, x in enumerate(out)) == d
    return out


def crafted_scalars(bw, n):
    """(note, d) for the G table's edges at radix 2^bw: the small scalars and n - 1, a zero digit in the
    first, a middle and the last row, a carry through every row, and the last entry (-2^(bw-1)) of every
    row below the top."""
    dg, half = (257 + bw - 1) // bw, 1 << (bw - 1)
    out = [("1", 1), ("2", 2), ("n - 1", n - 1)]
    top_bits = 256 - bw * (dg - 1)  # bits of d in the last row
    top = min(half, (1 << (top_bits - 1)) - 1) if top_bits > 1 else 0
    out.append(("every raw digit 2^(bw-1): a carry through every row",
                sum(half << (bw * t) for t in range(dg - 1)) + (top << (bw * (dg - 1)))))
    s = half + sum((half - 1) << (bw * t) for t in range(1, dg - 1))
    assert recode(s, bw)[:dg - 1] == [-half] * (dg - 1)
    out.append(("every digit below the top -2^(bw-1): the last entry of every row", s))
    base = sum((3 + t) << (bw * t) for t in range(dg - 1)) + (1 << (bw * (dg - 1)) if top_bits > 1 else 0)
    for name, row in (("first", 0), ("middle", dg // 2), ("last", dg - 1)):
        z = base - ((recode(base, bw)[row]) << (bw * row))
        assert recode(z, bw)[row] == 0
        out.append((f"zero digit in the {name} row", z))
    return [(k, v % n if v >= n else v) for k, v in out if 0 < (v % n if v >= n else v)]
