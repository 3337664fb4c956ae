"""Python side of the test-only device library tests/native_rsa_sign/librsasignwave_gpu.so (rsa_sign_wave_gpu.hip
over corda_amd/csrc/rsa_sign_wave.h): signer records made from Python integers, paired operands, and the three
operations. Expected values are Python integer arithmetic, computed by the tests."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "native_rsa_sign", "librsasignwave_gpu.so")
MONT2, MODEXP2, CRT = 0, 1, 2
SIGN_CHECK_FAILED = 10  # CG_SIGN_CHECK_FAILED

# RsaSignerRec (corda_amd/csrc/rsa_sign_wave.h)
REC_DTYPE = np.dtype([(f, "<u4") for f in ("ok", "bits", "L", "Lh", "K", "k", "em_bits", "block_len", "e", "n0inv_n",
                                           "n0inv_p", "n0inv_q")] +
                     [(f, "<u4", 128) for f in ("n", "rr_n", "qr_n")] +
                     [(f, "<u4", 64) for f in ("p", "q", "dp", "dq", "rr_p", "rr_q", "r3_p", "r3_q", "qinv")])

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(LIB_PATH)
        L.rs_rec_bytes.restype = ctypes.c_uint
        L.rs_run.argtypes = [ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5
        L.rs_run.restype = ctypes.c_int
        assert L.rs_rec_bytes() == REC_DTYPE.itemsize
        _lib = L
    return _lib


def limbs(v, count):
    assert 0 <= v < 1 << (32 * count)
    return np.frombuffer(v.to_bytes(4 * count, "little"), dtype="<u4")


def from_limbs(a):
    return int.from_bytes(np.ascontiguousarray(a, dtype="<u4").tobytes(), "little")


def n0inv(m):
    return (-pow(m, -1, 1 << 32)) % (1 << 32)


def k_of(L, Lh):
    """K as k_rsa_signer_expand chooses it."""
    return 2 if L > 64 or Lh > 32 else 1


def record(p, q, dp, dq, e=65537, n=None, Lh=None, qinv=None):
    """The record of a key (or of two arbitrary odd moduli p, q for the paired operations). Lh: the common
    limb count of the two sides (default: limbs(max(p, q)))."""
    n = p * q if n is None else n
    bits = n.bit_length()
    L = (bits + 31) // 32
    Lh = (max(p.bit_length(), q.bit_length()) + 31) // 32 if Lh is None else Lh
    R, Rn = 1 << (32 * Lh), 1 << (32 * L)
    r = np.zeros((), dtype=REC_DTYPE)
    r["ok"], r["bits"], r["L"], r["Lh"], r["K"], r["k"] = 1, bits, L, Lh, k_of(L, Lh), (bits + 7) // 8
    r["em_bits"], r["block_len"], r["e"] = bits - 1, (bits + 6) // 8, e
    r["n0inv_n"], r["n0inv_p"], r["n0inv_q"] = n0inv(n), n0inv(p), n0inv(q)
    r["n"], r["rr_n"], r["qr_n"] = limbs(n, 128), limbs(Rn * Rn % n, 128), limbs(q * Rn % n, 128)
    for f, v in (("p", p), ("q", q), ("dp", dp), ("dq", dq), ("rr_p", R * R % p), ("rr_q", R * R % q),
                 ("r3_p", R * R * R % p), ("r3_q", R * R * R % q),
                 ("qinv", pow(q, -1, p) if qinv is None else qinv)):
        r[f] = limbs(v, 64)
    return r


def pair(lo, hi):
    """A paired operand: the p side's value and the q side's."""
    return np.concatenate([limbs(lo, 64), limbs(hi, 64)])


def unpair(a):
    return from_limbs(a[:64]), from_limbs(a[64:])


def run(op, recs, a, b=None):
    """recs: list of records; a, b: per case 128 limbs. Returns (out [count, 128], status [count])."""
    count = len(recs)
    rec = np.ascontiguousarray(np.stack(recs)) if count else np.zeros(0, dtype=REC_DTYPE)
    a = np.ascontiguousarray(np.stack(a), dtype="<u4")
    b = a if b is None else np.ascontiguousarray(np.stack(b), dtype="<u4")
    assert a.shape == (count, 128) and b.shape == (count, 128)
    out = np.zeros((count, 128), dtype="<u4")
    st = np.zeros(count, dtype="<u4")
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib().rs_run(op, count, p(rec), p(a), p(b), p(out), p(st))
    assert rc == 0, f"rs_run: {rc}"
    return out, st
