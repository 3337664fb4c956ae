"""ctypes access to tests/native/librsawave_gpu.so (rsa_wave_gpu.hip): the RSA kernels' lane-cooperative
primitives on the GPU, over Python integers. __graft_entry__.build() makes the library; a missing
library is an error, not a skip."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.environ.get("CORDA_AMD_RSAWAVE_LIB") or os.path.join(HERE, "native", "librsawave_gpu.so")
LIMBS = 128
_U32P = ctypes.POINTER(ctypes.c_uint32)
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise RuntimeError(f"{SO} is missing: run __graft_entry__.build() (make -C tests/native)")
        L = ctypes.CDLL(SO)
        L.rw_mont_mul.argtypes = [ctypes.c_uint32] + [_U32P] * 6
        L.rw_double_mod.argtypes = [ctypes.c_uint32] + [_U32P] * 4
        L.rw_geq.argtypes = [ctypes.c_uint32] + [_U32P] * 4
        L.rw_modexp.argtypes = [ctypes.c_uint32] + [_U32P] * 7
        _lib = L
    return _lib


def _limbs(vals):
    out = np.zeros((len(vals), LIMBS), dtype="<u4")
    for i, v in enumerate(vals):
        out[i] = np.frombuffer(int(v).to_bytes(4 * LIMBS, "little"), dtype="<u4")
    return out


def _words(vals):
    return np.ascontiguousarray(np.array(vals, dtype=np.uint32))


def _p(arr):
    return arr.ctypes.data_as(_U32P)


def _ints(out):
    return [int.from_bytes(row.tobytes(), "little") for row in out]


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: HIP error {rc}")


def mont_mul(a, b, n, n0inv, L):
    """Per case a b R^-1 mod n, R = 2^(32 L) (lists of integers; L: limbs per case)."""
    A, Bm, Nm, out = _limbs(a), _limbs(b), _limbs(n), np.zeros((len(a), LIMBS), dtype="<u4")
    n0, Lw = _words(n0inv), _words(L)
    _check(lib().rw_mont_mul(len(a), _p(A), _p(Bm), _p(Nm), _p(n0), _p(Lw), _p(out)), "rw_mont_mul")
    return _ints(out)


def double_mod(x, n, L):
    X, Nm, out = _limbs(x), _limbs(n), np.zeros((len(x), LIMBS), dtype="<u4")
    Lw = _words(L)
    _check(lib().rw_double_mod(len(x), _p(X), _p(Nm), _p(Lw), _p(out)), "rw_double_mod")
    return _ints(out)


def geq(a, b, L):
    A, Bm, out = _limbs(a), _limbs(b), np.zeros((len(a), LIMBS), dtype="<u4")
    Lw = _words(L)
    _check(lib().rw_geq(len(a), _p(A), _p(Bm), _p(Lw), _p(out)), "rw_geq")
    assert not out[:, 1:].any()
    return [bool(v) for v in out[:, 0]]


def modexp(s, rr, n, n0inv, L, e):
    S, Rm, Nm, out = _limbs(s), _limbs(rr), _limbs(n), np.zeros((len(s), LIMBS), dtype="<u4")
    n0, Lw, Ew = _words(n0inv), _words(L), _words(e)
    _check(lib().rw_modexp(len(s), _p(S), _p(Rm), _p(Nm), _p(n0), _p(Lw), _p(Ew), _p(out)), "rw_modexp")
    return _ints(out)
