"""GPU tests of the RSA signer's lane code (corda_amd/csrc/rsa_sign_wave.h) through the test-only device library
tests/native_rsa_sign/librsasignwave_gpu.so, one wave per case, against Python integers:
  * the paired product: the crafted operand classes of tests/rsa_wave_cases.py (zero runs, runs of ones,
    operands next to the modulus, the six modulus shapes, the edges 0 / 1 / m - 1) in each half of the wave
    while the other half multiplies random data, at Lh = 16, 17, 24, 32 (K = 1) and 33, 48, 64 (K = 2);
  * the windowed ladder: exponents 0, 1, 2, 15, 16, 2^j, all ones, zero limbs, a partial top window, bases
    0, 1, m - 1 and random, another exponent in each half;
  * the recombination: m1 < m2, m1 = m2, m2 >= p, a result with leading zero bytes;
  * the per-signature consistency check: a record whose dQ was altered after expansion gives
    CG_SIGN_CHECK_FAILED and zero limbs -- an arithmetic refusal.
"""
import random

import numpy as np
import pytest

import hostsignrsa as H
import rsa_wave_cases as RC
import rsasignwave as W

pytestmark = pytest.mark.gpu

SIZES = (16, 17, 24, 32, 33, 48, 64)  # Lh; K = 1 up to 32, 2 above
PER_CLASS = 3


def _mont_cases(Lh, rng):
    """(class name, a, b, m) with a b R^-1 mod m the product under test."""
    mods = RC.moduli(Lh, rng)
    out = []
    for mod in RC.MODULI:
        m = mods[mod]
        for name, (make, _, _) in RC._mont_classes(Lh, mod, m, rng).items():
            for _ in range(PER_CLASS):
                try:
                    a, b, _y = make()
                except ValueError:  # a run longer than this size has room for
                    break
                out.append((f"{mod}/{name}", a, b, m))
        out += [(f"{mod}/edge", a, b, m) for a in (0, 1, m - 1) for b in (0, 1, m - 1)]
    return out


@pytest.mark.parametrize("Lh", SIZES)
def test_paired_product_crafted_classes_in_each_half(Lh):
    rng = random.Random(0x2A11 + Lh)
    R = 1 << (32 * Lh)
    cases = _mont_cases(Lh, rng)
    assert len({c[0].split("/")[1] for c in cases}) >= 5
    recs, ops_a, ops_b, want, names = [], [], [], [], []
    for name, a, b, m in cases:
        for side in (0, 1):
            o = (rng.getrandbits(32 * Lh - 1) | (1 << (32 * Lh - 2)) | 1)  # the other half: a random odd modulus
            oa, ob = rng.randrange(o), rng.randrange(o)
            ms, as_, bs = ((m, o), (a, oa), (b, ob)) if side == 0 else ((o, m), (oa, a), (ob, b))
            rec = W.record(ms[0], ms[1], 0, 0, Lh=Lh, qinv=0)
            assert int(rec["K"]) == (1 if Lh <= 32 else 2)
            recs.append(rec)
            ops_a.append(W.pair(*as_))
            ops_b.append(W.pair(*bs))
            want.append(tuple(x * y * pow(R, -1, mm) % mm for x, y, mm in zip(as_, bs, ms)))
            names.append(f"{name} in half {side}")
    out, st = W.run(W.MONT2, recs, ops_a, ops_b)
    assert not st.any()
    for i, w in enumerate(want):
        assert W.unpair(out[i]) == w, names[i]


def _exponents(Lh, rng):
    B = 32 * Lh
    zero_limbs = rng.getrandbits(B) & ~(((1 << 96) - 1) << 32) | (1 << (B - 1))
    return [0, 1, 2, 15, 16, 1 << 4, 1 << 31, 1 << 32, 1 << (B - 1), (1 << B) - 1, zero_limbs,
            (1 << (B - 6)) | rng.getrandbits(B - 7),   # top window 0b0010: a partial top window
            (1 << (B - 35)) | rng.getrandbits(B - 40),  # the top limb zero
            rng.getrandbits(B)]


@pytest.mark.parametrize("Lh", SIZES)
def test_windowed_ladder_exponent_shapes_and_bases(Lh):
    rng = random.Random(0x1ADD + Lh)
    mp, mq = (rng.getrandbits(32 * Lh) | (1 << (32 * Lh - 1)) | 1 for _ in range(2))
    exps = _exponents(Lh, rng)
    recs, ops, want = [], [], []
    for i, e in enumerate(exps):
        e2 = exps[len(exps) - 1 - i]  # the other half runs another exponent
        for xp, xq in ((0, 1), (1, mq - 1), (mp - 1, 0), (rng.randrange(mp), rng.randrange(mq))):
            recs.append(W.record(mp, mq, e, e2, Lh=Lh, qinv=0))
            ops.append(W.pair(xp, xq))
            want.append((pow(xp, e, mp), pow(xq, e2, mq)))
    out, st = W.run(W.MODEXP2, recs, ops)
    assert not st.any()
    for i, w in enumerate(want):
        assert W.unpair(out[i]) == w, (hex(exps[i // 4]), i % 4)


def _crt(x1, x2, p, q):
    """The x below p q with x = x1 mod p and x = x2 mod q."""
    return (x2 + q * ((x1 - x2) * pow(q, -1, p) % p)) % (p * q)


KEYS = ("rsa1024", "rsa1024_swapped", "rsa1025", "rsa1032", "rsa2048e3", "rsa2048", "rsa3072", "rsa3072_swapped", "rsa4096")


def test_crt_recombination_edges_and_the_consistency_check():
    rng = random.Random(0xC127)
    recs, xs, want, names = [], [], [], []
    m2_ge_p = 0
    for kid in KEYS:
        k = H.key(kid)
        n, e, d, p, q = k["n"], k["e"], k["d"], k["p"], k["q"]
        rec = W.record(p, q, k["dp"], k["dq"], e=e, qinv=k["qinv"])
        lo = min(p, q)
        pairs = {"random": (rng.randrange(p), rng.randrange(q)),
                 "m1 < m2": (rng.randrange(lo // 2), lo // 2 + rng.randrange(lo // 2)),
                 "m1 = m2": (lo - 2, lo - 2), "m1 = m2 = 0": (0, 0), "m1 = 0": (0, rng.randrange(q)),
                 "m2 = 0": (rng.randrange(p), 0)}
        if q > p:
            pairs["m2 >= p"] = (rng.randrange(p), p + rng.randrange(q - p))
            pairs["m2 = p"] = (1, p)
            m2_ge_p += 1
        for name, (m1, m2) in pairs.items():
            x = _crt(pow(m1, e, p), pow(m2, e, q), p, q)  # x^dP = m1 mod p, x^dQ = m2 mod q
            assert pow(x, d, n) == _crt(m1, m2, p, q)
            recs.append(rec)
            xs.append(x)
            want.append((0, pow(x, d, n)))
            names.append(f"{kid}: {name}")
        s_small = rng.getrandbits(n.bit_length() - 80)  # at least 9 leading zero bytes
        recs.append(rec)
        xs.append(pow(s_small, e, n))
        want.append((0, s_small))
        names.append(f"{kid}: leading zero bytes")
        # the record altered after its expansion: dQ + 2 (s is then wrong modulo q alone)
        bad = W.record(p, q, k["dp"], k["dq"] + 2, e=e, qinv=k["qinv"])
        x = rng.randrange(2, n)
        assert pow(_crt(pow(x, k["dp"], p), pow(x, k["dq"] + 2, q), p, q), e, n) != x
        recs.append(bad)
        xs.append(x)
        want.append((W.SIGN_CHECK_FAILED, 0))
        names.append(f"{kid}: dQ altered")
    assert m2_ge_p >= 2
    out, st = W.run(W.CRT, recs, [W.limbs(x, 128) for x in xs])
    for i, (ws, w) in enumerate(want):
        assert (int(st[i]), W.from_limbs(out[i])) == (ws, w), names[i]
    assert W.SIGN_CHECK_FAILED == H.SIGN_CHECK_FAILED and np.count_nonzero(st) == len(KEYS)
