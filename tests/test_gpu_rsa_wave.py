"""The lane-cooperative RSA primitives on the device (corda_amd/csrc/rsa_wave.h through the test-only
library tests/native/rsa_wave_gpu.hip) on the crafted cases of tests/rsa_wave_cases.py: the result
limbs equal Python's integers exactly. tests/test_rsa_wave_model.py proves on the CPU which carry
chain, exponent branch and size class each case reaches."""
import pytest

import rsa_wave_cases as C
import rsa_wave_model as M
import rsawave

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(engine):  # `engine` first: the session's context (and torch's device init) come first
    return C.build(modexp_model=False)


def _bad(cs, got):
    return [(c["name"], c["L"], c.get("mod"), hex(g)[:40], hex(int(c["want"]))[:40])
            for c, g in zip(cs, got) if g != c["want"]]


def test_mont_mul(cases):
    cs = cases["mont_mul"]
    got = rsawave.mont_mul([c["a"] for c in cs], [c["b"] for c in cs], [c["n"] for c in cs],
                           [M.n0inv_of(c["n"]) for c in cs], [c["L"] for c in cs])
    bad = _bad(cs, got)
    assert not bad, (len(bad), bad[:10])
    assert len(cs) > 1000


def test_double_mod(cases):
    cs = cases["double_mod"]
    got = rsawave.double_mod([c["x"] for c in cs], [c["n"] for c in cs], [c["L"] for c in cs])
    bad = _bad(cs, got)
    assert not bad, (len(bad), bad[:10])


def test_geq(cases):
    cs = cases["geq"]
    got = rsawave.geq([c["a"] for c in cs], [c["b"] for c in cs], [c["L"] for c in cs])
    bad = [(c["name"], c["L"], g, c["want"]) for c, g in zip(cs, got) if g != c["want"]]
    assert not bad, bad


def test_modexp(cases):
    cs = cases["modexp"]
    got = rsawave.modexp([c["s"] for c in cs], [pow(2, 64 * c["L"], c["n"]) for c in cs], [c["n"] for c in cs],
                         [M.n0inv_of(c["n"]) for c in cs], [c["L"] for c in cs], [c["e"] for c in cs])
    bad = _bad(cs, got)
    assert not bad, (len(bad), bad[:10])
    assert {c["e"] for c in cs} == set(C.EXPONENTS)
