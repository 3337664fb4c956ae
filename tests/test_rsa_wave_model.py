"""CPU proof of what tests/rsa_wave_cases.py reaches: the lane model (tests/rsa_wave_model.py) of
corda_amd/csrc/rsa_wave.h equals Python's integers on every crafted case, every named class reaches
its event at every size and modulus it is drawn for, and the random controls reach no generate and no
carried propagate below L: random operands (every valid signature is one) never exercise the ballot
ripple of rsa_resolve, which is why the crafted cases exist. The device runs the same cases in
tests/test_gpu_rsa_wave.py."""
import collections
import random

import pytest

import rsa_wave_cases as C
import rsa_wave_model as M


@pytest.fixture(scope="module")
def cases():
    return C.build()


def test_model_equals_python_integers_on_every_case(cases):
    for op in ("mont_mul", "double_mod", "geq", "modexp"):
        bad = [(op, c["name"], c["L"], c.get("mod")) for c in cases[op] if c["model"] != c["want"]]
        assert not bad, bad[:10]
    assert sum(len(v) for v in cases.values()) > 2000


def test_every_class_reaches_its_event_at_every_size(cases):
    seen = collections.defaultdict(set)
    for op in ("mont_mul", "double_mod"):
        for c in cases[op]:
            if c["pred"] is not None:
                assert c["pred"](c["ev"]), (op, c["name"], c["L"], c["mod"], c["event"], c["ev"])
                seen[(op, c["name"])].add((c["L"], c["mod"]))
    every = {(L, m) for L in C.SIZES for m in C.MODULI}
    one, two = [L for L in C.SIZES if L <= 64], [L for L in C.SIZES if L > 64]
    big = ("topff", "allones", "2^B-c")
    want = {
        ("mont_mul", "zero_run_to_L-1"): every,
        ("mont_mul", "ones_run"): every,
        ("mont_mul", "over_hi"): {(L, m) for L in C.SIZES if L not in (64, 128) for m in big},
        ("mont_mul", "over_top"): {(L, m) for L in (64, 128) for m in big},
        ("mont_mul", "t_equals_n"): {(L, "p q") for L in C.SIZES},
        ("mont_mul", "largest_accumulator"): {(L, "allones") for L in C.SIZES},
        ("double_mod", "chain_into_top"): {(L, m) for L, m in every if m not in ("allones", "2^B-c")},
        ("double_mod", "over"): {(L, m) for L, m in every if m in ("allones", "2^B-c")},
    }
    for name in ("zero_run_1", "zero_run_2", "zero_run_16"):
        want[("mont_mul", name)] = {(L, m) for L in one for m in C.MODULI}
        for half in ("lower", "upper"):
            want[("mont_mul", f"{name}_{half}")] = {(L, m) for L in two for m in C.MODULI}
    assert dict(seen) == want
    # `hi` at the sizes with a partly filled or unused top lane, one and two limbs per lane
    hi = {c["L"] for c in cases["mont_mul"] if c["name"] == "over_hi" and c["ev"]["hi"]}
    assert {33, 63, 65, 127} <= hi
    # the worst-case operands keep the deferred accumulators inside the bound rsa_resolve states
    assert max(c["ev"]["max_acc"] for op in ("mont_mul", "double_mod") for c in cases[op]) < 1 << 35
    assert max(c["ev"]["max_acc"] for c in cases["modexp"]) < 1 << 35


def test_zero_runs_sit_where_their_class_says(cases):
    """The crafted result really has the run: its limbs are zero, the limbs beside it are not, and at
    two limbs per lane it starts on the half of the lane the class names."""
    for c in cases["mont_mul"]:
        if not c["name"].startswith("zero_run_") or c["name"] == "zero_run_to_L-1":
            continue
        parts = c["name"].split("_")
        length = int(parts[2])
        limbs = [(c["want"] >> (32 * i)) & 0xFFFFFFFF for i in range(c["L"])]
        starts = [i for i in range(1, c["L"] - length) if not any(limbs[i:i + length]) and limbs[i - 1] and limbs[i + length]]
        assert starts, (c["name"], c["L"], c["mod"])
        if len(parts) == 4:
            assert any(i % 2 == (0 if parts[3] == "lower" else 1) for i in starts), (c["name"], c["L"], c["mod"])
    for c in cases["mont_mul"]:
        if c["name"] == "zero_run_to_L-1":
            assert c["want"] < 1 << (32 * (c["L"] - 6))


def test_random_controls_never_reach_the_ripple(cases):
    ctl = [c for c in cases["mont_mul"] if c["name"] == "control"]
    assert collections.Counter(c["L"] for c in ctl) == {L: C.N_CONTROLS for L in C.SIZES}
    assert sum(c["ev"]["gen"] for c in ctl) == 0 and sum(c["ev"]["cprop"] for c in ctl) == 0
    # nor does a whole e = 65537 exponentiation of a random s under a random modulus
    for c in cases["modexp"]:
        if c["e"] == 65537 and c["mod"] == "random" and c["name"].endswith("s=random"):
            assert c["ev"]["gen"] == 0 and c["ev"]["cprop"] == 0, (c["L"], c["ev"])


def test_geq_and_modexp_cover_their_lists(cases):
    names = {c["name"] for c in cases["geq"]}
    assert {"equal", "limb_0", "top_limb", "low_lane_greater_high_lane_less", "limbs_of_one_lane_disagree"} <= names
    for L in C.SIZES:
        here = [c for c in cases["geq"] if c["L"] == L]
        assert {c["want"] for c in here} == {True, False}
        for name in {c["name"] for c in here} - {"equal", "zero_zero"}:
            assert sorted(c["want"] for c in here if c["name"] == name) == [False, True]  # both orders
        assert {(c["e"], c["name"].split("s=")[1]) for c in cases["modexp"] if c["L"] == L} == \
            {(e, s) for e in C.EXPONENTS for s in ("random", "0", "1", "n-1")}
    assert set(C.EXPONENTS) == {1, 2, 3, 4, 6, 0x10000, 65537, 0x80000001, 0xFFFFFFFF}


def test_model_key_preparation_ends_at_r_squared():
    rng = random.Random(7)
    for bits in (1024, 1025, 1032, 2048, 2049, 3072, 4096):
        n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        rr, ev = M.keyprep(n)
        assert rr == pow(2, 64 * ((bits + 31) // 32), n), bits
        row = ev.row(0)
        assert row["gen"] == 0 and row["cprop"] == 0, (bits, row)  # a random key reaches no ripple event
