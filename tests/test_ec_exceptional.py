"""ECDSA items that reach the exceptional cases of the ladders' mixed additions
(tests/ec_exceptional.py, tests/golden/gen_ec_exceptional.py, tests/golden/ec_exceptional.json) on
the CPU: both oracles, the generator, and every item through the host build of the lane code at the
radix it was made for, with every limb bound asserted and the host-only counters of jac_madd_w /
jac_madd9 (ecdsa.h EC_EXC_COUNT) held against what the item's note claims. The GPU cannot show
that a collision happened: this file does, on the same lane code; tests/test_gpu_ec_exceptional.py
then runs the items on the device."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

import ec_exceptional as EX
import golden_io
import test_scalar_edges as TSE
from corda_amd import batch as B
from oracle import c_oracle, corda

sys.path.insert(0, golden_io.GOLDEN)
import gen_ec_exceptional as GEN  # noqa: E402

ITEMS = golden_io.load("ec_exceptional.json")
SPECS = GEN.specs()
HELPERS = ["t_ecdsa_verify_rows", "t_ecdsa_verify_wide"]
WORKERS = TSE.WORKERS


def _py_oracle(job):
    it, mode = job
    return corda.verify_item(it["scheme"], it["key_fmt"], bytes.fromhex(it["key"]), bytes.fromhex(it["sig"]),
                             bytes.fromhex(it["msg"]), mode)


def test_both_oracles_give_the_fixtures_verdicts():
    """Python and C oracle, both modes: VALID as constructed, the neg@last items INVALID."""
    for it, sp in zip(ITEMS, SPECS):
        assert it["expect"] == it["expect_isvalid"] == ("INVALID" if sp["kind"] == "neg last" else "VALID"), it["note"]
    jobs = [(it, mode) for mode in (corda.MODE_DOVERIFY, corda.MODE_ISVALID) for it in ITEMS]
    with TSE._pool(WORKERS) as ex:
        got = list(ex.map(_py_oracle, jobs, chunksize=4))
    for (it, mode), st in zip(jobs, got):
        assert corda.STATUS_NAMES[st] == it["expect"], (it["note"], mode)
    b, exp, exp_iv = golden_io.sig_batch(ITEMS)
    assert np.array_equal(c_oracle.verify_batch(b, B.MODE_DOVERIFY, WORKERS), exp)
    assert np.array_equal(c_oracle.verify_batch(b, B.MODE_ISVALID, WORKERS), exp_iv)
    assert sorted(set(exp.tolist())) == [B.VALID, B.INVALID]


def test_fixture_is_what_the_generator_writes():
    """The file holds exactly the generator's list; every kind is there for both curves and every
    radix; a seeded sample of every class regenerates to the same bytes (identities asserted, Python
    oracle's verdict); one key per crafted item, one per curve for the filter items."""
    assert len(SPECS) == len(ITEMS)
    for sp, it in zip(SPECS, ITEMS):
        assert (sp["class"], sp["scheme"], sp["note"]) == (it["class"], it["scheme"], it["note"])
    for scheme in (3, 2):
        for w in EX.SE.WIDE_RADIXES:
            d = EX.SE.ec_g_digits(w)
            notes = {sp["note"] for sp in SPECS if sp["scheme"] == scheme and sp["w"] == w and sp["kind"] != "filter"}
            want = {f"dbl@{m}" for m in (0, 1, d // 2, d - 2, d - 1)} | {f"neg@{m}" for m in (0, 1, d // 2, d - 2)}
            want |= {"neg@1 gap", "neg@last", "dbl@1 neg@2", "control 0", "control 1"}
            assert notes == {f"w{w} {x}" for x in want}, (scheme, w)
    rng = random.Random(0xECE7)
    per_class = {}
    for i, it in enumerate(ITEMS):
        per_class.setdefault((it["class"], it["scheme"]), []).append(i)
    for _, idx in sorted(per_class.items()):
        for i in rng.sample(idx, min(3, len(idx))):
            assert GEN.make_item(SPECS[i], i) == ITEMS[i], ITEMS[i]["note"]
    crafted = [it["key"] for sp, it in zip(SPECS, ITEMS) if sp["kind"] != "filter"]
    assert len(set(crafted)) == len(crafted)
    for scheme in (3, 2):
        assert len({it["key"] for sp, it in zip(SPECS, ITEMS) if sp["kind"] == "filter" and sp["scheme"] == scheme}) <= 1
    # the filter search as the file records it: FILTER_KEEP items per curve, or the whole budget spent
    with open(GEN.PATH) as f:
        filt = json.load(f)["meta"]["filter"]
    for scheme in (3, 2):
        rec, kept = filt[str(scheme)], [sp["cand"] for sp in SPECS if sp["kind"] == "filter" and sp["scheme"] == scheme]
        assert kept == rec["hits"] == sorted(set(kept)) and len(kept) == min(rec["found"], GEN.FILTER_KEEP)
        assert rec["tried"] <= GEN.FILTER_BUDGET[scheme] and all(c < rec["tried"] for c in kept)
        assert len(kept) == GEN.FILTER_KEEP or rec["tried"] == GEN.FILTER_BUDGET[scheme]
    assert sum(sp["class"] == "k1_filter" for sp in SPECS) == GEN.FILTER_KEEP
    assert os.path.getsize(os.path.join(golden_io.GOLDEN, "ec_exceptional.json")) < 100 * 1000


# ---------------------------------------------------------------- host lane build, with the counters
def _lane_chunk(job):
    bits, helper, part = job
    lib = TSE._lane_lib(bits)
    lib.t_ec_exc_counts.argtypes = [ctypes.c_void_p]
    out = []
    cnt = np.zeros(4, np.uint64)
    for i, it in part:
        st = TSE._lane_verdict(lib, helper, it)
        assert lib.t_ec_exc_counts(TSE.ptr(cnt)) == 0
        out.append((i, st, tuple(int(x) for x in cnt)))
    return out


def _expected_counts(sp, bits, helper):
    """(doublings, infinities, loads, exact-path entries or None for 'at least 1') of an item at the
    radix it was made for."""
    assert sp["w"] == bits
    dbl, inf, loads = EX.EXPECT[sp["kind"]]
    if helper != "t_ecdsa_verify_wide":
        return dbl, inf, loads, 0  # no jac_madd9 in the row ladders
    return dbl, inf, loads, None if sp["kind"] == "filter" else dbl + inf


@pytest.mark.parametrize("helper", HELPERS)
@pytest.mark.parametrize("bits", [26, 24, 22])
def test_lanes_take_the_exceptional_paths_the_notes_name(bits, helper):
    """The items of one radix through the host build of that radix (every limb bound asserted; a
    violated bound aborts the worker): the fixture's verdict, and the counters of the ladder equal to
    what the note claims: jac_madd_w's doublings, infinities and loads, and jac_madd9's entries into
    the exact path (the number of exceptional additions; at least 1 for a filter item, whose H is
    not 0: no doubling, no infinity)."""
    idx = [i for i, sp in enumerate(SPECS) if sp["w"] == bits]
    assert len(idx) >= 2 * 14
    TSE._lane_lib(bits)  # built once, before the workers start
    chunks = [(bits, helper, [(i, ITEMS[i]) for i in idx[k::WORKERS]]) for k in range(WORKERS) if idx[k::WORKERS]]
    with TSE._pool(len(chunks)) as ex:
        got = {i: (st, cnt) for part in ex.map(_lane_chunk, chunks) for i, st, cnt in part}
    wrong = []
    for i in idx:
        st, cnt = got[i]
        dbl, inf, loads, exact = _expected_counts(SPECS[i], bits, helper)
        if SPECS[i]["kind"] != "filter":  # the table of the issue is what the exact walk gives
            assert (dbl, inf, loads) == EX.walk(SPECS[i]["t1"], SPECS[i]["v"], bits, EX.N[SPECS[i]["scheme"]])
        ok = st == ITEMS[i]["expect_isvalid"] and cnt[:3] == (dbl, inf, loads)
        ok = ok and (cnt[3] >= 1 if exact is None else cnt[3] == exact)
        if not ok:
            wrong.append((ITEMS[i]["note"], ITEMS[i]["scheme"], st, cnt))
    assert not wrong, (bits, helper, len(wrong), wrong[:10])


def test_crafted_items_at_another_radix():
    """The radix-2^24 and 2^22 items through the default (2^26) build (the GPU tests run every item
    in every context): the fixture's verdict, and the counters ec_exceptional.walk derives in exact
    integers for that radix. Most are plain controls there; some collide at every radix (the low
    digits spell the same partial sums), and neg@last ends at infinity at any radix."""
    idx = [i for i, sp in enumerate(SPECS) if sp["w"] != 26]
    chunks = [(26, "t_ecdsa_verify_rows", [(i, ITEMS[i]) for i in idx[k::WORKERS]]) for k in range(WORKERS)]
    TSE._lane_lib(26)
    with TSE._pool(len(chunks)) as ex:
        got = {i: (st, cnt) for part in ex.map(_lane_chunk, chunks) for i, st, cnt in part}
    plain = 0
    for i in idx:
        st, cnt = got[i]
        sp = SPECS[i]
        assert st == ITEMS[i]["expect_isvalid"], ITEMS[i]["note"]
        assert cnt[:3] == EX.walk(sp["t1"], sp["v"], 26, EX.N[sp["scheme"]]), (ITEMS[i]["note"], cnt)
        if sp["kind"] == "neg last":
            assert cnt[:3] == (0, 1, 1), (ITEMS[i]["note"], cnt)
        plain += cnt[:3] == (0, 0, 1)
    assert plain >= len(idx) // 2


def test_k1_filter_hits_are_the_first_of_the_search():
    """The search of the generator again for secp256k1 (a few hundred candidates, here through the
    bounds-checked build): the stored candidates are its first hits, in order."""
    lib = TSE._lane_lib(26)
    hits = GEN.stored_filter_hits()[2]
    n = hits[-1] + 1
    out = GEN.search_counts(lib, 2, range(n))
    assert [int(j) for j in np.flatnonzero(out)] == hits
