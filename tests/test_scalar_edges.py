"""Crafted ladder scalars (tests/scalar_edges.py, tests/golden/scalar_edges.json and the per-row
items tests/golden/gen_scalar_edges.py makes on demand) on the CPU: the device recodings on
every target, the items against both oracles and their generator, and every
fixture item through the host build of the lane code (every limb bound asserted), at the default
fixed-base radix and, for their own targets, at the two budgeted radixes. A GPU mismatch in
tests/test_gpu_scalar_edges.py is debugged here."""
import ctypes
import multiprocessing
import os
import random
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import golden_io
import hostk
import scalar_edges as SE
from corda_amd import batch as B
from hostk import ptr, words
from oracle import c_oracle, corda

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_scalar_edges as GEN  # noqa: E402

ITEMS = GEN.all_items  # every item: the stored ones and the per-row ones the generator makes (cached)
STORED = golden_io.load("scalar_edges.json")
ED_NAMES = {0: "VALID", 1: "INVALID", 3: "KEY_INVALID"}
EC_NAMES = {0: "VALID", 1: "INVALID", 2: "SIG_MALFORMED", 3: "KEY_INVALID"}
WORKERS = min(16, len(os.sched_getaffinity(0)))


def _pool(n):
    """Worker processes, spawned: a fork of the test process can fail once the host builds of the
    lane code have reserved their (sparsely touched) multi-gigabyte tables in it."""
    return ProcessPoolExecutor(n, mp_context=multiprocessing.get_context("spawn"))


def _constructed_valid(it):
    """Items whose construction proves VALID: an ECDSA target, or an Ed25519 S below L."""
    return it["scheme"] != 4 or int.from_bytes(bytes.fromhex(it["sig"])[32:], "little") < SE.L


# ---------------------------------------------------------------- recodings
def _words256(x):
    return np.frombuffer(x.to_bytes(32, "little"), dtype="<u4").copy()


def _check_digits(fn, w, lists, top_unsigned=False):
    lib = hostk.lib()
    f = getattr(lib, fn)
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    h, reached, n = 1 << (w - 1), set(), 0
    out = np.zeros(64, np.int32)
    for note, x in lists:
        d = f(w, ptr(_words256(x)), ptr(out))
        assert d > 0, (fn, w)
        dg = [int(v) for v in out[:d]]
        assert sum(v << (w * i) for i, v in enumerate(dg)) == x, (note, dg)
        assert dg == SE.recode(x, w, d, top_unsigned), note
        for i, v in enumerate(dg):
            if top_unsigned and i == d - 1:
                assert 0 <= v <= 2 * h, (note, i, v)  # rows 31 and 32 of EcWideTab: 1..256
            else:
                assert -h <= v <= h, (note, i, v)     # a row holds the multiples 1..2^(w-1)
            reached.add((i, abs(v)))
        n += 1
    return reached, d, n


@pytest.mark.parametrize("w", [26, 24, 22, 10])
def test_ed25519_b_recoding_on_every_target(w):
    """sc_recode_wb<w> (w = 10: sc_recode_w16) on every S target: the digits sum to S, stay within
    the row's entries, and the lists reach the first and the last entry of every row below the top."""
    lists = SE.ed_s_targets(w)
    reached, d, n = _check_digits("t_sc_recode_wb", w, lists)
    assert d == SE.ed_digits(w) and n == len(lists) > 6 * d
    for u in range(d - 1):
        assert {(u, 1), (u, 2), (u, (1 << (w - 1)) - 1), (u, 1 << (w - 1))} <= reached, u
    if w in SE.WIDE_RADIXES:
        g = SE.group_sizes()["ed_b"]
        assert all({(u, g), (u, g + 1)} <= reached for u in range(d - 1))


@pytest.mark.parametrize("scheme", [2, 3])
@pytest.mark.parametrize("w", [26, 24, 22, 10])
def test_ecdsa_g_recoding_on_every_target(w, scheme):
    """ec_recode_wide<w, EC_WIDE_GDIGITS, false> (w = 10: ec_recode_w10) on every u1 target."""
    lists = SE.ec_u1_targets(scheme, w)
    reached, d, n = _check_digits("t_ec_recode", w, lists)
    assert n == len(lists) > 8 * (d - 1)
    assert d == (SE.ec_g_digits(w) if w in SE.WIDE_RADIXES else 26)
    g = SE.group_sizes()["ec_g"]
    for u in range(d - 1):
        assert {(u, 1), (u, 2), (u, g), (u, g + 1), (u, (1 << (w - 1)) - 1), (u, 1 << (w - 1))} <= reached, u
    if w in SE.WIDE_RADIXES:  # a table-build launch ends inside some row: both sides are listed
        assert any("+1" in note and " e" in note for note, _ in lists)


@pytest.mark.parametrize("scheme", [2, 3])
@pytest.mark.parametrize("w", [6, 8])
def test_ecdsa_per_key_recoding_on_every_target(w, scheme):
    """ec_recode_w6 and ec_recode_wide<8, 32, TopUnsigned> on every u2 target; radix 2^8 reaches the
    top digits 128, 129, 255 and 256 (the 33rd row) and both sides of the row lanes' boundary."""
    lists = SE.ec_u2_targets(scheme, w)
    reached, d, n = _check_digits("t_ec_recode", w, lists, top_unsigned=w == 8)
    assert n == len(lists)
    h = 1 << (w - 1)
    for u in range(d - 1):
        assert {(u, 1), (u, 2), (u, h - 1), (u, h)} <= reached, u
    if w == 8:
        g = SE.group_sizes()["ec_row"]
        assert {(31, 128), (31, 129), (31, 255), (31, 256), (31, 128 + g), (31, 129 + g), (0, g), (0, g + 1)} <= reached


# ---------------------------------------------------------------- the fixture
def _py_oracle(it):
    return corda.verify_item(it["scheme"], it["key_fmt"], bytes.fromhex(it["key"]), bytes.fromhex(it["sig"]),
                             bytes.fromhex(it["msg"]), corda.MODE_ISVALID)


def test_fixture_is_valid_under_the_python_oracle():
    """Every constructed item (an ECDSA target, or S < L) is VALID under oracle.corda.verify_item, and
    every other item has the verdict the fixture records."""
    with _pool(WORKERS) as ex:
        got = list(ex.map(_py_oracle, ITEMS(), chunksize=8))
    n_valid = 0
    for it, st in zip(ITEMS(), got):
        assert corda.STATUS_NAMES[st] == it["expect_isvalid"] == it["expect"], it["note"]
        if _constructed_valid(it):
            assert st == corda.VALID, it["note"]
            n_valid += 1
    assert n_valid >= len(ITEMS()) - len(SE.ed_s_above_l())
    assert any(it["expect"] == "INVALID" for it in ITEMS()) and any(
        it["expect"] == "VALID" and it["class"] == "ed_s_above_l" for it in ITEMS())


def test_c_oracle_agrees_with_the_fixture():
    b, exp, exp_iv = golden_io.sig_batch(ITEMS())
    assert np.array_equal(c_oracle.verify_batch(b, B.MODE_DOVERIFY, WORKERS), exp)
    assert np.array_equal(c_oracle.verify_batch(b, B.MODE_ISVALID, WORKERS), exp_iv)


def test_fixture_is_what_the_generator_writes():
    """The items are the generator's list (class, scheme, note, in order), and a seeded sample of
    every class, stored or made on demand, regenerates to the same bytes with the Python oracle's
    verdict."""
    specs = GEN.specs()
    assert len(specs) == len(ITEMS())
    for sp, it in zip(specs, ITEMS()):
        assert (sp["class"], sp["scheme"], sp["note"]) == (it["class"], it["scheme"], it["note"])
    rng = random.Random(0xED6E)
    per_class = {}
    for i, it in enumerate(ITEMS()):
        per_class.setdefault((it["class"], it["scheme"]), []).append(i)
    for _, idx in sorted(per_class.items()):
        for i in rng.sample(idx, 5):
            assert GEN.make_item(specs[i], i) == ITEMS()[i], ITEMS()[i]["note"]
    # one key for every Ed25519 item, one key per ECDSA item
    assert {it["key"] for it in ITEMS() if it["scheme"] == 4} == {SE.ED_IDENTITY_KEY.hex()}
    ec_keys = [it["key"] for it in ITEMS() if it["scheme"] != 4]
    assert len(set(ec_keys)) == len(ec_keys)
    # the file holds exactly the items the generator's rule stores, and stays under the 300 KB set for it
    assert STORED == [it for sp, it in zip(specs, ITEMS()) if GEN.in_fixture(sp)]
    assert os.path.getsize(os.path.join(golden_io.GOLDEN, "scalar_edges.json")) < 300 * 1000


# ---------------------------------------------------------------- host lane build
# Every helper takes every item of its scheme: the keys are raw (32 / 64 bytes), the Ed25519
# signatures 64 bytes. An item a helper could not take would be named here with the rule.
HELPER_EXCLUDES = {}
ED_HELPERS = [("t_ed_verify_w", 4), ("t_ed_verify_w", 6), ("t_ed_verify_wb", None), ("t_ed_verify_wb_signed", None),
              ("t_ed_verify_wide", None)]
EC_HELPERS = ["t_ecdsa_verify_rows", "t_ecdsa_verify_wide"]
VARIANT_DEFS = {24: ["-DED_WIDE_BW=24", "-DEC_WIDE_GW=24"], 22: ["-DED_WIDE_BW=22", "-DEC_WIDE_GW=22"]}  # csrc/Makefile
_LIBS = {}


def _lane_lib(bits):
    """The host build at fixed-base radix 2^bits (26: hostk's own; 24 / 22: the Makefile's variant
    defines, built by hostk.build_so under the name CG_HOSTK_DEFS would give it)."""
    if bits not in _LIBS:
        if bits == 26:
            lib = hostk.lib()
        else:
            defs = VARIANT_DEFS[bits]
            so = os.path.join(HERE, "native", "libhostkernels_%s.so" % "_".join(d.lstrip("-D") for d in defs))
            keep = hostk.DEFS, hostk.SO
            hostk.DEFS, hostk.SO = defs, so
            try:
                hostk.build_so()
            finally:
                hostk.DEFS, hostk.SO = keep
            lib = ctypes.CDLL(so)
        assert lib.t_wide_radix() == bits
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        lib.t_ed_verify_w.argtypes = [i32, vp, vp, vp, u64]
        for fn in ("t_ed_verify_wb", "t_ed_verify_wb_signed", "t_ed_verify_wide"):
            getattr(lib, fn).argtypes = [vp, vp, vp, u64, vp]
        lib.t_ecdsa_verify_rows.argtypes = [i32, vp, u64, u64, u32, u32, u64, u32, u64, u64]
        lib.t_ecdsa_verify_wide.argtypes = [i32, vp, u64, u64, u32, u32, u64, u32, u64, u64, vp]
        _LIBS[bits] = lib
    return _LIBS[bits]


def _lane_verdict(lib, helper, it):
    key, sig, msg = bytes.fromhex(it["key"]), bytes.fromhex(it["sig"]), bytes.fromhex(it["msg"])
    if it["scheme"] == 4:
        fn, w = helper
        m = np.frombuffer(msg + bytes(8), dtype=np.uint8).copy()
        args = (ptr(words(key)), ptr(words(sig)), ptr(m), len(msg))
        st = getattr(lib, fn)(w, *args) if w is not None else getattr(lib, fn)(*args, None)
        return ED_NAMES[st]
    arena = np.frombuffer(key + sig + msg + bytes(8), dtype=np.uint8).copy()
    args = (it["scheme"], ptr(arena), len(key) + len(sig) + len(msg), 0, len(key), it["key_fmt"], len(key), len(sig),
            len(key) + len(sig), len(msg))
    st = lib.t_ecdsa_verify_wide(*args, None) if helper == "t_ecdsa_verify_wide" else getattr(lib, helper)(*args)
    return EC_NAMES[st]


def _lane_chunk(job):
    bits, helper, part = job
    lib = _lane_lib(bits)
    return [(i, _lane_verdict(lib, helper, it)) for i, it in part]


def _run_lanes(bits, helper, idx):
    """Verdicts of items `idx` under one helper, over worker processes (a violated limb bound aborts
    the worker, which fails the test)."""
    _lane_lib(bits)  # built once, before the workers start
    chunks = [(bits, helper, [(i, ITEMS()[i]) for i in idx[k::WORKERS]]) for k in range(WORKERS) if idx[k::WORKERS]]
    with _pool(len(chunks)) as ex:
        got = dict(p for part in ex.map(_lane_chunk, chunks) for p in part)
    wrong = [(ITEMS()[i]["note"], got[i], ITEMS()[i]["expect_isvalid"]) for i in idx if got[i] != ITEMS()[i]["expect_isvalid"]]
    assert not wrong, (bits, helper, len(wrong), wrong[:8])
    return len(got)


def _of_scheme(ed):
    return [i for i, it in enumerate(ITEMS()) if (it["scheme"] == 4) == ed]


@pytest.mark.parametrize("helper", ED_HELPERS, ids=lambda h: h[0] + ("" if h[1] is None else str(h[1])))
def test_ed25519_lanes_on_every_item(helper):
    idx = [i for i in _of_scheme(True) if (helper[0], i) not in HELPER_EXCLUDES]
    assert _run_lanes(26, helper, idx) == len(idx) == len(_of_scheme(True))


@pytest.mark.parametrize("helper", EC_HELPERS)
def test_ecdsa_lanes_on_every_item(helper):
    idx = [i for i in _of_scheme(False) if (helper, i) not in HELPER_EXCLUDES]
    assert _run_lanes(26, helper, idx) == len(idx) == len(_of_scheme(False))


def test_no_item_is_excluded_from_every_helper():
    assert all(ITEMS()[i]["key_fmt"] == B.KEY_RAW for i in range(len(ITEMS())))
    for i, it in enumerate(ITEMS()):
        helpers = [h[0] for h in ED_HELPERS] if it["scheme"] == 4 else EC_HELPERS
        assert any((h, i) not in HELPER_EXCLUDES for h in helpers), it["note"]
        assert len(bytes.fromhex(it["key"])) == (32 if it["scheme"] == 4 else 64)


@pytest.mark.parametrize("bits", [24, 22])
def test_budgeted_radix_lanes_on_their_targets(bits):
    """The host build with the Makefile's radix-2^24 / 2^22 defines: that radix's S and u1 targets
    (and the scalars above L) through the wide and the full-table ladders, which both add the fixed
    base from the wide table of that radix."""
    mine = [i for i, it in enumerate(ITEMS()) if f"w{bits} " in it["note"] or it["class"] == "ed_s_above_l"]
    ed = [i for i in mine if ITEMS()[i]["scheme"] == 4]
    ec = [i for i in mine if ITEMS()[i]["class"] == "ec_u1"]
    d = SE.ed_digits(bits)
    assert len(ed) > 8 * (d - 1) and len(ec) > 2 * 8 * (d - 1)
    for helper in (("t_ed_verify_wide", None), ("t_ed_verify_wb", None), ("t_ed_verify_wb_signed", None)):
        _run_lanes(bits, helper, ed)
    for helper in EC_HELPERS:
        _run_lanes(bits, helper, ec)
