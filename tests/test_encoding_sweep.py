"""The encoding sweeps (tests/encoding_sweep.py, expected statuses in
tests/golden/encoding_sweep.json from the Python oracle) on the CPU: the rebuilt sweeps are the
recorded ones, the C oracle gives the recorded status on every item in both modes, the host build of
the lane code (ecdsa.h der_sig through DerArena, the key decoders of ecdsa.h / ed25519.h) gives it
under isValid semantics, and the sweeps hold what they are meant to hold. A GPU mismatch in
tests/test_gpu_encoding_sweep.py is debugged here.

The precedence matrix (sweep e), the same for schemes 2, 3 and 4; statuses doVerify / isValid:

  key                 signature   message   doVerify        isValid
  decodable           good        message   VALID           VALID
  decodable           wrong       message   INVALID         INVALID
  decodable           malformed   message   SIG_MALFORMED   SIG_MALFORMED
  decodable           empty       message   EMPTY           SIG_MALFORMED
  decodable           good        empty     EMPTY           VALID
  decodable           wrong       empty     EMPTY           INVALID
  decodable           malformed   empty     EMPTY           SIG_MALFORMED
  decodable           empty       empty     EMPTY           SIG_MALFORMED
  undecodable         any         any       KEY_INVALID     KEY_INVALID
  unsupported scheme  any         any       UNSUPPORTED     UNSUPPORTED
  key_idx past        any         any       NOT_RUN         NOT_RUN
"""
import ctypes
import json
import multiprocessing
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import encoding_sweep as ES
import golden_io
import hostk
import txsig_util
from corda_amd import batch as B
from hostk import ptr, words
from oracle import c_oracle, corda

with open(os.path.join(golden_io.GOLDEN, "encoding_sweep.json")) as _f:
    FIX = json.load(_f)
EXPECT, META = FIX["expect"], FIX["meta"]
MODES = (("doverify", B.MODE_DOVERIFY), ("isvalid", B.MODE_ISVALID))
WORKERS = min(16, len(os.sched_getaffinity(0)))
# Every item of every sweep goes through the host lanes (about 40 s for sweep a on 8 cores, less for
# the others): the stride over the key mutations that are neither a truncation, an extension nor at
# a full_at position is 1. A larger stride must keep every status class (asserted in _lane_subset).
KEY_STRIDE = 1


def _want(name, mode="isvalid"):
    return ES.status_array(EXPECT[name][mode])


def _names(st):
    return {corda.STATUS_NAMES[int(s)]: int(n) for s, n in zip(*np.unique(st, return_counts=True))}


def _wrong(items, got, want):
    bad = np.flatnonzero(np.asarray(got) != want)
    return [(items[int(j)].note, int(got[j]), int(want[j])) for j in bad[:8]], bad.size


# ---------------------------------------------------------------- the fixture
def test_sweeps_are_the_recorded_ones():
    assert FIX["base"] == ES.base_record()
    for name in "abcde":
        items = ES.sweep(name)
        assert len(items) == META[name]["items"] == len(EXPECT[name]["doverify"]) == len(EXPECT[name]["isvalid"]), name
        for mode, _ in MODES:
            assert _names(_want(name, mode)) == META[name][mode], (name, mode)
        assert len({it.note for it in items}) == len(items), name
    assert os.path.getsize(os.path.join(golden_io.GOLDEN, "encoding_sweep.json")) < 200 * 1000


def test_python_oracle_on_the_base_vectors_and_a_sample():
    """The generator ran oracle.corda.verify_item over every item (minutes); here every 97th item."""
    for name in "abcde":
        items = ES.sweep(name)
        for mode_name, mode in MODES:
            want = _want(name, mode_name)
            for j in range(0, len(items), 97):
                it = items[j]
                st = corda.NOT_RUN if it.past else corda.verify_item(it.scheme, it.fmt, it.key, it.sig, it.msg, mode)
                assert st == want[j], (it.note, mode_name)


@pytest.mark.parametrize("mode_name,mode", MODES)
def test_c_oracle_agrees_on_every_item(mode_name, mode):
    ab = ES.sweep("a") + ES.sweep("b")
    tb = ES.txsig_batch(ab)
    got = c_oracle.verify_batch(txsig_util.to_message_batch(tb), mode, WORKERS)
    want = np.concatenate([_want("a", mode_name), _want("b", mode_name)])
    wrong, n = _wrong(ab, got, want)
    assert n == 0, (n, wrong)
    cde = ES.sweep("c") + ES.sweep("d") + ES.sweep("e")
    got = c_oracle.verify_batch(ES.key_batch(cde), mode, WORKERS)
    want = np.concatenate([_want(s, mode_name) for s in "cde"])
    wrong, n = _wrong(cde, got, want)
    assert n == 0, (n, wrong)


# ---------------------------------------------------------------- what the sweeps hold
def test_sweep_a_holds_its_cases():
    items, st = ES.sweep("a"), _want("a")
    n = _names(st)
    assert n["SIG_MALFORMED"] >= 600 and n["INVALID"] >= 2500
    valid = [items[int(j)].note for j in np.flatnonzero(st == B.VALID)]
    assert valid == [f"{b}: base" for b in ES.BASE_NAMES[:4]]
    parsed = {len(it.sig) for it, s in zip(items, st) if s != B.SIG_MALFORMED}
    assert {80, 81} <= parsed                       # both sides of EC_SIG_STAGED (verify_ec.hip)
    assert any(128 <= ln <= 255 for ln in parsed)   # SEQUENCE length 81 xx
    assert any(256 <= ln < B.SIG_LEN_MAX for ln in parsed)  # 82 xx xx
    assert B.SIG_LEN_MAX in parsed and len(items[-1].sig) == B.SIG_LEN_MAX and st[-1] == B.INVALID
    # a well-formed long encoding is never malformed
    long_ = [j for j, it in enumerate(items) if re.search(r"(positive|negative), \d+ bytes$", it.note)]
    assert len(long_) == 4 * 3 * len(ES.LONG_E) and all(st[j] == B.INVALID for j in long_)
    wrap = [j for j, it in enumerate(items) if " length 84 " in it.note]
    assert len(wrap) == 4 * 2 * len(ES.WRAP_LENS) and all(st[j] == B.SIG_MALFORMED for j in wrap)
    # doVerify differs only on the empty signature
    dv = _want("a", "doverify")
    assert [items[int(j)].note.split(": ")[1] for j in np.flatnonzero(dv != st)] == ["cut to 0"] * 4


def test_sweep_b_holds_its_cases():
    items, st = ES.sweep("b"), _want("b")
    assert [items[int(j)].note for j in np.flatnonzero(st == B.VALID)] == ["ed: base"]
    for j, it in enumerate(items):
        assert (st[j] == B.SIG_MALFORMED) == (len(it.sig) != 64), it.note
    for pos in (31, 63):  # every top byte of R and of S
        assert sum(f"byte {pos} = " in it.note for it in items) == 255


# The mutated keys that stay VALID (all in sweep d: an Ed25519 point has one accepted encoding unless
# y < 19, and the base key's y is not): per curve
#   sec1 04: byte 0 = 06|07 of y's parity   (hybrid form of the same point)
#   sec1 hybrid: byte 0 = 04                (uncompressed form of the same point)
#   spki: the point tag 04 -> 06|07 of y's parity
def test_sweeps_c_and_d_hold_their_cases():
    for name in "cd":
        n = _names(_want(name))
        assert n["KEY_INVALID"] >= 1000 and n["INVALID"] >= 500, (name, n)
        assert EXPECT[name]["doverify"] == EXPECT[name]["isvalid"]  # no empty signature or message
    items, st = ES.sweep("c"), _want("c")
    assert all(items[int(j)].note.endswith(": base") for j in np.flatnonzero(st == B.VALID))
    items, st = ES.sweep("d"), _want("d")
    stay = [items[int(j)].note for j in np.flatnonzero(st == B.VALID) if not items[int(j)].note.endswith(": base")]
    want = []
    for scheme, c in ((2, "k1"), (3, "r1")):
        hyb = 6 | (ES.base()[c + "_low"]["key"][63] & 1)
        tag = len(ES.ecdsa_bc.spki_prefix(scheme, 65))
        want += [f"{c} sec1 04: byte 0 = {hyb:02x}", f"{c} sec1 hybrid: byte 0 = 04", f"{c} spki: byte {tag} = {hyb:02x}"]
    assert len(want) == 6 and [s.replace(ES.FULL_TAG, "") for s in stay] == want


def test_sweep_e_is_the_table_above():
    items = ES.sweep("e")
    rows = set()
    for line in __doc__.splitlines():
        m = re.match(r"  (decodable|undecodable|unsupported scheme|key_idx past)\s+(\w+)\s+(\w+)\s+(\w+)\s+(\w+)$", line)
        if m:
            rows.add(m.groups())
    assert len(rows) == 11
    for j, it in enumerate(items):
        m = re.match(r"scheme \d: (.+) key, (\w+) signature, (message|empty message)$", it.note)
        key, sig, msg = m.group(1), m.group(2), m.group(3).split()[0]
        got = tuple(corda.STATUS_NAMES[ES.STATUS_OF_DIGIT[EXPECT["e"][mode][j]]] for mode, _ in MODES)
        assert (key, sig, msg) + got in rows or (key, "any", "any") + got in rows, it.note
    assert len(items) == 3 * 4 * 4 * 2


# ---------------------------------------------------------------- host lane build
ST = {0: B.VALID, 1: B.INVALID, 2: B.SIG_MALFORMED, 3: B.KEY_INVALID}


def _lane_status(lib, it):
    """isValid status of one item from the host build of the lane code."""
    key, sig, msg = it.key, it.sig, it.msg
    if it.scheme != 4:
        arena = np.frombuffer(key + sig + msg + bytes(8), dtype=np.uint8).copy()
        return ST[lib.t_ecdsa_verify_rows(it.scheme, ptr(arena), len(key) + len(sig) + len(msg), 0, len(key), it.fmt, len(key),
                                          len(sig), len(key) + len(sig), len(msg))]
    # The two byte-level rules in front of the Ed25519 lane code live in the kernels, not the headers
    # (verify_ed.hip ed_key_locate: 32 raw bytes, or the 44 / 46-byte SPKI with its exact prefix; a
    # signature is 64 bytes): restated here, the point decode and the verification are the lanes'.
    if it.fmt == B.KEY_SPKI and len(key) == 44 and key[:12] == corda.ED25519_SPKI_PREFIX:
        a = key[12:]
    elif it.fmt == B.KEY_SPKI and len(key) == 46 and key[:14] == corda.ED25519_SPKI_PREFIX_NULL:
        a = key[14:]
    elif it.fmt == B.KEY_RAW and len(key) == 32:
        a = key
    else:
        return B.KEY_INVALID
    if len(sig) != 64:
        out = np.zeros(8, np.uint32)
        return B.KEY_INVALID if lib.t_ed_keyprep(ptr(words(a)), ptr(out)) else B.SIG_MALFORMED
    m = np.frombuffer(msg + bytes(8), dtype=np.uint8).copy()
    return ST[lib.t_ed_verify(ptr(words(a)), ptr(words(sig)), ptr(m), len(msg))]


def _lane_chunk(part):
    lib = hostk.lib()
    lib.t_ed_keyprep.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return [(j, _lane_status(lib, it)) for j, it in part]


def _lane_subset(name):
    """Positions of the sweep's items that go through the lanes: all of a and b; of c and d every
    base, truncation, extension and full_at mutation and every KEY_STRIDE-th of the rest."""
    items = ES.sweep(name)
    if name in "ab" or KEY_STRIDE == 1:
        return list(range(len(items)))
    always = re.compile(r": (base|cut to \d+|extended by \d+)$")
    rest = [j for j, it in enumerate(items) if not (always.search(it.note) or it.note.endswith(ES.FULL_TAG))]
    keep = sorted(set(range(len(items))) - set(rest) | set(rest[::KEY_STRIDE]))
    assert set(_want(name)[keep]) == set(_want(name)), name  # no status class vanishes
    return keep


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_host_lanes_agree(name):
    items, want = ES.sweep(name), _want(name)
    idx = _lane_subset(name)
    hostk.lib()  # built once, before the workers start
    chunks = [[(j, items[j]) for j in idx[k::4 * WORKERS]] for k in range(4 * WORKERS)]
    # spawned: a fork can fail once the host build has reserved its multi-gigabyte tables
    with ProcessPoolExecutor(WORKERS, mp_context=multiprocessing.get_context("spawn")) as ex:
        got = dict(p for part in ex.map(_lane_chunk, [c for c in chunks if c]) for p in part)
    assert len(got) == len(idx)
    wrong = [(items[j].note, got[j], int(want[j])) for j in idx if got[j] != want[j]]
    assert not wrong, (len(wrong), wrong[:8])
