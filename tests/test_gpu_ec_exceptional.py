"""GPU tests on the ECDSA items of tests/golden/ec_exceptional.json (tests/ec_exceptional.py,
tests/golden/gen_ec_exceptional.py): signatures whose fixed-base additions double the accumulator,
cancel it to infinity in mid-ladder (the next addition reloads), or end the ladder at infinity, and
honest signatures that are false positives of the signed-limb ladder's limb-0 filter (ec9.h). Random
scalars reach the first three with probability ~2^-256, and the last for secp256r1 about once in
10^5 wide items. tests/test_ec_exceptional.py proves on the host build of the same lane code, with
counters, that each item does what its note says; here the device build runs them:

  * every item under key-table entries with 1, 12, 160 and 4 x the wide threshold uses in one call
    (row-0, quarter, full and wide ladders: jac_madd_w in the first three, jac_madd9's divergent
    exact path in the last), at each fixed-base radix: an item collides as its note says at the
    radix it was made for, and most are controls at the others;
  * the filter items under one hot key per curve beside two thousand ordinary signatures of the
    same key and synthetic items of other hot keys, so that lanes on the exact path sit beside
    lanes on the fast path.

The reference is the C oracle on the distinct items, broadcast to their copies."""
import sys

import numpy as np
import pytest

import golden_io
from corda_amd import batch as B
from oracle import c_oracle
from test_gpu_scalar_edges import CLEAR, KEY_WIDE_MAX, MODES, WIDE_MIN, _device_forms, _expand, _same

pytestmark = pytest.mark.gpu

sys.path.insert(0, golden_io.GOLDEN)
import gen_ec_exceptional as GEN  # noqa: E402

ITEMS = golden_io.load("ec_exceptional.json")
USES = (1, 12, 160, CLEAR * WIDE_MIN[3])  # row 0, quarter, full, wide
EC_STAGES = ["r1_ladder_row0", "r1_ladder", "r1_ladder_wide", "k1_ladder_row0", "k1_ladder", "k1_ladder_wide"]


def _every_item_under_every_mode(eng, bits, stages=False):
    assert eng.info()["fixed_base_bits"] == bits
    mine = [it for it in ITEMS if it["note"].startswith(f"w{bits} ")]
    assert len(mine) == 2 * 14 and len(ITEMS) >= 3 * len(mine)  # this radix's items; the others are mostly controls
    entries = [np.full(c, j) for c in USES for j in range(len(ITEMS))]
    assert sum(it["scheme"] == 3 for it in ITEMS) < KEY_WIDE_MAX
    b, pos, ent, b0 = _expand(ITEMS, entries, 4100 + bits)
    uses = np.repeat(USES, len(ITEMS))[ent]
    for c in USES:
        assert np.unique(pos[uses == c]).size == len(ITEMS), c
    want = np.array([B.STATUS_BY_NAME[it["expect"]] for it in ITEMS], dtype=np.uint8)
    last = np.array([it["class"] == "neg last" for it in ITEMS])
    assert np.all(want[last] == B.INVALID) and np.all(want[~last] == B.VALID) and last.sum() == 6
    for mode in MODES:
        ref0 = c_oracle.verify_batch(b0, mode, 16)
        assert np.array_equal(ref0, want)  # VALID as constructed; neg@last INVALID
        ref = ref0[pos]
        if stages:
            eng.stage_times()
        st = eng.verify(b, mode)
        if stages:
            launched = eng.stage_times()
            assert all(launched[s][1] > 0 for s in EC_STAGES), launched
        _same(st, ref, pos, ITEMS, f"radix 2^{bits} verify, mode {mode}")
        lo = np.full(len(ITEMS), 255, np.uint8)
        hi = np.zeros(len(ITEMS), np.uint8)
        np.minimum.at(lo, pos, st)
        np.maximum.at(hi, pos, st)
        assert np.array_equal(lo, hi), [ITEMS[int(j)]["note"] for j in np.flatnonzero(lo != hi)[:6]]
        assert np.all(st[last[pos]] == B.INVALID) and np.all(st[~last[pos]] == B.VALID)
        _same(_device_forms(eng, b, mode), ref, pos, ITEMS, f"radix 2^{bits} verify_device, mode {mode}")
        _same(_device_forms(eng, b, mode, prepared=True), ref, pos, ITEMS, f"radix 2^{bits} every key in full, mode {mode}")


def test_every_table_mode_at_the_default_radix(engine):
    _every_item_under_every_mode(engine, 26)


@pytest.fixture(scope="module", params=[24, 22])
def budgeted(request, engine):  # `engine` first; a param's context closes before the next opens
    from corda_amd import _lib
    from corda_amd.engine import Engine
    # radix 2^22 with stage timing, as test_gpu_scalar_edges.test_four_table_modes_give_one_verdict opens it
    e = Engine(0, stage_timing=request.param == 22, table_bytes_max=_lib.lib().cg_table_bytes(request.param))
    yield request.param, e
    e.close()


def test_every_table_mode_at_the_budgeted_radixes(budgeted):
    """At radix 2^22 (a stage-timing context) also: all six ECDSA ladder stages launched."""
    bits, eng = budgeted
    _every_item_under_every_mode(eng, bits, stages=bits == 22)


def test_filter_items_beside_fast_path_lanes(engine):
    """The filter's false positives under wide tables at the default radix: per curve one entry of
    the filter key with every kept item 32 times among 2 000 ordinary signatures of that key
    (the generator's candidates 0 .. 1999: the same key, other messages), and 1 000 synthetic items
    of two other hot keys, shuffled: the C oracle's verdicts, and every filter item VALID."""
    from tools.workload import wl
    assert engine.info()["fixed_base_bits"] == 26
    specs = [sp for sp in GEN.specs() if sp["kind"] == "filter"]
    kept = [it for it in ITEMS if it["class"] in ("r1_filter", "k1_filter")]
    assert [sp["note"] for sp in specs] == [it["note"] for it in kept] and any(it["scheme"] == 2 for it in kept)
    distinct, entries = list(kept), []
    for scheme in (3, 2):
        hits = [j for j, it in enumerate(kept) if it["scheme"] == scheme]
        if not hits:
            continue
        cls = kept[hits[0]]["class"]
        first = len(distinct)
        for i in range(2000):
            sp = {"class": cls, "kind": "filter", "scheme": scheme, "w": 26, "note": f"{cls} ordinary {i}", "cand": i}
            distinct.append(GEN.make_item(sp, i, oracle=False))
        entry = np.concatenate([np.repeat(hits, 32), np.arange(first, first + 2000)])
        assert entry.size >= CLEAR * WIDE_MIN[scheme]
        entries.append(entry)
    bf, pos, _, b0 = _expand(distinct, entries, 77)
    r1, _ = wl.ecdsa_batch(1, 1000, n_keys=2, msg_len=64, corrupt_permille=100, seed=91, nthreads=16)
    k1, _ = wl.ecdsa_batch(0, 1000, n_keys=2, msg_len=64, corrupt_permille=100, seed=92, nthreads=16)
    b, perm = wl.concat([bf, r1, k1], shuffle_seed=93)
    is_kept = np.zeros(b.n, bool)
    is_kept[:bf.n] = pos < len(kept)
    is_kept = is_kept[perm]
    assert is_kept.sum() == 32 * len(kept)
    for mode in MODES:
        ref = np.concatenate([c_oracle.verify_batch(b0, mode, 16)[pos], c_oracle.verify_batch(r1, mode, 16),
                              c_oracle.verify_batch(k1, mode, 16)])[perm]
        assert np.all(ref[is_kept] == B.VALID) and np.any(ref == B.INVALID)
        for what, st in (("verify", engine.verify(b, mode)), ("verify_device", _device_forms(engine, b, mode))):
            bad = np.flatnonzero(st != ref)
            assert bad.size == 0, (what, mode, bad.size, bad[:8], st[bad[:8]], ref[bad[:8]])
            assert np.all(st[is_kept] == B.VALID)
