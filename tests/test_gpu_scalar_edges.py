"""GPU tests on crafted ladder scalars (tests/scalar_edges.py; items from tests/golden/scalar_edges.json
and, for the per-row targets, made on demand by tests/golden/gen_scalar_edges.py): the
first, last and group-boundary entries of every fixed-base and per-key table row, the recoding
carries and the top of the scalar range, which the random scalars of every other test reach with
probability 2^-W per row.

  * the wide tables at each fixed-base radix (26: the session context; 24 and 22: budgeted contexts
    as tests/test_gpu_tables.py opens them), every key hot enough for wide tables;
  * the same items under key-table entries with 1, 12, 160 and 4 x the wide threshold uses in one
    call: row-0, quarter, full and wide tables, whose verdicts must be equal ("the mode changes only
    speed, never a verdict", keyws.h), and with every key prepared in full;
  * the Ed25519 items through the transaction-signature entry points.

The reference is the C oracle on the distinct items, broadcast to their copies (a copy is another
item-table entry over the same bytes). tests/test_scalar_edges.py runs the same items through the
host build of the lane code."""
import os
import sys

import numpy as np
import pytest

import golden_io
import scalar_edges as SE
import txsig_util
from corda_amd import batch as B
from oracle import c_oracle

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(golden_io.GOLDEN))
import gen_scalar_edges as GEN  # noqa: E402

ITEMS = GEN.all_items  # the stored items and the per-row ones the generator makes (once per process)
WIDE_MIN = {4: SE.header_int("KEY_WIDE_MIN_USES_ED", "keyws.h"), 3: SE.header_int("KEY_WIDE_MIN_USES_EC", "keyws.h"),
            2: SE.header_int("KEY_WIDE_MIN_USES_EC", "keyws.h")}
KEY_WIDE_MAX = SE.header_int("KEY_WIDE_MAX", "keyws.h")
# the one-shot entry points estimate a key's uses from a hashed 1-in-KEY_USES_SAMPLE sample: this
# factor keeps the estimate clear of the threshold
CLEAR = SE.header_int("KEY_USES_SAMPLE", "keyws.h")
MODES = (B.MODE_DOVERIFY, B.MODE_ISVALID)


def _constructed_valid(it):
    return it["scheme"] != 4 or int.from_bytes(bytes.fromhex(it["sig"])[32:], "little") < SE.L


def _of_radix(bits, cls):
    return [it for it in ITEMS() if it["class"] == cls and f"w{bits} " in it["note"]]


def _expand(distinct, entries, seed):
    """A batch over `distinct` fixture items: one key-table entry per element of `entries` (an array
    of positions in `distinct`, all under the same key bytes; an entry aliases the key's bytes in the
    arena), one item per listed position, shuffled. Returns (batch, position of each item, entry of
    each item, the batch of the distinct items)."""
    b0, _, _ = golden_io.sig_batch(distinct)
    first = np.array([int(e[0]) for e in entries])
    assert all(len({distinct[int(p)]["key"] for p in np.unique(e)}) == 1 for e in entries[:64])
    keys = b0.keys[b0.items["key_idx"][first]].copy()
    pos = np.concatenate(entries)
    ent = np.repeat(np.arange(len(entries), dtype=np.uint32), [len(e) for e in entries])
    order = np.random.default_rng(seed).permutation(pos.size)
    pos, ent = pos[order], ent[order]
    items = b0.items[pos].copy()
    items["key_idx"] = ent
    return B.Batch(keys, items, b0.arena), pos, ent, b0


def _device_forms(eng, b, mode, prepared=False):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    kd, idd, ad = up(b.keys), up(b.items), up(b.arena)
    sd = torch.full((b.n,), 255, dtype=torch.uint8, device=dev)
    if prepared:
        eng.prepare_keys_device(kd.data_ptr(), len(b.keys), ad.data_ptr(), b.arena.size)
        eng.verify_items_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size,
                                sd.data_ptr(), mode)
    else:
        eng.verify_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size, sd.data_ptr(),
                          mode)
    torch.cuda.synchronize()
    return sd.cpu().numpy()


def _same(st, ref, pos, distinct, what):
    bad = np.flatnonzero(st != ref)
    assert bad.size == 0, (what, bad.size, [(distinct[int(pos[j])]["note"], int(st[j]), int(ref[j])) for j in bad[:6]])


# ---------------------------------------------------------------- wide tables, per radix
def _wide_tables(eng, bits):
    assert eng.info()["fixed_base_bits"] == bits
    ed = _of_radix(bits, "ed_s") + [it for it in ITEMS() if it["class"] == "ed_s_above_l"]
    ec = _of_radix(bits, "ec_u1") + [it for it in ITEMS() if it["class"] == "ec_u2"]
    d = SE.ed_digits(bits)
    assert len(ed) > 8 * (d - 1) and len(ec) > 2 * 8 * (d - 1) + 1000
    distinct = ed + ec
    ed_uses = max(len(ed), CLEAR * WIDE_MIN[4])  # one identity-key entry, padded with its own items
    entries = [np.resize(np.arange(len(ed)), ed_uses)]
    entries += [np.full(CLEAR * WIDE_MIN[3], len(ed) + j) for j in range(len(ec))]
    for scheme in (2, 3):
        assert sum(it["scheme"] == scheme for it in ec) < KEY_WIDE_MAX
    b, pos, _, b0 = _expand(distinct, entries, 1000 + bits)
    valid = np.array([_constructed_valid(it) for it in distinct])[pos]
    for mode in MODES:
        ref = c_oracle.verify_batch(b0, mode, 16)[pos]
        assert np.all(ref[valid] == B.VALID) and np.any(ref == B.INVALID)
        _same(eng.verify(b, mode), ref, pos, distinct, f"radix 2^{bits} verify, mode {mode}")
        _same(_device_forms(eng, b, mode), ref, pos, distinct, f"radix 2^{bits} verify_device, mode {mode}")


def test_wide_tables_at_the_default_radix(engine):
    _wide_tables(engine, 26)


@pytest.fixture(scope="module", params=[24, 22])
def budgeted(request, engine):  # `engine` first, as tests/test_gpu_rsa.py; a param's context closes before the next opens
    from corda_amd import _lib
    from corda_amd.engine import Engine
    e = Engine(0, table_bytes_max=_lib.lib().cg_table_bytes(request.param))
    yield request.param, e
    e.close()


def test_wide_tables_at_the_budgeted_radixes(budgeted):
    bits, eng = budgeted
    _wide_tables(eng, bits)


# ---------------------------------------------------------------- every table mode in one call
def test_four_table_modes_give_one_verdict(engine):
    """The radix-2^10 and per-key-row targets under key-table entries with 1, 12, 160 and 4 x the wide
    threshold uses (row 0, quarter, full, wide): the oracle's verdicts, the same verdict for an item
    under every entry, every ladder stage launched, and the same again with every key built in full
    (cg_prepare_keys_device + cg_verify_items_device)."""
    from corda_amd import _lib
    from corda_amd.engine import Engine
    ed = _of_radix(10, "ed_s") + [it for it in ITEMS() if it["class"] == "ed_s_above_l"]
    ec = _of_radix(10, "ec_u1") + [it for it in ITEMS() if it["class"] == "ec_u2"]
    distinct = ed + ec
    entries, uses = [], []
    for c in (1, 12, 160, None):
        n_ed = c or CLEAR * WIDE_MIN[4]
        k = max(4, -(-len(ed) // n_ed))  # at least 4 entries, and room for every target
        entries += list(np.resize(np.arange(len(ed)), k * n_ed).reshape(k, n_ed))
        n_ec = c or CLEAR * WIDE_MIN[3]
        entries += [np.full(n_ec, len(ed) + j) for j in range(len(ec))]
        uses += [c or 0] * (k + len(ec))
    b, pos, ent, b0 = _expand(distinct, entries, 77)
    uses = np.array(uses)[ent]
    for c in (1, 12, 160, 0):  # every target under every count
        assert np.unique(pos[uses == c]).size == len(distinct), c
    for scheme in (4, 3, 2):
        fam = np.array([it["scheme"] == scheme for it in distinct])[pos]
        assert all(np.unique(ent[fam & (uses == c)]).size >= 4 for c in (1, 12, 160, 0)), scheme
    valid = np.array([_constructed_valid(it) for it in distinct])[pos]
    stages = ["ed_ladder_row0", "ed_ladder", "ed_ladder_wide", "r1_ladder_row0", "r1_ladder", "r1_ladder_wide",
              "k1_ladder_row0", "k1_ladder", "k1_ladder_wide"]
    with Engine(0, stage_timing=True, table_bytes_max=_lib.lib().cg_table_bytes(22)) as eng:
        for mode in MODES:
            ref = c_oracle.verify_batch(b0, mode, 16)[pos]
            assert np.all(ref[valid] == B.VALID)
            eng.stage_times()
            st = eng.verify(b, mode)
            launched = eng.stage_times()
            assert all(launched[s][1] > 0 for s in stages), launched
            _same(st, ref, pos, distinct, f"four modes, mode {mode}")
            lo = np.full(len(distinct), 255, np.uint8)
            hi = np.zeros(len(distinct), np.uint8)
            np.minimum.at(lo, pos, st)
            np.maximum.at(hi, pos, st)
            differ = np.flatnonzero(lo != hi)
            assert differ.size == 0, [distinct[int(j)]["note"] for j in differ[:6]]
            _same(_device_forms(eng, b, mode), ref, pos, distinct, f"four modes verify_device, mode {mode}")
            _same(_device_forms(eng, b, mode, prepared=True), ref, pos, distinct, f"every key in full, mode {mode}")


# ---------------------------------------------------------------- transaction signatures
def test_tx_signature_path_on_the_ed25519_targets(engine):
    """The SignableData splice fixes the message, and an identity-key signature depends on S alone:
    every Ed25519 item through cg_verify_tx_signatures and the packed form at the default radix,
    under one entry hot enough for wide tables and one with each item once, against the C oracle on
    the materialised messages."""
    from corda_amd import signable
    ed = [it for it in ITEMS() if it["scheme"] == 4]
    rng = np.random.default_rng(31)
    bld = B.TxSigBuilder()
    tmpl = bld.template(*signable.template(1, 4))
    key = bld.key(4, 0, SE.ED_IDENTITY_KEY)
    tx = [bld.tx_id(rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in range(16)]
    for j, it in enumerate(ed):
        bld.add_signature(key, tx[j % 16], tmpl, bytes.fromhex(it["sig"]))
    tb0 = bld.build()
    hot = np.resize(np.arange(len(ed)), CLEAR * WIDE_MIN[4])
    pos = np.concatenate([hot, np.arange(len(ed))])
    ent = np.concatenate([np.zeros(hot.size, np.uint32), np.ones(len(ed), np.uint32)])
    order = rng.permutation(pos.size)
    pos, ent = pos[order], ent[order]
    sigs = tb0.sigs[pos].copy()
    sigs["key_idx"] = ent
    tb = B.TxSigBatch(np.concatenate([tb0.keys, tb0.keys]), tb0.ids, sigs, tb0.tmpls, tb0.arena)
    valid = np.array([_constructed_valid(it) for it in ed])[pos]
    pb = tb.packed()
    for mode in MODES:
        ref = c_oracle.verify_batch(txsig_util.to_message_batch(tb0), mode, 16)[pos]
        assert np.all(ref[valid] == B.VALID) and np.any(ref == B.INVALID)
        _same(engine.verify_tx_signatures(tb, mode), ref, pos, ed, f"verify_tx_signatures, mode {mode}")
        _same(engine.verify_tx_signatures_packed(pb, mode), ref, pos, ed, f"packed, mode {mode}")
