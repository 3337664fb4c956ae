"""GPU tests on the encoding sweeps (tests/encoding_sweep.py; expected statuses in
tests/golden/encoding_sweep.json from the Python oracle, which tests/test_encoding_sweep.py holds
against the C oracle and the host build of the lane code): every item's status is compared for
equality, in both modes.

  * sweeps a + b (ECDSA and Ed25519 signatures: every truncation, extension and byte mutation,
    well-formed DER of up to 65,535 bytes, 4-byte lengths near 2^32) as one tx-signature batch and
    as its message batch: the same signature bytes through k_ec_prep<C, false> and <C, true> on both
    sides of its 80-byte staging limit, and through both forms of the Ed25519 hash kernel;
  * sweep a relaid out (odd phases, poison between fields, the arena ending on the last byte of
    the 65,535-byte signature): the arena parser of signatures longer than 80 bytes;
  * sweeps c + d + e (mutated keys of every accepted form, the precedence matrix): one key-table
    entry per item, so the row-0 key preparation, and 40 further good items under each undamaged EC
    key, so those encodings are also decoded for the larger (quarter and full) table builds."""
import json
import os

import numpy as np
import pytest

import encoding_sweep as ES
import golden_io
import layout_util as LU
import txsig_util
from corda_amd import batch as B

pytestmark = pytest.mark.gpu

with open(os.path.join(golden_io.GOLDEN, "encoding_sweep.json")) as _f:
    EXPECT = json.load(_f)["expect"]
MODES = (("doverify", B.MODE_DOVERIFY), ("isvalid", B.MODE_ISVALID))
EXTRA_GOOD = 40  # further good items under each undamaged key encoding of sweep d


def _want(names, mode_name):
    return np.concatenate([ES.status_array(EXPECT[s][mode_name]) for s in names])


def _items(names):
    """The items of the sweeps `names`, each note led by its sweep's letter."""
    return [it._replace(note=f"sweep {s}, {it.note}") for s in names for it in ES.sweep(s)]


def _same(st, want, items, what):
    """`items[j]` names sweep and mutation of status j (statuses past len(items) are the extra good items)."""
    bad = np.flatnonzero(st != want)
    note = lambda j: items[j].note if j < len(items) else "extra good item %d" % (j - len(items))  # noqa: E731
    assert bad.size == 0, (what, f"{bad.size} of {st.size} differ",
                           [(note(int(j)), "got", int(st[j]), "want", int(want[j])) for j in bad[:8]])


def _device(eng, b, mode):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    kd, idd, ad = up(b.keys), up(b.items), up(b.arena)
    sd = torch.full((b.n,), 255, dtype=torch.uint8, device=dev)
    eng.verify_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size, sd.data_ptr(), mode)
    torch.cuda.synchronize()
    return sd.cpu().numpy()


@pytest.fixture(scope="module")
def signatures():
    """Sweeps a + b: (items, tx-signature batch, its message batch)."""
    items = _items("ab")
    tb = ES.txsig_batch(items)
    mb = txsig_util.to_message_batch(tb)
    assert tb.n == mb.n == len(items) and int(tb.sigs["sig_len"].max()) == B.SIG_LEN_MAX
    return items, tb, mb


@pytest.fixture(scope="module")
def keys():
    """Sweeps c + d + e and the extra good items: (items, batch, expected per mode)."""
    items = _items("cde")
    base = ES.d_base_keys()
    assert len(base) == 12
    b = ES.key_batch(items, extra=[k + (EXTRA_GOOD,) for k in base])
    assert b.n == len(items) + 12 * EXTRA_GOOD
    # one key-table entry per item but for the mutations that meet in the same bytes and sweep e's few keys
    assert len(b.keys) > 0.95 * len(items)
    want = {m: np.concatenate([_want("cde", m), np.full(12 * EXTRA_GOOD, B.VALID, np.uint8)]) for m, _ in MODES}
    return items, b, want


@pytest.mark.parametrize("mode_name,mode", MODES)
def test_signature_sweeps_as_messages(engine, signatures, mode_name, mode):
    items, _, mb = signatures
    want = _want("ab", mode_name)
    _same(engine.verify(mb, mode), want, items, f"verify, {mode_name}")
    _same(_device(engine, mb, mode), want, items, f"verify_device, {mode_name}")


@pytest.mark.parametrize("mode_name,mode", MODES)
def test_signature_sweeps_as_tx_signatures(engine, signatures, mode_name, mode):
    items, tb, _ = signatures
    want = _want("ab", mode_name)
    _same(engine.verify_tx_signatures(tb, mode), want, items, f"verify_tx_signatures, {mode_name}")
    pb = tb.packed()
    assert pb.stream.size >= B.SIG_LEN_MAX  # the 65,535-byte signature lies in the dense stream
    _same(engine.verify_tx_signatures_packed(pb, mode), want, items, f"packed, {mode_name}")


@pytest.mark.parametrize("mode_name,mode", MODES)
def test_ecdsa_signature_sweep_relaid_out(engine, signatures, mode_name, mode):
    """Sweep a at byte phases 0..3 with poison behind every field, the arena ending with
    size % 4 == 3 on the last byte of the 65,535-byte signature."""
    _, _, mb = signatures
    items = _items("a")
    a = mb.subset(np.arange(len(items)))
    r = LU.relayout_batch(a, seed=404, rem=3, last="sig")
    LU.same_content(LU.batch_fields(a), a.arena, LU.batch_fields(r), r.arena)
    stats = LU.layout_stats(LU.batch_fields(r), r.arena.size)
    assert stats["sig"]["phases"] == {0, 1, 2, 3} and stats["sig"]["ends"] and r.arena.size % 4 == 3
    assert int(r.items["sig_off"][-1]) + B.SIG_LEN_MAX == r.arena.size
    long_ = r.items["sig_len"] > 80
    assert {int(p) for p in r.items["sig_off"][long_] % 4} == {0, 1, 2, 3}
    want = _want("a", mode_name)
    _same(engine.verify(r, mode), want, items, f"relaid out verify, {mode_name}")
    _same(_device(engine, r, mode), want, items, f"relaid out verify_device, {mode_name}")


@pytest.mark.parametrize("mode_name,mode", MODES)
def test_key_sweeps_and_precedence(engine, keys, mode_name, mode):
    items, b, want = keys
    _same(engine.verify(b, mode), want[mode_name], items, f"verify, {mode_name}")
    _same(_device(engine, b, mode), want[mode_name], items, f"verify_device, {mode_name}")
