"""tests/golden/rsa_special.json on the GPU, Engine(rsa=True): special-form prime moduli, whose key
preparation reaches the carry ripple of rsa_resolve inside k_rsa_keyprep (a valid signature verifies
only if R^2 mod n came out right), and keys for every branch of the exponent ladder (e = 1, even e,
a set middle bit, every bit set). Every verdict equals the fixture's `expect`, which
tests/test_rsa_special.py ties to the restatement on the CPU."""
import json
import os

import numpy as np
import pytest

from corda_amd import _lib
from corda_amd import batch as B

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    g = json.load(open(os.path.join(HERE, "golden", name)))
    return g["keys"], [{"kid": i["key"], "key": bytes.fromhex(g["keys"][i["key"]]["spki"]), "fmt": i["key_fmt"],
                        "sig": bytes.fromhex(i["sig"]), "msg": bytes.fromhex(i["msg"]), "expect": i["expect"],
                        "note": i["key"] + ": " + i["note"]} for i in g["items"]]


KEYS, ITEMS = _load("rsa_special.json")
SPECIAL = [k for k in KEYS if "c" in KEYS[k]]


@pytest.fixture(scope="module")
def eng(engine):  # `engine` first: the session's default context (and torch's device init) come first
    from corda_amd.engine import Engine
    e = Engine(0, table_bytes_max=int(_lib.lib().cg_table_bytes(22)), rsa=True)
    yield e
    e.close()


def pack(items, own_keys=False):
    bb = B.BatchBuilder()
    for i in items:
        if own_keys:
            bb._key_index.clear()  # a key-table entry per item
        bb.add_with_key(1, i["fmt"], i["key"], i["sig"], i["msg"])
    return bb.build()


def want(items, mode):
    """`expect`; a DOVERIFY caller gets EMPTY for an empty signature or message (none here)."""
    assert all(len(i["sig"]) and len(i["msg"]) for i in items)
    return np.array([B.STATUS_BY_NAME[i["expect"]] for i in items], dtype=np.uint8)


def _bad(items, st, exp):
    return [(items[j]["note"], int(st[j]), int(exp[j])) for j in np.flatnonzero(st != exp)]


@pytest.mark.parametrize("mode", [B.MODE_DOVERIFY, B.MODE_ISVALID])
def test_every_item_host_and_device_forms(eng, mode):
    import torch
    b = pack(ITEMS)
    exp = want(ITEMS, mode)
    assert (exp == B.VALID).sum() >= 97 and (exp == B.INVALID).sum() >= 34
    st = eng.verify(b, mode)
    assert not _bad(ITEMS, st, exp), _bad(ITEMS, st, exp)[:10]
    for kid in KEYS:  # every key has a VALID item: without one nothing witnesses its arithmetic
        assert any(i["kid"] == kid and s == B.VALID for i, s in zip(ITEMS, st)), kid
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    kd, idd, ad = up(b.keys), up(b.items), up(b.arena)
    sd = torch.full((b.n,), 255, dtype=torch.uint8, device=dev)
    eng.verify_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size, sd.data_ptr(), mode)
    torch.cuda.synchronize()
    st = sd.cpu().numpy()
    assert not _bad(ITEMS, st, exp), ("verify_device", _bad(ITEMS, st, exp)[:10])
    sd.fill_(255)
    eng.prepare_keys_device(kd.data_ptr(), len(b.keys), ad.data_ptr(), b.arena.size)
    eng.verify_items_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size,
                            sd.data_ptr(), mode)
    torch.cuda.synchronize()
    st = sd.cpu().numpy()
    assert not _bad(ITEMS, st, exp), ("prepare_keys + verify_items", _bad(ITEMS, st, exp)[:10])


def test_each_special_key_between_two_ordinary_keys(eng):
    """Key-table neighbours of other sizes: ordinary, special, ordinary, special, ..., every item under
    its own key-table entry, so each special key's preparation runs beside two ordinary ones."""
    okeys, oitems = _load("rsa_gpu.json")
    ordinary = [i for i in oitems if okeys[i["kid"]]["accepted"] and i["note"].endswith(": valid")]
    assert len({i["kid"] for i in ordinary}) >= 6
    items = []
    for j, kid in enumerate(KEYS):
        items.append(ordinary[j % len(ordinary)])
        items.append(next(i for i in ITEMS if i["kid"] == kid and i["expect"] == "VALID"))
    items.append(ordinary[len(KEYS) % len(ordinary)])
    b = pack(items, own_keys=True)
    assert len(b.keys) == len(items) == 2 * len(KEYS) + 1
    st = eng.verify(b, B.MODE_DOVERIFY)
    assert (st == B.VALID).all(), _bad(items, st, want(items, B.MODE_DOVERIFY))


def test_many_items_under_one_special_key(eng):
    """130 items under one special 2048-bit key (more waves than one block, the key prepared once), then
    2 x 8192 + 5 items, more than the verify grid has waves, so that a wave takes two signatures per
    round (G = 2) under the special key."""
    mine = [i for i in ITEMS if i["kid"] == "p2048"]
    assert len(mine) == 12
    items = [mine[j % 12] for j in range(130)]
    exp = want(items, B.MODE_ISVALID)
    st = eng.verify(pack(items), B.MODE_ISVALID)
    assert np.array_equal(st, exp), _bad(items, st, exp)[:10]
    assert (st == B.VALID).sum() == 97  # 9 of a key's 12 items are valid
    b0 = pack(mine)
    idx = np.arange(2 * 8192 + 5) % 12
    st = eng.verify(B.Batch(b0.keys, b0.items[idx].copy(), b0.arena), B.MODE_DOVERIFY)
    exp = want(mine, B.MODE_DOVERIFY)[idx]
    assert np.array_equal(st, exp), np.flatnonzero(st != exp)[:10]
