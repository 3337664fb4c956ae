"""RSA_SHA256 (RSASSA-PSS) on the GPU: Engine(rsa=True) / CG_FLAG_RSA through every verify entry
point. Every verdict is exact: it equals the BC 1.57 restatement (corda_amd/hostverify.py) on the
materialised bytes, keys the device decode declines stay UNSUPPORTED, and the verdicts of the other
schemes' items equal the default engine's."""
import ctypes
import json
import os

import numpy as np
import pytest

import composite_cases as CC
import golden_io
import txsig_util
from corda_amd import _lib, hostverify, signable
from corda_amd import batch as B
from corda_amd import transactions as T
from corda_amd.crypto import BatchItem, InvalidKeySpecException, PublicKey, TransactionSignature

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _smallest_tables():
    return int(_lib.lib().cg_table_bytes(22))


@pytest.fixture(scope="module")
def eng(engine):  # `engine` first: the session's default context (and torch's device init) come first
    from corda_amd.engine import Engine
    e = Engine(0, table_bytes_max=_smallest_tables(), rsa=True)
    yield e
    e.close()


# ---------------------------------------------------------------- fixtures and the reference
def _fixture_items():
    g = json.load(open(os.path.join(HERE, "golden", "rsa_gpu.json")))
    out = []
    for i in g["items"]:
        k = g["keys"][i["key"]]
        out.append({"key": bytes.fromhex(k["spki"]), "fmt": i["key_fmt"], "sig": bytes.fromhex(i["sig"]),
                    "msg": bytes.fromhex(i["msg"]), "accepted": k["accepted"], "expect": i["expect"],
                    "note": i["key"] + ": " + i["note"]})
    for i in golden_io.load("rsa.json"):
        out.append({"key": bytes.fromhex(i["key"]), "fmt": i["key_fmt"], "sig": bytes.fromhex(i["sig"]),
                    "msg": bytes.fromhex(i["msg"]), "accepted": True, "expect": i["expect"],
                    "note": "rsa.json: " + i["note"]})
    return g["keys"], out


KEYS, FIXTURE = _fixture_items()
_DECODED = {}


def host_status(key, sig, msg, mode):
    """The restatement's status for an accepted key (hostverify on the bytes; doVerify's empty checks)."""
    if mode == B.MODE_DOVERIFY and (len(sig) == 0 or len(msg) == 0):
        return B.EMPTY
    if key not in _DECODED:
        _DECODED[key] = hostverify.rsa_decode_key(key)
    return B.VALID if hostverify.rsa_verify(_DECODED[key], sig, msg) else B.INVALID


def expected(items, mode):
    return np.array([host_status(i["key"], i["sig"], i["msg"], mode) if i["accepted"] else B.UNSUPPORTED
                     for i in items], dtype=np.uint8)


def pack(items, own_keys=False):
    """items: dicts with key / fmt / sig / msg (scheme 1) or golden items (hex fields, scheme)."""
    bb = B.BatchBuilder()
    for i in items:
        if own_keys:
            bb._key_index.clear()  # a key-table entry (and a copy of the key bytes) per item
        if "scheme" in i:
            bb.add_with_key(i["scheme"], i["key_fmt"], bytes.fromhex(i["key"]), bytes.fromhex(i["sig"]),
                            bytes.fromhex(i["msg"]))
        else:
            bb.add_with_key(1, i["fmt"], i["key"], i["sig"], i["msg"])
    return bb.build()


def _signed_pool():
    """Signed items under every accepted fixture key: per key 6 valid and 2 corrupted signatures over
    messages of several lengths (made once; the batch-shape tests draw from it)."""
    rng = np.random.default_rng(0x25A)
    pool = {}
    for kid, k in KEYS.items():
        if not k["accepted"] or "d" not in k or kid.endswith("_noparams"):
            continue
        n, d, spki = int(k["n"], 16), int(k["d"], 16), bytes.fromhex(k["spki"])
        lst = []
        for j in range(8):
            msg = rng.integers(0, 256, int(rng.choice([1, 31, 64, 270, 300])), dtype=np.uint8).tobytes()
            sig = hostverify.rsa_pss_sign(n, d, msg, rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            if j >= 6:
                sig = sig[:-1] + bytes([sig[-1] ^ (1 << (j - 6))])
            lst.append({"key": spki, "fmt": 1, "sig": sig, "msg": msg, "accepted": True})
        pool[kid] = lst
    return pool


@pytest.fixture(scope="module")
def pool():
    return _signed_pool()


def _mixed(pool, n_rsa, n_other, seed):
    """n_rsa RSA items drawn over every key and n_other golden Ed25519 / ECDSA items, shuffled."""
    rng = np.random.default_rng(seed)
    kids = sorted(pool)
    rsa = [pool[kids[int(rng.integers(len(kids)))]][int(rng.integers(8))] for _ in range(n_rsa)]
    gold = golden_io.load("ed25519.json") + golden_io.load("ecdsa.json")
    other = [gold[int(j)] for j in rng.integers(0, len(gold), n_other)]
    items = rsa + other
    order = rng.permutation(len(items))
    return [items[int(j)] for j in order]


def _check_mixed(items, st, ref_other, mode, what):
    """RSA verdicts vs the restatement, every other item vs the default engine's verdict."""
    for j, it in enumerate(items):
        if "scheme" in it:
            assert st[j] == ref_other[j], (what, j, it["note"], int(st[j]), int(ref_other[j]))
        else:
            want = host_status(it["key"], it["sig"], it["msg"], mode)
            assert st[j] == want, (what, j, len(it["key"]), int(st[j]), want)


# ---------------------------------------------------------------- 1. the flag
def test_open_accepts_the_rsa_flag(engine):  # (`engine`: the session's context opens the device first)
    L = _lib.lib()
    for flags, want in ((_lib.FLAG_RSA, 0), (_lib.FLAG_RSA | _lib.FLAG_STAGE_TIMING, 0), (4, -1)):
        cfg = _lib.cg_config(0, flags, 0, 0, 0, 0, 0, _smallest_tables())
        h = ctypes.c_void_p()
        rc = L.cg_open(ctypes.byref(h), ctypes.byref(cfg))
        if h:
            L.cg_close(h)
        assert rc == want, (flags, rc)


# ---------------------------------------------------------------- 2. every fixture item, both modes
@pytest.mark.parametrize("mode", [B.MODE_DOVERIFY, B.MODE_ISVALID])
def test_every_fixture_item(eng, engine, mode):
    b = pack(FIXTURE)
    st = eng.verify(b, mode)
    want = expected(FIXTURE, mode)
    bad = [(FIXTURE[j]["note"], int(st[j]), int(want[j])) for j in np.flatnonzero(st != want)]
    assert not bad, bad[:10]
    assert (st == B.UNSUPPORTED).sum() == sum(1 for i in FIXTURE if not i["accepted"]) >= 11
    assert (st == B.VALID).sum() >= 60 and (st == B.INVALID).sum() >= 100
    if mode == B.MODE_DOVERIFY:
        assert (st == B.EMPTY).sum() >= 12
    # cg_rsa_key_bits agrees with what the engine did, key by key
    for i, s in zip(FIXTURE, st):
        assert (_lib.rsa_key_bits(i["key"]) != 0 and i["fmt"] == B.KEY_SPKI) == (s != B.UNSUPPORTED), i["note"]
    # the default engine: the existing behaviour, UNSUPPORTED everywhere
    assert (engine.verify(b, mode) == B.UNSUPPORTED).all()


# ---------------------------------------------------------------- 3. batch shapes
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 130])
def test_batch_sizes(eng, pool, n):
    kids = sorted(pool)
    items = [pool[kids[j % len(kids)]][(j // len(kids)) % 8] for j in range(n)]
    st = eng.verify(pack(items), B.MODE_DOVERIFY)
    assert np.array_equal(st, expected(items, B.MODE_DOVERIFY)), st.tolist()


def test_all_items_under_one_key(eng, pool):
    items = [pool["rsa3072"][j % 8] for j in range(70)]
    st = eng.verify(pack(items), B.MODE_ISVALID)
    assert np.array_equal(st, expected(items, B.MODE_ISVALID))
    assert (st == B.VALID).sum() == 54


def test_every_item_under_its_own_key_adjacent_moduli_differ(eng, pool):
    order = ["rsa1024", "rsa4096", "rsa1025", "rsa3072", "rsa1032", "rsa2048e3"]
    items = [pool[order[j % 6]][(j // 6) % 8] for j in range(66)]
    b = pack(items, own_keys=True)
    assert len(b.keys) == 66
    st = eng.verify(b, B.MODE_DOVERIFY)
    assert np.array_equal(st, expected(items, B.MODE_DOVERIFY)), st.tolist()


def test_interleaved_with_the_other_schemes(eng, engine, pool):
    items = _mixed(pool, 40, 120, 7)
    b = pack(items)
    for mode in (B.MODE_DOVERIFY, B.MODE_ISVALID):
        _check_mixed(items, eng.verify(b, mode), engine.verify(b, mode), mode, "mixed")
    # a flag-on call without any RSA key changes no verdict
    gold = [i for i in items if "scheme" in i]
    bg = pack(gold)
    assert np.array_equal(eng.verify(bg), engine.verify(bg))


def test_more_items_than_waves(eng, pool):
    """Above 8192 listed items (the verify grid's waves) a wave takes several signatures per round and
    hashes their messages lane-parallel: 3 x 8192 + 77 items, so G = 3 with a ragged last group, early
    verdicts (EMPTY, NOT_RUN, an over-long signature) mixed into the groups, and a second engine call
    with 40 000 items that walks the list twice. The reference is computed once per distinct item."""
    kids = sorted(pool)
    base = [pool[k][j] for k in kids for j in range(8)]
    base.append(dict(base[0], msg=b""))                    # EMPTY under doVerify
    base.append(dict(base[9], sig=b"\x00" + base[9]["sig"]))  # longer than the modulus: INVALID
    want_base = expected(base, B.MODE_DOVERIFY)
    b0 = pack(base)
    for n in (3 * 8192 + 77, 40000):
        idx = np.arange(n) % len(base)
        items = b0.items[idx].copy()
        items["msg_off"][5::97] = b0.arena.size + 8  # outside the arena: NOT_RUN
        want = want_base[idx].copy()
        want[5::97] = np.where(want[5::97] == B.EMPTY, B.EMPTY, B.NOT_RUN)
        st = eng.verify(B.Batch(b0.keys, items, b0.arena), B.MODE_DOVERIFY)
        assert np.array_equal(st, want), np.flatnonzero(st != want)[:10]


# ---------------------------------------------------------------- 4. chunking and the device forms
def test_chunked_host_and_device_forms(engine, pool):
    import torch
    from corda_amd.engine import Engine
    items = _mixed(pool, 70, 130, 11)
    b = pack(items)
    ref_other = engine.verify(b)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    with Engine(0, chunk_items=64, table_bytes_max=_smallest_tables(), rsa=True) as e:
        rsa_at = {j for j, it in enumerate(items) if "scheme" not in it}
        assert all(any(j in rsa_at for j in range(c, c + 50)) for c in (0, 50, 100, 150))  # RSA in every chunk
        _check_mixed(items, e.verify(b), ref_other, B.MODE_DOVERIFY, "host, 64-item chunks")
        kd, idd, ad = up(b.keys), up(b.items), up(b.arena)
        sd = torch.full((b.n,), 255, dtype=torch.uint8, device=dev)
        e.verify_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size, sd.data_ptr())
        torch.cuda.synchronize()
        _check_mixed(items, sd.cpu().numpy(), ref_other, B.MODE_DOVERIFY, "verify_device")
        sd.fill_(255)
        e.prepare_keys_device(kd.data_ptr(), len(b.keys), ad.data_ptr(), b.arena.size)
        e.verify_items_device(kd.data_ptr(), len(b.keys), idd.data_ptr(), b.n, ad.data_ptr(), b.arena.size,
                              sd.data_ptr())
        torch.cuda.synchronize()
        _check_mixed(items, sd.cpu().numpy(), ref_other, B.MODE_DOVERIFY, "prepare_keys + verify_items")


# ---------------------------------------------------------------- 5. arena layout
def test_arena_layout(eng, pool):
    """Unaligned signature and message offsets, the arena ending at the last byte of a signature, and
    a signature / message running past the arena (NOT_RUN)."""
    picks = [pool["rsa1025"][0], pool["rsa4096"][1], pool["rsa2048e3"][6], pool["rsa1032"][2]]
    arena = bytearray()
    keys = np.zeros(len(picks), B.KEY_DTYPE)
    items = np.zeros(len(picks) + 2, B.ITEM_DTYPE)
    for j, it in enumerate(picks):
        arena += bytes((-len(arena)) % 4) + bytes(1 + j % 3)  # key offsets 1, 2, 3 mod 4
        keys[j] = (len(arena), len(it["key"]), 1, 1, 0)
        arena += it["key"]
    for j, it in enumerate(picks):
        arena += bytes(1 if len(arena) % 4 == 0 else 0)
        items[j]["msg_off"], items[j]["msg_len"], items[j]["key_idx"] = len(arena), len(it["msg"]), j
        arena += it["msg"]
        if j == len(picks) - 1:  # the last signature ends the arena, at a length that is no multiple of 4
            while (len(arena) + len(it["sig"])) % 4 != 1:
                arena += b"\x00"
        elif len(arena) % 4 == 0:
            arena += b"\x00"
        items[j]["sig_off"], items[j]["sig_len"] = len(arena), len(it["sig"])
        arena += it["sig"]
    assert len(arena) % 4 == 1 and any(int(o) % 4 for o in items["sig_off"][:4])
    items[4] = items[0]
    items[4]["sig_off"] = len(arena) - 10  # runs past the arena
    items[5] = items[1]
    items[5]["msg_off"] = len(arena) - 3
    n = len(arena)
    buf = np.frombuffer(bytes(arena) + b"\xa5" * 3, dtype=np.uint8).copy()  # what follows never matters
    st = eng.verify(B.Batch(keys, items, buf[:n]), B.MODE_DOVERIFY)
    want = [host_status(i["key"], i["sig"], i["msg"], B.MODE_DOVERIFY) for i in picks] + [B.NOT_RUN, B.NOT_RUN]
    assert st.tolist() == want
    assert want[:4] == [B.VALID, B.VALID, B.INVALID, B.VALID]


# ---------------------------------------------------------------- 6. transaction forms
def _rsa2048():
    k = json.load(open(os.path.join(HERE, "golden", "rsa.json")))["test_private_key"]
    return int(k["n"], 16), int(k["d"], 16), bytes.fromhex(k["spki"])


def _tx_case():
    """Transactions signed by an Ed25519 key and the 2048-bit RSA test key, under two SignatureMetadata
    templates; one RSA signature is over another transaction's id."""
    from oracle import corda as ocorda, ed25519_i2p as ed
    rng = np.random.default_rng(21)
    n, d, spki = _rsa2048()
    rk = PublicKey(1, spki, B.KEY_SPKI)
    seed = ed.entropy_seed(20)
    ek = PublicKey(4, ed.public_from_seed(seed))
    stxs, tids = [], []
    for t in range(5):
        comps = [rng.integers(0, 256, int(rng.integers(1, 200)), dtype=np.uint8).tobytes() for _ in range(3)]
        salt = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        tids.append(ocorda.tx_id(comps, salt, b"\x01" + salt))
        stxs.append([comps, salt])
    out = []
    for t, (comps, salt) in enumerate(stxs):
        pv = 1 + t % 2  # two templates per scheme id
        signed_id = tids[(t + 1) % 5] if t == 3 else tids[t]  # transaction 3: RSA over the wrong id
        rsig = hostverify.rsa_pss_sign(n, d, signable.serialize(signed_id, pv, 1), bytes([t]) * 32)
        sigs = [TransactionSignature(ed.sign(seed, signable.serialize(tids[t], pv, 4)), ek, pv, 4),
                TransactionSignature(rsig, rk, pv, 1)]
        out.append(T.SignedWireTransaction(T.WireTransactionData(comps, salt, b"\x01" + salt), sigs))
    return out, tids


def _tx_reference(stxs, tids):
    want = []
    for t, stx in enumerate(stxs):
        for s in stx.sigs:
            msg = signable.serialize(tids[t], s.platform_version, s.scheme_number_id)
            if s.by.scheme == 1:
                want.append(host_status(s.by.encoded, s.bytes, msg, B.MODE_DOVERIFY))
            else:
                want.append(B.VALID)
    return want


def test_transaction_forms(eng):
    import torch
    stxs, tids = _tx_case()
    want = _tx_reference(stxs, tids)
    assert want == [B.VALID] * 6 + [B.VALID, B.INVALID] + [B.VALID] * 2
    # cg_verify_transactions: ids computed on the device
    txs, comps, keys, sigs, tmpls, arena = T.pack_signed_transactions(stxs, rsa=True)
    ids, txst, sst = eng.verify_transactions(txs, comps, keys, sigs, tmpls, arena)
    assert [bytes(i) for i in ids] == tids and not txst.any()
    assert sst.tolist() == want
    # signatures over known ids: 24-byte and 12-byte tables, host and device forms
    tb = B.TxSigBuilder()
    for t, stx in enumerate(stxs):
        for s in stx.sigs:
            k = tb.key(s.by.scheme, s.by.fmt, s.by.encoded)
            tb.add_signature(k, tb.tx_id(tids[t]), tb.template(*signable.template(s.platform_version, s.scheme_number_id)),
                             s.bytes)
    tb = tb.build()
    assert len(tb.tmpls) == 4
    assert eng.verify_tx_signatures(tb).tolist() == want
    pb = tb.packed()
    assert eng.verify_tx_signatures_packed(pb).tolist() == want
    # the message form of the same signatures
    assert eng.verify(txsig_util.to_message_batch(tb)).tolist() == want
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    kd, ijd, sgd, ad = up(tb.keys), up(tb.ids), up(tb.sigs), up(tb.arena)
    sd = torch.full((tb.n,), 255, dtype=torch.uint8, device=dev)
    eng.verify_tx_signatures_device(kd.data_ptr(), len(tb.keys), ijd.data_ptr(), tb.n_ids, sgd.data_ptr(), tb.n,
                                    tb.tmpls, ad.data_ptr(), tb.arena.size, sd.data_ptr())
    torch.cuda.synchronize()
    assert sd.cpu().numpy().tolist() == want
    # packed device form: the stream lives in the arena after the key and template bytes
    base = (pb.arena.size + 15) & ~15
    whole = np.concatenate([pb.arena, np.zeros(base - pb.arena.size, np.uint8), pb.stream, np.zeros(16, np.uint8)])
    wd, s12 = up(whole), up(pb.sigs)
    sd.fill_(255)
    eng.verify_tx_signatures_packed_device(kd.data_ptr(), len(pb.keys), ijd.data_ptr(), pb.n_ids, s12.data_ptr(), pb.n,
                                           base, pb.stream.size, pb.tmpls, wd.data_ptr(), base + pb.stream.size,
                                           sd.data_ptr())
    torch.cuda.synchronize()
    assert sd.cpu().numpy().tolist() == want


# ---------------------------------------------------------------- 7. pool
def test_pool_equals_single_engine(eng, pool):
    from corda_amd.engine import EnginePool
    items = _mixed(pool, 30, 60, 13)
    b = pack(items)
    with EnginePool([0, 0], table_bytes_max=_smallest_tables(), rsa=True) as p:
        assert p.rsa
        assert np.array_equal(p.verify(b), eng.verify(b))
        assert np.array_equal(p.verify(b, B.MODE_ISVALID), eng.verify(b, B.MODE_ISVALID))


# ---------------------------------------------------------------- 8. Crypto
class _Counting:
    """Engine wrapper: what Crypto handed to the GPU and what came back."""

    def __init__(self, e):
        self.e, self.rsa, self.calls = e, e.rsa, []

    def verify(self, batch, mode=0):
        st = self.e.verify(batch, mode)
        self.calls.append((batch.keys["scheme"][batch.items["key_idx"]].copy(), st.copy()))
        return st

    def __getattr__(self, name):
        return getattr(self.e, name)


def test_crypto_runs_rsa_on_the_gpu(eng):
    ce = _Counting(eng)
    crypto = CC.crypto_with(ce)
    CC.rsa_fallback(crypto)  # the existing assertions, the verdicts now the GPU's
    schemes = np.concatenate([c[0] for c in ce.calls])
    sts = np.concatenate([c[1] for c in ce.calls])
    assert (schemes == 1).sum() >= 58 and not (sts[schemes == 1] == B.UNSUPPORTED).any()
    # a declined key still yields the reference's host outcome
    for i in FIXTURE:
        if i["accepted"] or i["fmt"] != B.KEY_SPKI:
            continue
        n0 = len(ce.calls)
        st, err = crypto.verify_batch_ex([BatchItem(PublicKey(1, i["key"], B.KEY_SPKI), i["sig"], i["msg"])],
                                         B.MODE_ISVALID)
        assert len(ce.calls) == n0 + 1 and ce.calls[-1][1].tolist() == [B.UNSUPPORTED], i["note"]
        if i["expect"] == "HOST_EXCEPTION":
            assert st[0] == 240 and isinstance(err[0], InvalidKeySpecException), i["note"]
        else:
            assert st[0] == B.STATUS_BY_NAME[i["expect"]] and not err, i["note"]
    # transactions with RSA signers: no host fallback is needed any more
    stxs, tids = _tx_case()
    n0 = len(ce.calls)
    ids, results = T.verify_wire_transactions(stxs, crypto)
    assert ids == tids and len(ce.calls) == n0  # verify_transactions only: no per-item fallback batch
    assert [r is None for r in results] == [True, True, True, False, True]
    assert results[3][0] == 1
