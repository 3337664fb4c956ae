"""CPU tests of the RSA plumbing above the kernels: the HIP-free cg_rsa_key_bits export over accepted
and declined keys, CG_FLAG_RSA in the header and the binding, the rsa= option of Engine / EnginePool,
and the routing in corda_amd/crypto.py and transactions.py with a stub engine (RSA items are offered
to the engine only when it runs them, and whatever it declines is decided on the host as before)."""
import inspect
import json
import os
import re

import numpy as np

import composite_cases as CC
from corda_amd import _lib, hostverify
from corda_amd import batch as B
from corda_amd import transactions as T
from corda_amd.crypto import BatchItem, HOST_EXCEPTION, InvalidKeySpecException, PublicKey
from corda_amd.engine import Engine, EnginePool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GPU = json.load(open(os.path.join(HERE, "golden", "rsa_gpu.json")))
OLD = json.load(open(os.path.join(HERE, "golden", "rsa.json")))


def test_flag_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "cordagpu.h")).read()
    assert re.search(r"#define CG_FLAG_RSA 2u\b", hdr)
    assert re.search(r"#define CG_ABI_VERSION 2\b", hdr)
    assert _lib.FLAG_RSA == 2 and _lib.FLAG_RSA != _lib.FLAG_STAGE_TIMING
    assert "cg_rsa_key_bits" in _lib.declared_symbols()
    assert hasattr(_lib.lib(), "cg_rsa_key_bits")


def test_rsa_key_bits_over_accepted_and_declined_keys():
    for kid, k in GPU["keys"].items():
        spki = bytes.fromhex(k["spki"])
        got = _lib.rsa_key_bits(spki)
        if k["accepted"]:
            assert got == k["bits"] == hostverify.rsa_decode_key(spki)[0].bit_length(), kid
        elif kid == "fmt_raw":  # a good encoding: declined by its cg_key.fmt, which the decode never sees
            assert got == 2048
        else:
            assert got == 0, kid
    for i in OLD["items"]:
        assert _lib.rsa_key_bits(bytes.fromhex(i["key"])) == i["bits"]
    # every truncation and every single-byte change of the header of a good key is declined or still
    # decodes to the same modulus length (a change inside n or e): never a crash, never another size
    good = bytes.fromhex(GPU["keys"]["rsa1024"]["spki"])
    assert _lib.rsa_key_bits(good) == 1024
    for cut in range(len(good)):
        assert _lib.rsa_key_bits(good[:cut]) == 0, cut
    for pos in range(33):
        for delta in (1, 0x80):
            b = bytearray(good)
            b[pos] ^= delta
            assert _lib.rsa_key_bits(bytes(b)) in (0, 1024, 1025), pos  # (the sign byte: one bit longer)
    assert _lib.rsa_key_bits(b"") == 0 and _lib.rsa_key_bits(b"\x30" * 300) == 0
    # the other schemes' keys
    for f in ("ed25519.json", "ecdsa.json"):
        it = json.load(open(os.path.join(HERE, "golden", f)))["items"][0]
        assert _lib.rsa_key_bits(bytes.fromhex(it["key"])) == 0


def test_engine_and_pool_take_the_rsa_option():
    for cls in (Engine, EnginePool):
        p = inspect.signature(cls.__init__).parameters
        assert "rsa" in p and p["rsa"].default is False, cls
    src = open(os.path.join(ROOT, "corda_amd", "engine.py")).read()
    assert src.count("_lib.FLAG_RSA if rsa else 0") == 2 and src.count("self.rsa = bool(rsa)") == 2


def test_jvm_sources_carry_the_option():
    kt = open(os.path.join(ROOT, "jvm/src/main/kotlin/net/corda/core/crypto/CryptoBatch.kt")).read()
    c = open(os.path.join(ROOT, "jvm/jni/cordagpu_jni.c")).read()
    assert "val gpuRsa: Boolean = false" in kt and 'g.getBoolean("gpuRsa")' in kt
    assert "if (c.gpuRsa) CG_FLAG_RSA else 0" in kt and "private const val CG_FLAG_RSA = 2" in kt
    assert "cfg.flags = (uint32_t)flags" in c
    # the fallback for whatever the GPU declines stays
    assert re.search(r"CG_UNSUPPORTED -> \{ Crypto\.doVerify\(item\.publicKey", kt)


class StubEngine:
    """Records what it is handed and declines everything RSA, as a GPU whose decode accepts no key
    would; the other schemes go to the C oracle (tests/composite_cases.OracleEngine)."""

    def __init__(self, rsa):
        self.rsa = rsa
        self.offered = []  # scheme of every item of every call

    def verify(self, batch, mode=0):
        schemes = batch.keys["scheme"][batch.items["key_idx"]]
        self.offered.extend(int(s) for s in schemes)
        if (schemes == 1).all():
            return np.full(batch.n, B.UNSUPPORTED, np.uint8)
        st = CC.OracleEngine().verify(batch, mode)
        st[schemes == 1] = B.UNSUPPORTED
        return st


def _rsa_items():
    out = [(BatchItem(PublicKey(1, bytes.fromhex(i["key"]), B.KEY_SPKI), bytes.fromhex(i["sig"]),
                      bytes.fromhex(i["msg"])), i["expect"]) for i in OLD["items"]]
    for i in GPU["items"]:
        k = GPU["keys"][i["key"]]
        if i["key_fmt"] == B.KEY_SPKI:
            out.append((BatchItem(PublicKey(1, bytes.fromhex(k["spki"]), B.KEY_SPKI), bytes.fromhex(i["sig"]),
                                  bytes.fromhex(i["msg"])), i["expect"]))
    return out


def test_crypto_routing_with_a_stub_engine():
    items = _rsa_items()
    out = {}
    for rsa in (False, True):
        eng = StubEngine(rsa)
        crypto = CC.crypto_with(eng)
        for mode in (B.MODE_ISVALID, B.MODE_DOVERIFY):
            st, err = crypto.verify_batch_ex([b for b, _ in items], mode)
            out[rsa, mode] = (st.copy(), {k: type(v) for k, v in err.items()})
            for j, (b, expect) in enumerate(items):
                if expect == "HOST_EXCEPTION":
                    assert st[j] == HOST_EXCEPTION and isinstance(err[j], InvalidKeySpecException)
                elif mode == B.MODE_DOVERIFY and (not b.signature_data or not b.clear_data):
                    assert st[j] == B.EMPTY
                else:
                    assert st[j] == B.STATUS_BY_NAME[expect], (rsa, mode, j)
        # offered to the engine only when the engine runs RSA
        assert (1 in eng.offered) == rsa
        if rsa:
            assert eng.offered.count(1) == 2 * len(items)
        # the existing fallback assertions hold either way (a mixed batch included)
        CC.rsa_fallback(crypto)
    for mode in (B.MODE_ISVALID, B.MODE_DOVERIFY):  # today's host verdicts, item for item
        assert np.array_equal(out[False, mode][0], out[True, mode][0]) and out[False, mode][1] == out[True, mode][1]
    # a key that is not X.509 is never offered
    eng = StubEngine(True)
    crypto = CC.crypto_with(eng)
    crypto.verify_batch_ex([BatchItem(PublicKey(1, b"\x00" * 64, B.KEY_RAW), b"s", b"m")], B.MODE_ISVALID)
    assert eng.offered == []


def test_composite_rsa_leaf_joins_the_gpu_batch():
    from corda_amd.composite import CompositeKey, CompositeSignaturesWithKeys
    from corda_amd.crypto import TransactionSignature
    from corda_amd import signable
    k = OLD["test_private_key"]
    n, d = int(k["n"], 16), int(k["d"], 16)
    rk = PublicKey(1, bytes.fromhex(k["spki"]), B.KEY_SPKI)
    (sa, a) = CC.party(20)
    ck = CompositeKey.Builder().add_keys(a, rk).build()
    pre, suf = signable.template(1, 1)
    rsig = TransactionSignature(hostverify.rsa_pss_sign(n, d, pre + CC.SECURE_HASH + suf, bytes(32)), rk, 1, 1)
    sig = CompositeSignaturesWithKeys([CC.tx_sig(sa, a), rsig])
    for rsa in (False, True):
        eng = StubEngine(rsa)
        crypto = CC.crypto_with(eng)
        assert crypto.is_valid(ck, sig, CC.SECURE_HASH) is True  # the stub declines: the host decides the leaf
        assert (1 in eng.offered) == rsa


def test_transactions_pack_rsa_signatures_only_for_an_rsa_engine():
    from corda_amd.crypto import TransactionSignature
    rk = PublicKey(1, bytes.fromhex(OLD["test_private_key"]["spki"]), B.KEY_SPKI)
    stx = T.SignedWireTransaction(T.WireTransactionData([b"c"], bytes(32), b"\x01" + bytes(32)),
                                  [TransactionSignature(b"\x07" * 256, rk, 1, 1)])
    for rsa, want in ((False, 1), (True, 256)):
        txs, comps, keys, sigs, tmpls, arena = T.pack_signed_transactions([stx], rsa)
        assert int(sigs["sig_len"][0]) == want
    assert int(T.pack_signed_transactions([stx])[3]["sig_len"][0]) == 1
