"""The Ed25519 signer on the CPU: its lane arithmetic (corda_amd/csrc: sc_muladd, the 32- and
64-byte-prefix SHA-512 forms, ed_fixed_base9, ed_encode, ed_signer_expand) compiled for the host with
FE_BOUNDS_CHECK at every fixed-base radix and held against Python integers, hashlib and the Python
oracle; the same source as a stand-alone program under the address and undefined-behaviour sanitizers;
the new C ABI structs and NULL-context calls; the Python mirror's exceptions.

The digit edges of the fixed-base table (a zero digit, +-2^(BW-1), the carry through every row) are
held here and by the crafted-S verify tests over the same table on the GPU (test_gpu_scalar_edges.py):
the r of a signature is a hash output and cannot be steered to them."""
import ctypes
import hashlib
import random
import subprocess

import numpy as np
import pytest

import hostsign as H
from corda_amd import _lib
from corda_amd import batch as B
from corda_amd import crypto as C
from oracle import ed25519_i2p as ed

L = H.L
RECORDS = H.records()


def test_fixture_shape():
    """What the generator promises: ~200 records, the RFC vectors, every boundary length, every splice."""
    assert 190 <= len(RECORDS) <= 210
    lens = {len(bytes.fromhex(r["msg"])) for r in RECORDS if "msg" in r}
    assert lens >= {0, 1, 47, 48, 79, 80, 111, 112, 127, 128, 129, 175, 176, 207, 208, 303, 304, 335, 336, 4096}
    splices = {(len(r["prefix"]) // 2, len(r["suffix"]) // 2) for r in RECORDS if "prefix" in r}
    assert splices == {(p, s) for p in (0, 1, 2, 3, 45, 81, 233) for s in (0, 3)} | {(234, 3)}
    assert sum(r["status"] == B.EMPTY for r in RECORDS) == 1
    for r in RECORDS:  # the fixture against the oracle it came from
        seed = bytes.fromhex(r["seed"])
        assert ed.public_from_seed(seed).hex() == r["pub"]
        if r["status"] == 0:
            assert ed.sign(seed, H.record_message(r)).hex() == r["sig"]
        else:
            assert r["sig"] == "00" * 64 and H.record_message(r) == b""


def _muladd(lb, k, a, r):
    out = np.zeros(8, dtype="<u4")
    lb.t_sc_muladd(H.ptr(H.scalar_words(k)), H.ptr(H.scalar_words(a)), H.ptr(H.scalar_words(r)), H.ptr(out))
    return int.from_bytes(out.tobytes(), "little")


def test_sc_muladd():
    lb = H.lib(26)
    cases = [(0, 0, 0), (L - 1, 2 ** 255 - 8, L - 1), (L - 1, 2 ** 254, L - 1), (0, 2 ** 255 - 8, L - 1), (L - 1, 0, 0)]
    rng = random.Random(8032)
    for _ in range(1000):
        a = (rng.getrandbits(255) & ~7 & ~(1 << 254)) | (1 << 254) if rng.random() < 0.5 else rng.getrandbits(255)
        cases.append((rng.randrange(L), a, rng.randrange(L)))
    for k, a, r in cases:
        assert _muladd(lb, k, a, r) == (r + k * a) % L, (k, a, r)


def _fixed_base(lb, s, bw):
    enc = np.zeros(8, dtype="<u4")
    dig = np.zeros(H.n_digits(bw), dtype="<i4")
    lb.t_fixed_base(H.ptr(H.scalar_words(s)), H.ptr(enc), H.ptr(dig))
    return enc.tobytes(), [int(d) for d in dig]


def _mul_b(s):
    return ed.encode_point(ed._to_affine(ed.scalarmult(s, ed.B))) if s else bytes([1]) + bytes(31)


@pytest.mark.parametrize("bw", H.RADIXES)
def test_fixed_base_crafted_and_random(bw):
    lb = H.lib(bw)
    assert lb.t_b_digits() == H.n_digits(bw)
    cases = H.crafted_scalars(bw)
    rng = random.Random(bw)
    cases += [("random", rng.randrange(L)) for _ in range(64)]
    for note, s in cases:
        enc, dig = _fixed_base(lb, s, bw)
        assert dig == H.recode(s, bw), note
        assert enc == _mul_b(s), (bw, note)
    assert _fixed_base(lb, 0, bw)[0] == bytes([1]) + bytes(31)  # the identity
    half = 1 << (bw - 1)
    # the crafted scalars do reach the last entry of every row below the top, and a zero in three rows
    last = dict(cases)["every digit below the top -2^(bw-1)"]
    assert H.recode(last, bw)[:-1] == [-half] * (H.n_digits(bw) - 1)


def _hash_inputs():
    lens = sorted({len(H.record_message(r)) for r in RECORDS if "msg" in r and r["status"] == 0})
    return lens


@pytest.mark.parametrize("pw", (8, 16))
def test_sha512_prefix_arena_form(pw):
    """SHA-512(prefix || msg), 32- and 64-byte prefix, at every fixture length and byte phase."""
    lb = H.lib(26)
    rng = random.Random(pw)
    for ln in _hash_inputs():
        prefix = bytes(rng.getrandbits(8) for _ in range(4 * pw))
        msg = bytes(rng.getrandbits(8) for _ in range(ln))
        for phase in range(4):
            out = np.zeros(16, dtype="<u4")
            lb.t_sha512_prefix_arena(pw, H.ptr(H.words(prefix)), msg, ln, phase, H.ptr(out))
            assert out.tobytes() == hashlib.sha512(prefix + msg).digest(), (pw, ln, phase)


@pytest.mark.parametrize("pw", (8, 16))
def test_sha512_prefix_splice_form(pw):
    lb = H.lib(26)
    rng = random.Random(100 + pw)
    shapes = sorted({(len(r["prefix"]) // 2, len(r["suffix"]) // 2) for r in RECORDS if "prefix" in r})
    for pl, sl in shapes:
        prefix = bytes(rng.getrandbits(8) for _ in range(4 * pw))
        pre, tx_id, suf = (bytes(rng.getrandbits(8) for _ in range(n)) for n in (pl, 32, sl))
        out = np.zeros(16, dtype="<u4")
        lb.t_sha512_prefix_splice(pw, H.ptr(H.words(prefix)), pre, pl, tx_id, suf, sl, H.ptr(out))
        assert out.tobytes() == hashlib.sha512(prefix + pre + tx_id + suf).digest(), (pw, pl, sl)


@pytest.mark.parametrize("bw", H.RADIXES)
def test_signer_expand_and_lane_path_match_fixture(bw):
    """ed_signer_expand and the whole per-item lane path against every fixture record."""
    lb = H.lib(bw)
    expanded = {}
    for r in RECORDS:
        seed = bytes.fromhex(r["seed"])
        if seed not in expanded:
            out = np.zeros(24, dtype="<u4")
            lb.t_signer_expand(H.ptr(H.words(seed)), H.ptr(out))
            a, prefix = ed.secret_expand(seed)
            assert out[:8].tobytes() == a.to_bytes(32, "little") and out[8:16].tobytes() == prefix
            expanded[seed] = out[16:].tobytes()
        assert expanded[seed].hex() == r["pub"], r["note"]
        if r["status"] != 0:
            continue
        sig = np.zeros(16, dtype="<u4")
        if "msg" in r:
            msg = bytes.fromhex(r["msg"])
            for phase in (range(4) if bw == 26 else (1,)):
                lb.t_sign_arena(H.ptr(H.words(seed)), msg, len(msg), phase, H.ptr(sig))
                assert sig.tobytes().hex() == r["sig"], (r["note"], phase)
        else:
            pre, tx_id, suf = (bytes.fromhex(r[k]) for k in ("prefix", "id", "suffix"))
            lb.t_sign_splice(H.ptr(H.words(seed)), pre, len(pre), tx_id, suf, len(suf), H.ptr(sig))
            assert sig.tobytes().hex() == r["sig"], r["note"]


def _case_file(path, bw):
    with open(path, "w") as f:
        for r in RECORDS:
            if r["status"] != 0:
                continue
            if "msg" in r:
                f.write(f"M {r['seed']} {r['pub']} {r['msg']} {r['sig']}\n")
            else:
                f.write(f"T {r['seed']} {r['pub']} {r['prefix'] or '-'} {r['id']} {r['suffix'] or '-'} {r['sig']}\n")
        for _, s in H.crafted_scalars(bw):
            f.write(f"B {s.to_bytes(32, 'little').hex()} {_mul_b(s).hex()}\n")


@pytest.mark.parametrize("bw", H.RADIXES)
def test_lane_code_under_sanitizers(bw, tmp_path):
    """The same source with its own main, built with -fsanitize=address,undefined, as a child process
    over the fixture and the crafted scalars: no sanitizer is loaded into this interpreter."""
    exe = H.sanitized_main(bw)
    cases = str(tmp_path / "cases.txt")
    _case_file(cases, bw)
    p = subprocess.run([exe, cases], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    n = sum(r["status"] == 0 for r in RECORDS) + len(H.crafted_scalars(bw))
    assert p.stdout.strip() == f"{n} cases, 0 mismatches"


def test_sanitized_main_reports_a_mismatch(tmp_path):
    """The stand-alone program is not vacuous: a wrong expected signature is a mismatch."""
    r = next(r for r in RECORDS if "msg" in r and r["status"] == 0)
    bad = bytearray.fromhex(r["sig"])
    bad[40] ^= 1
    cases = tmp_path / "bad.txt"
    cases.write_text(f"M {r['seed']} {r['pub']} {r['msg']} {bad.hex()}\n")
    p = subprocess.run([H.sanitized_main(26), str(cases)], capture_output=True, text=True)
    assert p.returncode == 1 and "1 cases, 4 mismatches" in p.stdout


# ---------------------------------------------------------------- ABI
def test_sign_structs_match_header():
    src = open(_lib.HEADER_PATH).read()
    assert "} cg_sign_req;      /* 8 bytes */" in src and "} cg_sign_item;      /* 16 bytes */" in src
    assert "#define CG_SIGNERS_MAX 65535" in src and "#define CG_ABI_VERSION 2" in src
    assert B.SIGN_REQ_DTYPE.itemsize == 8 and B.SIGN_ITEM_DTYPE.itemsize == 16
    assert [B.SIGN_REQ_DTYPE.fields[f][1] for f in ("tx_idx", "signer", "tmpl")] == [0, 4, 6]
    assert [B.SIGN_ITEM_DTYPE.fields[f][1] for f in ("msg_off", "msg_len", "signer")] == [0, 8, 12]
    # the header's own field order and widths
    import re
    req = re.search(r"typedef struct cg_sign_req \{(.*?)\} cg_sign_req;", src, re.S).group(1)
    assert re.findall(r"(uint\d+_t)\s+(\w+);", req) == [("uint32_t", "tx_idx"), ("uint16_t", "signer"), ("uint16_t", "tmpl")]
    item = re.search(r"typedef struct cg_sign_item \{(.*?)\} cg_sign_item;", src, re.S).group(1)
    assert re.findall(r"(uint\d+_t)\s+(\w+);", item) == [("uint64_t", "msg_off"), ("uint32_t", "msg_len"),
                                                          ("uint32_t", "signer")]


def test_sign_symbols_exported_and_null_ctx_is_an_argument_error():
    lb = _lib.lib()
    for name in ("cg_signers_load", "cg_signers_clear", "cg_sign_tx_ids", "cg_sign_tx_ids_device", "cg_sign_batch",
                 "cg_pool_signers_load", "cg_pool_signers_clear", "cg_pool_sign_tx_ids"):
        assert name in _lib.declared_symbols() and hasattr(lb, name), name
    assert lb.cg_abi_version() == 2
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lb.cg_signers_load(None, p, 1, p) == -1
    assert lb.cg_signers_clear(None) == -1
    assert lb.cg_sign_tx_ids(None, p, 1, p, 1, None, 0, None, 0, p, p) == -1
    assert lb.cg_sign_tx_ids_device(None, p, 1, p, 1, None, 0, None, 0, p, p, None) == -1
    assert lb.cg_sign_batch(None, p, 1, p, 8, p, p) == -1
    assert lb.cg_pool_signers_load(None, p, 1, p) == -1
    assert lb.cg_pool_signers_clear(None) == -1
    assert lb.cg_pool_sign_tx_ids(None, p, 1, p, 1, None, 0, None, 0, p, p, None) == -1
    assert (buf == 0).all() and "NULL" in _lib.last_error()


def test_sign_request_builder_packs_ids_templates_and_requests():
    b = B.SignRequestBuilder()
    t0, t1 = b.template(b"prefix-0", b"s0"), b.template(b"p1", b"")
    assert b.template(b"prefix-0", b"s0") == t0
    ids = [bytes([k]) * 32 for k in range(3)]
    for k, i in enumerate(ids + ids[:1]):
        b.add_request(k % 2, b.tx_id(i), (t0, t1)[k % 2])
    sr = b.build()
    assert sr.n == 4 and sr.n_ids == 3 and sr.reqs.dtype == B.SIGN_REQ_DTYPE
    assert list(sr.reqs["tx_idx"]) == [0, 1, 2, 0] and list(sr.reqs["signer"]) == [0, 1, 0, 1]
    assert list(sr.reqs["tmpl"]) == [t0, t1, t0, t1]
    t = sr.tmpls[t0]
    assert bytes(sr.arena[int(t["prefix_off"]):int(t["prefix_off"]) + int(t["prefix_len"])]) == b"prefix-0"
    assert bytes(sr.arena[int(t["suffix_off"]):int(t["suffix_off"]) + int(t["suffix_len"])]) == b"s0"
    with pytest.raises(ValueError):
        b.add_request(0x10000, 0, 0)
    with pytest.raises(ValueError):
        b.tx_id(b"short")


# ---------------------------------------------------------------- the mirror's exceptions (no engine is reached)
def test_mirror_refuses_before_the_engine():
    seed = bytes.fromhex(RECORDS[1]["seed"])
    priv = C.PrivateKey(C.EDDSA_ED25519_SHA512, seed)
    pub = C.PublicKey(C.EDDSA_ED25519_SHA512, bytes.fromhex(RECORDS[1]["pub"]))
    assert seed.hex() not in repr(priv)
    with pytest.raises(Exception, match="Signing of an empty array is not permitted!"):
        C.Crypto.do_sign(priv, b"")
    k1 = C.PrivateKey(C.ECDSA_SECP256K1_SHA256, bytes(32))
    with pytest.raises(C.UnsupportedOperationException):
        C.Crypto.do_sign(k1, b"data")
    with pytest.raises(Exception, match="Signing of an empty array is not permitted!"):
        C.Crypto.do_sign(k1, b"")  # doSign's own order: the empty check comes before any signing
    with pytest.raises(C.IllegalArgumentException, match="Unsupported key/algorithm"):
        C.Crypto.do_sign(C.PrivateKey(99, bytes(32)), b"data")
    r1 = C.PublicKey(C.ECDSA_SECP256R1_SHA256, bytes(33), B.KEY_RAW)
    with pytest.raises(C.IllegalArgumentException,
                       match="Metadata schemeCodeName: ECDSA_SECP256R1_SHA256 is not aligned with the key type: "
                             "EDDSA_ED25519_SHA512."):
        C.Crypto.do_sign_tx(C.KeyPair(r1, priv), C.SignableData(bytes(32)))
    with pytest.raises(C.UnsupportedOperationException):
        C.Crypto.sign_all(C.KeyPair(C.PublicKey(C.ECDSA_SECP256K1_SHA256, bytes(33)), k1), [bytes(32)])
    with pytest.raises(C.InvalidKeyException):
        C.Crypto.do_sign(C.PrivateKey(C.EDDSA_ED25519_SHA512, bytes(31)), b"data")
    assert pub == C.PublicKey(C.EDDSA_ED25519_SHA512, bytes.fromhex(RECORDS[1]["pub"]))


class _FakeEngine:
    """An engine stand-in that signs with the Python oracle: the mirror's packing, key-pair check and
    status handling without a GPU."""

    def __init__(self):
        self.seeds, self.loads = [], 0

    def load_signers(self, seeds):
        self.seeds, self.loads = [bytes(s) for s in seeds], self.loads + 1
        return [ed.public_from_seed(s) for s in self.seeds]

    def clear_signers(self):
        self.seeds = []

    def sign(self, signer_msgs):
        sigs = np.frombuffer(b"".join(ed.sign(self.seeds[i], m) for i, m in signer_msgs), dtype=np.uint8)
        return sigs.reshape(-1, 64), np.zeros(len(signer_msgs), dtype=np.uint8)

    def sign_tx_ids(self, sr):
        out = []
        for q in sr.reqs:
            t = sr.tmpls[int(q["tmpl"])]
            pre = bytes(sr.arena[int(t["prefix_off"]):int(t["prefix_off"]) + int(t["prefix_len"])])
            suf = bytes(sr.arena[int(t["suffix_off"]):int(t["suffix_off"]) + int(t["suffix_len"])])
            i = int(q["tx_idx"])
            out.append(ed.sign(self.seeds[int(q["signer"])], pre + bytes(sr.ids[32 * i:32 * i + 32]) + suf))
        return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, 64), np.zeros(sr.n, dtype=np.uint8)


def test_mirror_signs_through_the_engine_interface():
    from corda_amd import signable
    cr = C._Crypto()
    fake = _FakeEngine()
    cr.use_engine(fake)
    seeds = [ed.entropy_seed(n) for n in (20, 70)]
    pairs = [C.KeyPair(C.PublicKey(C.EDDSA_ED25519_SHA512, ed.public_from_seed(s)),
                       C.PrivateKey(C.EDDSA_ED25519_SHA512, s)) for s in seeds]
    assert cr.do_sign(pairs[0].private, b"abc") == ed.sign(seeds[0], b"abc")
    ids = [hashlib.sha256(bytes([k])).digest() for k in range(5)]
    out = cr.sign_all(pairs[1], ids, (1, 4))
    pre, suf = signable.template(1, 4)
    assert [t.bytes for t in out] == [ed.sign(seeds[1], pre + i + suf) for i in ids]
    assert all(t.by == pairs[1].public and (t.platform_version, t.scheme_number_id) == (1, 4) for t in out)
    ts = cr.do_sign_tx(pairs[0], C.SignableData(ids[0], 1, 4))
    assert ts.bytes == ed.sign(seeds[0], signable.serialize(ids[0], 1, 4)) and ts.by == pairs[0].public
    assert fake.loads == 2 and fake.seeds == seeds  # one load per new key, the set kept
    # a pair whose public half belongs to another private key
    with pytest.raises(C.IllegalArgumentException, match="not the private key's"):
        cr.do_sign_tx(C.KeyPair(pairs[1].public, pairs[0].private), C.SignableData(ids[0]))
    assert cr.sign_all(pairs[0], []) == []
    cr.forget_signers()
    assert fake.seeds == []
