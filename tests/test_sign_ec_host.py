"""CPU tests of the ECDSA signer: the lane code of corda_amd/csrc/sign_ec.h built for the host with
FE_BOUNDS_CHECK at the three fixed-base radixes (tests/hostsignec.py) against tests/golden/ecdsa_sign.json;
the same source as a stand-alone program under the sanitizers; r = x mod n called directly; the DER
encoder against the oracle's; the new C ABI declarations and NULL-context calls; the Python mirror's
random= path through a fake engine that signs with the oracle."""
import ctypes
import hashlib
import os
import random as pyrandom
import re
import subprocess

import numpy as np
import pytest

import hostsignec as H
from corda_amd import _lib, batch as B, crypto as C
from oracle import ecdsa_bc as bc

RECORDS = H.records()
EDGES = H.edges()
FIXTURE = H.FIXTURE


def _n(scheme):
    return bc.CURVES[scheme].n


def test_fixture_shape():
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(os.path.dirname(FIXTURE), "derive_keys.json"))
    for scheme in (2, 3):
        rs = [r for r in RECORDS if r["scheme"] == scheme]
        n = _n(scheme)
        assert {len(r["msg"]) for r in rs if "msg" in r} >= {0, 1, 2, 3, 4, 5, 55, 56, 57, 63, 64, 65, 119, 120, 121}
        assert {len(r["prefix"]) for r in rs if "prefix" in r} == {0, 1, 2, 3, 45, 81, 233, 234}
        ks = {int.from_bytes(r["k"], "big"): r["status"] for r in rs}
        assert all(ks[k] == 0 for k in (1, 2, n - 2, n - 1))
        assert all(ks[k] == H.NONCE_REJECTED for k in (0, n, n + 1, 2 ** 256 - 1))
        assert any(r["status"] == H.NONCE_REJECTED and 0 < int.from_bytes(r["k"], "big") < n for r in rs)  # s = 0
        assert any(r["status"] == H.EMPTY and r["msg"] == b"" for r in rs)
        lens = set()
        for r in rs:
            if r["status"] == 0:
                a, b = bc.der_decode_sig(r["sig"])
                lens |= {("r", len(bc.der_encode_int(a)) - 2), ("s", len(bc.der_encode_int(b)) - 2)}
            else:
                assert r["sig"] == b""
        assert {("r", 33), ("r", 32), ("s", 33), ("s", 32)} <= lens
        assert min(v for a, v in lens if a == "r") <= 31 and min(v for a, v in lens if a == "s") <= 31
        import scalar_edges
        want = {k for w in scalar_edges.WIDE_RADIXES for _, k in scalar_edges.ec_u1_targets(scheme, w)}
        assert {int.from_bytes(k, "big") for s, k, _ in EDGES if s == scheme} == want


def test_fixture_agrees_with_the_oracle():
    """Every full record's bytes are the oracle's (the edges' digests are checked against the lane code,
    and against the oracle at generation)."""
    for r in RECORDS:
        if r["status"] == 0:
            d, k = int.from_bytes(r["d"], "big"), int.from_bytes(r["k"], "big")
            assert bc.der_encode_sig(*bc.sign(r["scheme"], d, H.record_message(r), k)) == r["sig"], r["note"]


@pytest.mark.parametrize("bw", H.RADIXES)
def test_lane_code_matches_every_fixture_record(bw):
    for r in RECORDS:
        want = (r["status"], len(r["sig"]), H.slot(r["sig"]))
        if "msg" in r:
            for phase in range(4):
                assert H.sign_arena(bw, r["scheme"], r["d"], r["msg"], r["k"], phase) == want, (r["note"], phase)
        else:
            assert H.sign_splice(bw, r["scheme"], r["d"], r["prefix"], r["id"], r["suffix"], r["k"]) == want, r["note"]
            assert H.sign_arena(bw, r["scheme"], r["d"], H.record_message(r), r["k"], 1) == want, r["note"]


@pytest.mark.parametrize("bw", H.RADIXES)
def test_lane_code_matches_every_edge_record(bw):
    """The G table's edge scalars as k. The digits the rows were read by include the last entry of a row
    (|digit| = 2^(bw-1)) at this radix."""
    msg, half, reached = H.edge_msg(), 1 << (bw - 1), False
    nd = H.lib(bw).t_g_digits()
    digits = (ctypes.c_int32 * nd)()
    for scheme, k, dg in EDGES:
        st, ln, out = H.sign_arena(bw, scheme, H.key(scheme)[0], msg, k, 0, digits)
        if H.digest(out[:ln]) != dg or st != 0:
            want = bc.der_encode_sig(*bc.sign(scheme, int.from_bytes(H.key(scheme)[0], "big"), msg, int.from_bytes(k, "big")))
            assert (st, out[:ln].hex()) == (0, want.hex()), (scheme, k.hex())
        assert out[ln:] == bytes(H.SLOT - ln)
        reached = reached or any(abs(v) == half for v in digits)
    assert reached


@pytest.mark.parametrize("scheme", (2, 3))
def test_signer_load_check_and_public_key(scheme):
    lb, n = H.lib(26), _n(scheme)
    xy = ctypes.create_string_buffer(64)
    for d in (0, n, n + 1, 2 ** 256 - 1):
        assert lb.t_signer_load(H.CURVE[scheme], d.to_bytes(32, "big"), xy) == H.KEY_INVALID and xy.raw == bytes(64)
    for d in (1, 2, n - 1, int.from_bytes(H.key(scheme)[0], "big")):
        assert lb.t_signer_load(H.CURVE[scheme], d.to_bytes(32, "big"), xy) == 0
        assert xy.raw == bc.raw_key(bc.public_point(scheme, d))
    assert H.key(scheme)[1] == bc.raw_key(bc.public_point(scheme, int.from_bytes(H.key(scheme)[0], "big")))


@pytest.mark.parametrize("scheme", (2, 3))
def test_x_mod_n_at_the_values_no_signature_reaches(scheme):
    """r = x mod n for x = n - 1, n, n + 1 and p - 1: x(k G) >= n has probability ~2^-128, so the
    subtraction is called directly."""
    lb, n, p = H.lib(26), _n(scheme), bc.CURVES[scheme].p
    assert n < p < 2 * n
    out = ctypes.create_string_buffer(32)
    for x in (0, 1, n - 1, n, n + 1, p - 1):
        lb.t_x_mod_n(H.CURVE[scheme], x.to_bytes(32, "big"), out)
        assert int.from_bytes(out.raw, "big") == x % n, hex(x)


def test_der_encoder_matches_the_oracle_at_every_length():
    """StdDSAEncoder.encode for r and s of every byte length with the top bit of the leading byte clear and
    set (1 .. 33 content bytes each), and random pairs."""
    lb, rng = H.lib(26), pyrandom.Random(7)
    out = ctypes.create_string_buffer(H.SLOT)
    vals = [1, 0x7f, 0x80, 0xff]
    for nb in range(2, 33):
        vals += [1 << (8 * nb - 8), (1 << (8 * nb - 1)) - 1, 1 << (8 * nb - 1), (1 << (8 * nb)) - 1]
    pairs = [(a, b) for a in vals for b in (1, 0x80, vals[-1], vals[len(vals) // 2])] + \
            [(b, a) for a in vals for b in (1, 0x80, vals[-1], vals[len(vals) // 2])] + \
            [(rng.getrandbits(rng.randrange(1, 257)) | 1, rng.getrandbits(rng.randrange(1, 257)) | 1) for _ in range(300)]
    for r, s in pairs:
        ln = lb.t_der(r.to_bytes(32, "big"), s.to_bytes(32, "big"), out)
        want = bc.der_encode_sig(r, s)
        assert ln == len(want) and out.raw == H.slot(want), (hex(r), hex(s))


# ---------------------------------------------------------------- the stand-alone program under the sanitizers
def _case_lines():
    lines = []
    for r in RECORDS:
        h = lambda b: b.hex() if b else "-"  # noqa: E731
        if "msg" in r:
            lines.append(f"M {r['scheme']} {r['d'].hex()} {h(r['msg'])} {r['k'].hex()} {r['status']} {h(r['sig'])}")
        else:
            lines.append(f"T {r['scheme']} {r['d'].hex()} {h(r['prefix'])} {r['id'].hex()} {h(r['suffix'])} "
                         f"{r['k'].hex()} {r['status']} {h(r['sig'])}")
    for scheme in (2, 3):
        n, p = _n(scheme), bc.CURVES[scheme].p
        for x in (n - 1, n, n + 1, p - 1):
            lines.append(f"X {scheme} {x.to_bytes(32, 'big').hex()} {(x % n).to_bytes(32, 'big').hex()}")
    return lines


@pytest.mark.parametrize("bw", H.RADIXES)
def test_lane_code_under_sanitizers(bw, tmp_path):
    """The same source with its own main, built with -fsanitize=address,undefined, as a child process over
    the fixture's full records: no sanitizer is loaded into this interpreter."""
    cases = tmp_path / "cases.txt"
    lines = _case_lines()
    cases.write_text("\n".join(lines) + "\n")
    p = subprocess.run([H.sanitized_main(bw), str(cases)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == f"{len(lines)} cases, 0 mismatches"


def test_sanitized_main_reports_a_mismatch(tmp_path):
    """The stand-alone program is not vacuous: a deliberately wrong expected signature is a mismatch."""
    r = next(r for r in RECORDS if "msg" in r and r["status"] == 0)
    bad = bytearray(r["sig"])
    bad[40] ^= 1
    cases = tmp_path / "bad.txt"
    cases.write_text(f"M {r['scheme']} {r['d'].hex()} {r['msg'].hex()} {r['k'].hex()} 0 {bad.hex()}\n")
    p = subprocess.run([H.sanitized_main(26), str(cases)], capture_output=True, text=True)
    assert p.returncode == 1 and "1 cases, 4 mismatches" in p.stdout


# ---------------------------------------------------------------- ABI
def test_header_declarations():
    src = open(_lib.HEADER_PATH).read()
    assert "#define CG_NONCE_REJECTED 9" in src and "#define CG_EC_SIG_MAX 72" in src and "#define CG_ABI_VERSION 2" in src
    assert B.NONCE_REJECTED == 9 and B.EC_SIG_MAX == 72
    block = src[src.index("/* ---- ECDSA signing"):src.index("/* ---- Key derivation")]
    for cite in ("Crypto.kt:395-402", "Crypto.kt:415-422", "NotaryService.kt:73-80", "Not cleared", "not constant-time"):
        assert cite in block, cite
    for fn, n_args in (("cg_ec_signers_load", 6), ("cg_ec_signers_clear", 1), ("cg_ec_sign_tx_ids", 13),
                       ("cg_ec_sign_tx_ids_device", 14), ("cg_ec_sign_batch", 9), ("cg_pool_ec_signers_load", 6),
                       ("cg_pool_ec_signers_clear", 1), ("cg_pool_ec_sign_tx_ids", 14)):
        m = re.search(r"\bint %s\(([^;]*)\);" % fn, src)
        assert m and len(m.group(1).split(",")) == n_args, fn


def test_symbols_exported_and_null_ctx_is_an_argument_error():
    lb = _lib.lib()
    for name in ("cg_ec_signers_load", "cg_ec_signers_clear", "cg_ec_sign_tx_ids", "cg_ec_sign_tx_ids_device",
                 "cg_ec_sign_batch", "cg_pool_ec_signers_load", "cg_pool_ec_signers_clear", "cg_pool_ec_sign_tx_ids"):
        assert name in _lib.declared_symbols() and hasattr(lb, name), name
    assert lb.cg_abi_version() == 2
    buf = np.zeros(128, dtype=np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lb.cg_ec_signers_load(None, p, p, 1, p, p) == -1
    assert lb.cg_ec_signers_clear(None) == -1
    assert lb.cg_ec_sign_tx_ids(None, p, 1, p, 1, None, 0, None, 0, p, p, p, p) == -1
    assert lb.cg_ec_sign_tx_ids_device(None, p, 1, p, 1, None, 0, None, 0, p, p, p, p, None) == -1
    assert lb.cg_ec_sign_batch(None, p, 1, p, 8, p, p, p, p) == -1
    assert lb.cg_pool_ec_signers_load(None, p, p, 1, p, p) == -1
    assert lb.cg_pool_ec_signers_clear(None) == -1
    assert lb.cg_pool_ec_sign_tx_ids(None, p, 1, p, 1, None, 0, None, 0, p, p, p, p, None) == -1
    assert (buf == 0).all() and "NULL" in _lib.last_error()


# ---------------------------------------------------------------- the mirror, through a fake engine
class _FakeEngine:
    """An engine stand-in that signs with the Python oracle and applies BC's refusals: the mirror's packing,
    key-pair check, draws and redraws without a GPU."""

    def __init__(self):
        self.keys, self.loads, self.calls, self.nonce_arrays = [], 0, [], []

    def load_ec_signers(self, keys):
        self.keys, self.loads = [(s, bytes(d)) for s, d in keys], self.loads + 1
        st = np.array([0 if 0 < int.from_bytes(d, "big") < _n(s) else H.KEY_INVALID for s, d in self.keys], dtype=np.uint8)
        return [bc.raw_key(bc.public_point(s, int.from_bytes(d, "big"))) if st[i] == 0 else bytes(64)
                for i, (s, d) in enumerate(self.keys)], st

    def clear_ec_signers(self):
        self.keys = []

    def _sign(self, signer_msgs, nonces):
        n = len(signer_msgs)
        assert isinstance(nonces, np.ndarray) and nonces.dtype == np.uint8 and nonces.size == 32 * n
        self.calls.append(n)
        self.nonce_arrays.append(nonces)
        sigs, ln, st = np.zeros((n, 72), dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        for j, (i, m) in enumerate(signer_msgs):
            scheme, d = self.keys[i]
            k = int.from_bytes(nonces[32 * j:32 * j + 32].tobytes(), "big")
            if not 0 < k < _n(scheme):
                st[j] = H.NONCE_REJECTED
                continue
            sig = bc.der_encode_sig(*bc.sign(scheme, int.from_bytes(d, "big"), m, k))
            sigs[j, :len(sig)], ln[j] = np.frombuffer(sig, dtype=np.uint8), len(sig)
        nonces[:] = 0  # as Engine.sign_ec does with the array the C ABI read
        return sigs, ln, st

    def sign_ec(self, signer_msgs, nonces):
        return self._sign(signer_msgs, nonces)

    def sign_ec_tx_ids(self, sr, nonces):
        msgs = []
        for q in sr.reqs:
            t = sr.tmpls[int(q["tmpl"])]
            pre = bytes(sr.arena[int(t["prefix_off"]):int(t["prefix_off"]) + int(t["prefix_len"])])
            suf = bytes(sr.arena[int(t["suffix_off"]):int(t["suffix_off"]) + int(t["suffix_len"])])
            i = int(q["tx_idx"])
            msgs.append((int(q["signer"]), pre + bytes(sr.ids[32 * i:32 * i + 32]) + suf))
        return self._sign(msgs, nonces)


class _Draws:
    def __init__(self, draws):
        self.draws, self.used = list(draws), 0

    def __call__(self, nbytes):
        assert nbytes == 32
        self.used += 1
        return self.draws[self.used - 1]


def _pair(scheme, d):
    return C.KeyPair(C.PublicKey(scheme, bc.raw_key(bc.public_point(scheme, d)), B.KEY_RAW),
                     C.PrivateKey(scheme, d.to_bytes(32, "big")))


def test_mirror_without_random_still_refuses_ecdsa_keys():
    cr = C._Crypto()
    cr.use_engine(_FakeEngine())
    pair = _pair(3, 12345)
    with pytest.raises(C.UnsupportedOperationException):
        cr.do_sign(pair.private, b"data")
    with pytest.raises(C.UnsupportedOperationException):
        cr.sign_all(pair, [bytes(32)], (1, 3))
    with pytest.raises(C.UnsupportedOperationException):
        cr.do_sign_tx(pair, C.SignableData(bytes(32), 1, 3))
    with pytest.raises(Exception, match="Signing of an empty array is not permitted!"):
        cr.do_sign(pair.private, b"", random=lambda n: bytes(n))  # doSign's order: the empty check first


def test_mirror_redraws_only_the_refused_candidate():
    """secp256r1, first draw 0xFF..FF (>= n): the signature is the oracle's for the second draw, and exactly
    two draws were consumed."""
    cr, fake = C._Crypto(), _FakeEngine()
    cr.use_engine(fake)
    d, k2 = 0x1234567890abcdef, hashlib.sha256(b"second draw").digest()
    draws = _Draws([b"\xff" * 32, k2, b"\x01" * 32])
    sig = cr.do_sign(_pair(3, d).private, b"clear data", random=draws)
    assert sig == bc.der_encode_sig(*bc.sign(3, d, b"clear data", int.from_bytes(k2, "big")))
    assert draws.used == 2 and fake.calls == [1, 1]
    assert all((a == 0).all() for a in fake.nonce_arrays)  # the arrays handed down come back zeroed


def test_mirror_signs_transaction_ids_and_redraws_per_item():
    from corda_amd import signable
    cr, fake = C._Crypto(), _FakeEngine()
    cr.use_engine(fake)
    d = 0xfeedface
    pair = _pair(2, d)
    ids = [hashlib.sha256(bytes([k])).digest() for k in range(4)]
    ks = [hashlib.sha256(b"k%d" % j).digest() for j in range(5)]
    # item 2's first candidate is 0: it alone is redrawn, with the fifth draw (ks[3])
    draws = _Draws(ks[:2] + [bytes(32)] + ks[2:])
    out = cr.sign_all(pair, ids, (1, 2), random=draws)
    pre, suf = signable.template(1, 2)
    used = [ks[0], ks[1], ks[3], ks[2]]
    assert [t.bytes for t in out] == [bc.der_encode_sig(*bc.sign(2, d, pre + i + suf, int.from_bytes(k, "big")))
                                      for i, k in zip(ids, used)]
    assert all(t.by == pair.public and (t.platform_version, t.scheme_number_id) == (1, 2) for t in out)
    assert draws.used == 5 and fake.calls == [4, 1] and fake.loads == 1
    ts = cr.do_sign_tx(pair, C.SignableData(ids[0], 1, 2), random=_Draws([ks[4]]))
    assert ts.bytes == bc.der_encode_sig(*bc.sign(2, d, signable.serialize(ids[0], 1, 2), int.from_bytes(ks[4], "big")))
    assert fake.loads == 1  # the set is kept


def test_mirror_refuses_a_pair_whose_halves_do_not_belong_together():
    cr = C._Crypto()
    cr.use_engine(_FakeEngine())
    a, b = _pair(3, 1111), _pair(3, 2222)
    with pytest.raises(C.IllegalArgumentException, match="not the private key's"):
        cr.do_sign_tx(C.KeyPair(b.public, a.private), C.SignableData(bytes(32), 1, 3), random=lambda n: b"\x05" * n)
    with pytest.raises(C.IllegalArgumentException, match="is not aligned with the key type"):
        cr.do_sign_tx(C.KeyPair(_pair(2, 1111).public, a.private), C.SignableData(bytes(32), 1, 3),
                      random=lambda n: b"\x05" * n)
    with pytest.raises(C.InvalidKeyException):
        cr.do_sign(C.PrivateKey(3, bytes(32)), b"data", random=lambda n: b"\x05" * n)  # d = 0
