"""Per-transaction verdicts on the CPU: the host build of corda_amd/csrc/txverdict.h (the lane logic
the kernels of txverdict.hip run, tests/native/txverdict_test.cpp) against a pure-Python restatement of
the rules (tests/txverdict_cases.py), for both record strides and both forms (one lane per transaction,
a wave striding the span), and against the object-level mirror (transactions.verify_signatures_except,
composite.is_fulfilled_by); the same cases once more through a program built with
-fsanitize=address,undefined; RequirementBuilder round trips; the header layouts; the Kotlin / JNI
declarations."""
import os
import re
import subprocess

import numpy as np
import pytest

from corda_amd import _lib
from corda_amd import batch as B

import txverdict_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    out = []
    for stride in (12, 24):
        for with_class in (False, True):
            out.append((f"random/{stride}/{with_class}", C.random_case(11 + stride, 2000, stride, with_class)))
            out.append((f"hostile/{stride}/{with_class}", C.hostile_case(stride, with_class, budget_dag=True,
                                                                         reserved=True)))
        out.append((f"boundary/{stride}", C.boundary_case(3, stride, True)))
    return out


@pytest.fixture(scope="module")
def cases():
    return [(name, c, C.reference(c)) for name, c in _cases()]


def test_header_layouts_match_the_dtypes():
    L = C.native()
    assert [L.tv_sizes(k) for k in range(6)] == [B.TX_CHECK_DTYPE.itemsize, B.REQ_NODE_DTYPE.itemsize,
                                                 B.TX_VERDICT_DTYPE.itemsize, B.REQ_MAX_DEPTH, B.REQ_MAX_VISITS, 32]
    src = open(_lib.HEADER_PATH).read()
    for struct, dt in (("cg_tx_check", B.TX_CHECK_DTYPE), ("cg_req_node", B.REQ_NODE_DTYPE),
                       ("cg_tx_verdict", B.TX_VERDICT_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* (\d+) bytes \*/" % (struct, struct), src, re.S)
        fields = re.findall(r"^\s*(u?int\d+_t)\s+(\w+);", body.group(1), re.M)
        assert [f for _, f in fields] == list(dt.names)
        assert [int(re.search(r"\d+", t).group()) // 8 for t, _ in fields] == [dt[f].itemsize for f in dt.names]
        assert [t.startswith("u") for t, _ in fields] == [dt[f].kind == "u" for f in dt.names]
        assert int(body.group(2)) == dt.itemsize
        off = 0
        for f in dt.names:  # natural C layout: no padding anywhere
            assert dt.fields[f][1] == off
            off += dt[f].itemsize
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(CG_REQ_[A-Z_]+)\s*=?\s+(\d+)", src)}
    assert (enum["CG_REQ_FULFILLED"], enum["CG_REQ_MISSING"], enum["CG_REQ_HOST"], enum["CG_REQ_BAD"]) == \
        (B.REQ_FULFILLED, B.REQ_MISSING, B.REQ_HOST, B.REQ_BAD)
    assert (enum["CG_REQ_MAX_DEPTH"], enum["CG_REQ_MAX_VISITS"]) == (B.REQ_MAX_DEPTH, B.REQ_MAX_VISITS)
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CG_TXV_[A-Z_]+) (\d+)u", src)}
    assert flags == {"CG_TXV_SPAN_BAD": B.TXV_SPAN_BAD, "CG_TXV_REQ_HOST": B.TXV_REQ_HOST,
                     "CG_TXV_COMPOSITE_SIGNER": B.TXV_COMPOSITE_SIGNER}


@pytest.mark.parametrize("lanes", [1, 64])
def test_lane_logic_equals_the_restated_rules(cases, lanes):
    for name, c, want in cases:
        vd, rs, most = C.run_native(c, lanes)
        C.assert_same((vd, rs), want, getattr(c, "names", None), f"{name}, {lanes} lane(s)")
        assert most <= B.REQ_MAX_VISITS, name


def test_random_cases_reach_every_outcome(cases):
    """The random tables are worth something: every status code is a first-bad status somewhere, requirements
    come back fulfilled and missing under leaves and composites, with and without a composite signer."""
    name, c, (vd, rs) = cases[0]
    assert set(vd["status"]) == set(C.STATUSES)
    assert np.count_nonzero(vd["first_bad"] == B.NO_BAD) > 300
    comp_root = c.nodes["n_children"][c.reqs] != 0
    for sel in (comp_root, ~comp_root):
        assert np.count_nonzero(rs[sel] == B.REQ_FULFILLED) > 40 and np.count_nonzero(rs[sel] == B.REQ_MISSING) > 40
    signer = (vd["flags"] & B.TXV_COMPOSITE_SIGNER) != 0
    assert 20 < np.count_nonzero(signer) < len(vd) - 20
    assert np.any(c.checks["n_sigs"] == 0) and np.any(c.checks["n_req"] == 0)
    assert set(rs) <= {B.REQ_FULFILLED, B.REQ_MISSING}


def test_hostile_tables(cases):
    """Each malformed table gives the code the header promises, and the rest of the batch is untouched."""
    c, (vd, rs) = next((c, w) for n, c, w in cases if n == "hostile/12/True")
    got_vd, got_rs, most = C.run_native(c)
    C.assert_same((got_vd, got_rs), (vd, rs), c.names)
    T = {n: t for t, n in enumerate(c.names)}

    def req(name):
        ck = c.checks[T[name]]
        return list(got_rs[int(ck["first_req"]):int(ck["first_req"]) + int(ck["n_req"])])

    def flags(name):
        return int(got_vd[T[name]]["flags"])

    assert req("plain") == [B.REQ_FULFILLED, B.REQ_MISSING, B.REQ_FULFILLED]  # 8 deep is evaluated
    assert (got_vd[T["plain"]]["first_bad"], got_vd[T["plain"]]["status"], flags("plain")) == (1, B.EMPTY, 0)
    assert got_vd[T["plain"]]["n_missing"] == 1
    assert req("child index equal to its parent") == [B.REQ_BAD, B.REQ_FULFILLED]
    assert req("child index below its parent") == [B.REQ_BAD]
    assert req("child range past the node table") == [B.REQ_BAD, B.REQ_FULFILLED]
    assert req("backward child inside a good root") == [B.REQ_BAD]
    assert req("root out of range") == [B.REQ_BAD, B.REQ_BAD, B.REQ_FULFILLED]
    assert req("nested 9 deep") == [B.REQ_HOST, B.REQ_FULFILLED]
    assert req("weights wrap") == [B.REQ_MISSING]
    assert req("no signatures") == [B.REQ_MISSING, B.REQ_MISSING]
    assert got_vd[T["no signatures"]]["status"] == B.VALID and got_vd[T["no signatures"]]["n_missing"] == 2
    assert got_vd[T["no requirements"]].tolist() == (B.NO_BAD, B.VALID, 0, 0)
    assert req("key index past the key table") == [B.REQ_MISSING, B.REQ_MISSING]
    assert got_vd[T["saturation"]]["n_missing"] == 0xFFFF and req("saturation")[-1] == B.REQ_FULFILLED
    assert req("visit budget") == [B.REQ_HOST, B.REQ_FULFILLED] and most == B.REQ_MAX_VISITS
    for name in ("child index equal to its parent", "root out of range", "nested 9 deep", "visit budget",
                 "requirement range past reqs", "requirement range far past reqs"):
        assert flags(name) == B.TXV_REQ_HOST, name
    for name in ("foreign tx_idx", "span past the table", "span far past the table", "span start past the table",
                 "reserved not zero"):
        assert got_vd[T[name]].tolist() == (B.NO_BAD, B.NOT_RUN, B.TXV_SPAN_BAD | B.TXV_REQ_HOST, 0), name
        assert req(name) == [B.REQ_HOST]


def test_under_the_host_sanitizers(cases, tmp_path):
    """The same cases through the stand-alone program built with AddressSanitizer and
    UndefinedBehaviorSanitizer, every table in a heap block of exactly its size."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main() { return 0; }", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    exe = C.build_program(os.path.join(C.HERE, "native", "txverdict_test_san"),
                          ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    for k, (name, c, want) in enumerate(cases):
        for lanes in (1, 64):
            fin, fout = str(tmp_path / f"case{k}.bin"), str(tmp_path / f"out{k}.bin")
            C.to_file(c, lanes, fin)
            r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and r.stdout.startswith("ok: "), name + "\n" + r.stdout + r.stderr[-3000:]
            vd, rs, most = C.from_file(c, fout)
            C.assert_same((vd, rs), want, getattr(c, "names", None), f"{name}, sanitizers, {lanes} lane(s)")
            assert most <= B.REQ_MAX_VISITS


# ---------------------------------------------------------------- the object level
def _ed_keys(n):
    from corda_amd.crypto import PublicKey
    from corda_amd import keys as K
    raw = [bytes([k + 1]) * 32 for k in range(n)]
    return [PublicKey(4, r, B.KEY_RAW) for r in raw], [PublicKey(4, K.ED25519_SPKI_PREFIX + r, B.KEY_SPKI) for r in raw]


def _random_composite(rng, pool, depth):
    from corda_amd.composite import CompositeKey
    b = CompositeKey.Builder()
    n = int(rng.integers(2, 4))
    kids = []
    for j in rng.choice(len(pool), n, replace=False):
        if depth > 1 and rng.random() < 0.4:
            kids.append(_random_composite(rng, pool, depth - 1))
        else:
            kids.append(pool[j])
    weights = [int(rng.integers(1, 4)) for _ in kids]
    for k, w in zip(kids, weights):
        if any(k == o for o in b._children and [c.node for c in b._children]):
            continue
        b.add_key(k, w)
    total = sum(c.weight for c in b._children)
    return b.build(int(rng.integers(1, total + 1))) if len(b._children) > 1 else pool[0]


def test_requirement_builder_round_trip():
    """Equal keys share a class and a root, equal CompositeKeys one child block; every child index is
    greater than its parent's; and the flattened tables, walked by the lane logic, give
    composite.is_fulfilled_by for random signer sets."""
    from corda_amd.composite import CompositeKey, is_fulfilled_by
    rng = np.random.default_rng(7)
    raw, spki = _ed_keys(10)
    rb = B.RequirementBuilder()
    assert [rb.key_class(k) for k in raw] == [rb.key_class(k) for k in spki] == list(range(10))
    shared = CompositeKey.Builder().add_keys(raw[0], spki[1], raw[2]).build(2)  # a notary's 2-of-3
    same = CompositeKey.Builder().add_keys(spki[0], raw[1], spki[2]).build(2)
    assert shared == same
    required = [[raw[3], shared], [same, spki[3]], []]
    for _ in range(60):
        required.append([_random_composite(rng, raw if rng.random() < 0.5 else spki, 3)
                         for _ in range(int(rng.integers(1, 4)))])
    spans = [rb.add_transaction(r) for r in required]
    reqs, nodes = rb.build()
    assert spans[0] == (0, 2) and spans[1] == (2, 2) and spans[2] == (4, 0)
    assert reqs[1] == reqs[2] and reqs[0] == reqs[3]
    comp = np.flatnonzero(nodes["n_children"])
    assert np.all(nodes["a"][comp] > comp) and np.all(nodes["a"][comp] + nodes["n_children"][comp] <= len(nodes))
    assert len(set(zip(nodes["a"][comp].tolist(), nodes["n_children"][comp].tolist()))) < len(comp)  # shared blocks
    # signer sets: each transaction signs with a random subset of the ten keys, in either byte form
    keys = np.zeros(20, B.KEY_DTYPE)
    keys["scheme"] = 4
    key_class = rb.key_classes(raw + spki)
    assert list(key_class) == list(range(10)) * 2
    tx_idx, key_idx, signers = [], [], []
    for t in range(len(required)):
        who = [int(k) for k in rng.choice(20, int(rng.integers(0, 5)), replace=False)]
        signers.append([(raw + spki)[k] for k in who])
        tx_idx += [t] * len(who)
        key_idx += who
    checks = np.zeros(len(required), B.TX_CHECK_DTYPE)
    checks["n_sigs"] = [len(s) for s in signers]
    checks["first_sig"] = np.concatenate([[0], np.cumsum(checks["n_sigs"])[:-1]])
    checks["first_req"], checks["n_req"] = [s[0] for s in spans], [s[1] for s in spans]
    c = C.case(C._sig_table(12, np.array(tx_idx, np.uint32), np.array(key_idx, np.uint32)),
               np.zeros(len(tx_idx), np.uint8), keys, key_class, checks, reqs, nodes)
    vd, rs, _ = C.run_native(c)
    C.assert_same((vd, rs), C.reference(c))
    seen = set()
    for t, req in enumerate(required):
        for r, k in enumerate(req):
            want = B.REQ_FULFILLED if is_fulfilled_by(k, set(signers[t])) else B.REQ_MISSING
            assert rs[spans[t][0] + r] == want, (t, r)
            seen.add(want)
    assert seen == {B.REQ_FULFILLED, B.REQ_MISSING}


class _FakeEngine:
    """verify_required_signatures_packed on the CPU: the statuses are given, the reduction is the host build
    of the lane logic."""
    rsa = False

    def __init__(self, status_of):
        self.status_of = status_of

    def verify_required_signatures_packed(self, pb, checks, reqs, nodes, key_class=None, mode=0, want_status=False):
        status = np.array([self.status_of(int(s["tx_idx"]), j) for j, s in enumerate(pb.sigs)], np.uint8)
        c = C.case(pb.sigs, status, pb.keys, key_class, checks, reqs, nodes)
        vd, rs, _ = C.run_native(c)
        return vd, rs


def test_verify_signatures_except_batch_equals_the_serial_mirror():
    """verify_signatures_except_batch over an engine that reduces on the CPU: per transaction the exception
    of the serial verify_signatures_except (type, message, missing set), for failing signatures at any
    ordinal, missing leaf and composite requirements, keys allowed to be missing and a composite signer."""
    from corda_amd import transactions as T
    from corda_amd.composite import CompositeKey
    from corda_amd.crypto import TransactionSignature, _Crypto
    rng = np.random.default_rng(19)
    raw, spki = _ed_keys(8)
    notary = CompositeKey.Builder().add_keys(raw[0], raw[1], raw[2]).build(2)
    stxs, plan = [], {}
    for t in range(120):
        who = [int(k) for k in rng.choice(8, int(rng.integers(0, 5)), replace=False)]
        sigs = [TransactionSignature(bytes([t % 251, j]) * 32, (raw if rng.random() < 0.5 else spki)[k])
                for j, k in enumerate(who)]
        required = {raw[int(k)] for k in rng.choice(8, int(rng.integers(0, 3)), replace=False)}
        if rng.random() < 0.6:
            required.add(notary)
        stx = T.SignedTransaction(bytes([t]) * 32, sigs, required, [T.Command("Move", (raw[3],))], notary)
        for j in range(len(sigs)):
            plan[(t, j)] = int(rng.choice([B.VALID] * 8 + [B.INVALID, B.SIG_MALFORMED, B.KEY_INVALID, B.EMPTY]))
        stxs.append(stx)
    status_of = lambda t, j: plan[(t, j - sum(len(s.sigs) for s in stxs[:t]))]  # noqa: E731

    class Serial(_Crypto):  # the serial mirror's engine: the planned status of every item, in order
        def verify_batch_ex(self, items, mode=0):
            return np.array([self.pending.pop(0) for _ in items], np.uint8), {}

    crypto = _Crypto()
    crypto.use_engine(_FakeEngine(status_of))
    allowed = (raw[7],)
    got = T.verify_signatures_except_batch(stxs, None, allowed, crypto)
    kinds = set()
    for t, stx in enumerate(stxs):
        serial = Serial()
        serial.pending = [plan[(t, j)] for j in range(len(stx.sigs))]
        want = None
        try:
            T.verify_signatures_except(stx, lambda i, s: b"x", allowed, serial)
        except Exception as e:  # noqa: BLE001
            want = e
        assert type(got[t]) is type(want) and str(got[t]) == str(want), (t, got[t], want)
        if isinstance(want, T.SignaturesMissingException):
            assert got[t].missing == want.missing and got[t].descriptions == want.descriptions and got[t].id == want.id
        kinds.add(type(want).__name__)
    assert {"NoneType", "SignaturesMissingException", "SignatureException"} <= kinds


# ---------------------------------------------------------------- the Kotlin binding and the JNI shim
def test_kotlin_and_jni_declare_the_required_signatures_call():
    kt = open(os.path.join(ROOT, "jvm/src/main/kotlin/net/corda/core/crypto/CryptoBatch.kt")).read()
    c = open(os.path.join(ROOT, "jvm/jni/cordagpu_jni.c")).read()
    decl = re.search(r"external fun nativeVerifyRequiredPacked\((.*?)\): Int", kt, re.S).group(1)
    assert decl.replace(" ", "").replace("\n", "").startswith("ctx:Long,pool:Long,")
    nk = len([p for p in decl.split(",") if p.strip()])
    cm = re.search(r"Java_net_corda_core_crypto_CryptoBatch_nativeVerifyRequiredPacked\((.*?)\)\s*{", c, re.S)
    assert cm and len([p for p in cm.group(1).split(",") if p.strip()]) == nk + 2
    body = c[cm.end():]
    body = body[:body.index("\nJNIEXPORT") if "\nJNIEXPORT" in body else len(body)]
    assert "cg_pool_verify_required_signatures_packed(" in body and "cg_verify_required_signatures_packed(" in body
    assert "fun verifyRequiredSignaturesAll(" in kt
    fn = kt[kt.index("fun verifyRequiredSignaturesAll("):]
    nxt = re.search(r"\n    (?:private |internal )?(?:fun|val|var|class|object|/\*\*|@)", fn[1:])
    fn = fn[:nxt.start() + 1] if nxt else fn
    assert "withHandles {" in fn and "nativeVerifyRequiredPacked(c, p," in fn
    assert "HashMap<PublicKey, Int>" in fn and "CompositeKey" in fn
    # the verdict constants are the header's
    hdr = open(_lib.HEADER_PATH).read()
    for name in ("CG_TXV_SPAN_BAD", "CG_TXV_REQ_HOST", "CG_TXV_COMPOSITE_SIGNER"):
        v = int(re.search(r"#define %s (\d+)u" % name, hdr).group(1))
        assert re.search(r"const val %s = %d\b" % (name, v), kt), name
    for name in ("CG_REQ_FULFILLED", "CG_REQ_MISSING", "CG_REQ_HOST", "CG_REQ_BAD"):
        v = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert re.search(r"const val %s = %d\b" % (name, v), kt), name
    # the byte layouts the Kotlin packer writes are the C structs'
    assert int(re.search(r"TX_CHECK_BYTES = (\d+)", kt).group(1)) == B.TX_CHECK_DTYPE.itemsize
    assert int(re.search(r"REQ_NODE_BYTES = (\d+)", kt).group(1)) == B.REQ_NODE_DTYPE.itemsize
    assert int(re.search(r"TX_VERDICT_BYTES = (\d+)", kt).group(1)) == B.TX_VERDICT_DTYPE.itemsize
