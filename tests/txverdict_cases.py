"""Test helper for the per-transaction verdicts (cg_tx_verdicts): the cases, a pure-Python restatement of
the rules in include/cordagpu.h, and the host build of corda_amd/csrc/txverdict.h
(tests/native/txverdict_test.cpp) that the CPU tests check against the restatement and the GPU tests
use as the kernels' reference."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np

from corda_amd import batch as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "txverdict_test.cpp")
HDR = os.path.join(HERE, "..", "corda_amd", "csrc", "txverdict.h")
ABI = os.path.join(HERE, "..", "include", "cordagpu.h")
SO = os.path.join(HERE, "native", "libtxverdicttest.so")
STATUSES = np.array([B.VALID, B.INVALID, B.SIG_MALFORMED, B.KEY_INVALID, B.UNSUPPORTED, B.EMPTY, B.NOT_RUN], np.uint8)
INT_MAX = 2**31 - 1


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in (SRC, HDR, ABI))


def native():
    if _stale(SO):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", SO + ".tmp", SRC])
        os.replace(SO + ".tmp", SO)
    L = ctypes.CDLL(SO)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.tv_run.argtypes = [vp, u32, u64, vp, vp, u32, vp, vp, u64, vp, u32, vp, u32, u32, vp, vp]
    L.tv_run.restype = u64
    L.tv_sizes.argtypes = [u32]
    L.tv_sizes.restype = u32
    return L


def build_program(out, flags):
    if _stale(out):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-o", out, SRC])
    return out


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def case(sigs, status, keys, key_class, checks, reqs, nodes, **extra):
    return SimpleNamespace(sigs=sigs, status=np.ascontiguousarray(status, np.uint8), keys=keys, key_class=key_class,
                           checks=checks, reqs=np.ascontiguousarray(reqs, np.uint32), nodes=nodes, **extra)


def run_native(c, lanes=1):
    """(verdicts, req_status, most node visits of one requirement) from the host build of txverdict.h."""
    vd = np.zeros(len(c.checks), B.TX_VERDICT_DTYPE)
    rs = np.full(len(c.reqs), 77, np.uint8)
    most = native().tv_run(_p(c.sigs), c.sigs.dtype.itemsize, len(c.sigs), _p(c.status), _p(c.keys), len(c.keys),
                           _p(c.key_class), _p(c.checks), len(c.checks), _p(c.reqs), len(c.reqs), _p(c.nodes),
                           len(c.nodes), lanes, _p(vd), _p(rs))
    return vd, rs, int(most)


def to_file(c, lanes, path):
    """The case in the form tests/native/txverdict_test.cpp's main reads."""
    h = np.array([c.sigs.dtype.itemsize, len(c.sigs), len(c.keys), c.key_class is not None, len(c.checks), len(c.reqs),
                  len(c.nodes), lanes], np.uint64)
    parts = [h, c.sigs, c.status, c.keys] + ([c.key_class] if c.key_class is not None else []) + \
        [c.checks, c.reqs, c.nodes]
    with open(path, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())


def from_file(c, path):
    raw = open(path, "rb").read()
    nv, nr = 8 * len(c.checks), len(c.reqs)
    assert len(raw) == nv + nr + 8
    return (np.frombuffer(raw[:nv], B.TX_VERDICT_DTYPE), np.frombuffer(raw[nv:nv + nr], np.uint8),
            int(np.frombuffer(raw[nv + nr:], np.uint64)[0]))


# ---------------------------------------------------------------- the rules, restated
class _Host(Exception):
    pass


class _Bad(Exception):
    pass


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def _requirement(nodes, root, classes):
    """CG_REQ_* of the requirement rooted at `root` for a signer class set (no composite signer)."""
    n = len(nodes)
    visits = [1]

    def children_ok(i):
        return int(nodes[i]["a"]) > i and int(nodes[i]["a"]) + int(nodes[i]["n_children"]) <= n

    def composite(i, depth):
        if not children_ok(i):
            raise _Bad
        if depth > B.REQ_MAX_DEPTH:
            raise _Host
        total = 0
        for ch in range(int(nodes[i]["a"]), int(nodes[i]["a"]) + int(nodes[i]["n_children"])):
            if visits[0] >= B.REQ_MAX_VISITS:
                raise _Host
            visits[0] += 1
            if nodes[ch]["n_children"] == 0:
                ok = int(nodes[ch]["a"]) in classes
            else:
                ok = composite(ch, depth + 1)
            if ok:
                total = _i32(total + int(nodes[ch]["weight"]))
        return total >= int(nodes[i]["threshold"])

    if root >= n:
        return B.REQ_BAD
    if nodes[root]["n_children"] == 0:
        return B.REQ_FULFILLED if int(nodes[root]["a"]) in classes else B.REQ_MISSING
    try:
        return B.REQ_FULFILLED if composite(root, 1) else B.REQ_MISSING
    except _Host:
        return B.REQ_HOST
    except _Bad:
        return B.REQ_BAD


def reference(c):
    """(verdicts, req_status) by the rules of include/cordagpu.h, transaction by transaction."""
    n_sigs, n_keys, n_reqs = len(c.sigs), len(c.keys), len(c.reqs)
    vd = np.zeros(len(c.checks), B.TX_VERDICT_DTYPE)
    rs = np.full(n_reqs, B.REQ_HOST, np.uint8)
    memo = {}
    for t, ck in enumerate(c.checks):
        fs, n, fr, nr = int(ck["first_sig"]), int(ck["n_sigs"]), int(ck["first_req"]), int(ck["n_req"])
        span_bad = ck["reserved"] != 0 or fs + n > n_sigs or bool(np.any(c.sigs["tx_idx"][fs:fs + n] != t))
        flags, first_bad, status, classes, comp = 0, B.NO_BAD, B.VALID, frozenset(), False
        if span_bad:
            flags, status = B.TXV_SPAN_BAD, B.NOT_RUN
        else:
            bad = np.flatnonzero(c.status[fs:fs + n] != B.VALID)
            if bad.size:
                first_bad, status = int(bad[0]), int(c.status[fs + bad[0]])
            kidx = c.sigs["key_idx"][fs:fs + n].astype(np.int64)
            kidx = kidx[kidx < n_keys]
            classes = frozenset(int(x) for x in (c.key_class[kidx] if c.key_class is not None else kidx))
            comp = bool(np.any(c.keys["scheme"][kidx] == B.COMPOSITE_KEY))
            flags |= B.TXV_COMPOSITE_SIGNER if comp else 0
        missing = 0
        if fr + nr > n_reqs:
            flags |= B.TXV_REQ_HOST
        else:
            for r in range(fr, fr + nr):
                if span_bad:
                    st = B.REQ_HOST
                else:
                    root = int(c.reqs[r])
                    if (root, classes) not in memo:
                        memo[(root, classes)] = _requirement(c.nodes, root, classes)
                    st = memo[(root, classes)]
                    if st == B.REQ_FULFILLED and comp and c.nodes[root]["n_children"] != 0:
                        st = B.REQ_MISSING
                missing += st == B.REQ_MISSING
                if st in (B.REQ_HOST, B.REQ_BAD):
                    flags |= B.TXV_REQ_HOST
                rs[r] = st
        vd[t] = (first_bad, status, flags, min(missing, 0xFFFF))
    return vd, rs


# ---------------------------------------------------------------- case builders
class Nodes:
    """A node table under construction: children blocks are appended after their parents."""

    def __init__(self):
        self.rows = []

    def leaf(self, cls, weight=0):
        self.rows.append([cls, 0, weight, 0])
        return len(self.rows) - 1

    def block(self, n):
        first = len(self.rows)
        self.rows += [[0, 0, 0, 0] for _ in range(n)]
        return first

    def random_tree(self, rng, at, depth, n_classes, weight=0):
        """Fills node `at` with a random subtree of at most `depth` composite levels."""
        if depth == 0 or rng.random() < 0.35:
            self.rows[at] = [int(rng.integers(0, n_classes)), 0, weight, 0]
            return
        n = int(rng.integers(2, 5))
        first = self.block(n)
        ws = [INT_MAX if rng.random() < 0.05 else int(rng.integers(1, 6)) for _ in range(n)]
        small = sum(w for w in ws if w != INT_MAX) or 1
        thr = int(rng.integers(-1, small + 2)) if rng.random() < 0.9 else int(rng.integers(-2**31, 2**31))
        self.rows[at] = [first, n, weight, thr]
        for j in range(n):
            self.random_tree(rng, first + j, depth - 1, n_classes, ws[j])

    def array(self):
        a = np.zeros(len(self.rows), B.REQ_NODE_DTYPE)
        for i, (x, n, w, t) in enumerate(self.rows):
            a[i] = (x, n, w, t)
        return a


def _sig_table(stride, tx_idx, key_idx):
    t = np.zeros(len(tx_idx), B.TXSIG12_DTYPE if stride == 12 else B.TXSIG_DTYPE)
    t["tx_idx"], t["key_idx"] = tx_idx, key_idx
    t["sig_len"] = 64
    return t


def _keys(rng, n_keys, composite_every=0):
    keys = np.zeros(n_keys, B.KEY_DTYPE)
    keys["scheme"] = rng.choice([2, 3, 4], n_keys)
    keys["len"] = 32
    if composite_every:
        keys["scheme"][composite_every - 1::composite_every] = B.COMPOSITE_KEY
    return keys


def random_case(seed, n_tx, stride, with_class, sizes=None, n_keys=16, composite_every=16, p_valid=0.8):
    """n_tx transactions of 0-9 signatures (or `sizes`), statuses from all seven codes, 0-3 requirements
    each out of 40 shared roots: leaves and random composite trees of depth <= 3. Key classes, when given,
    put several key entries in one class (duplicate signers, raw / SPKI pairs); every 16th key entry is a
    CompositeKey (a composite signer)."""
    rng = np.random.default_rng(seed)
    keys = _keys(rng, n_keys, composite_every)
    n_classes = n_keys // 2 if with_class else n_keys
    key_class = rng.integers(0, n_classes, n_keys).astype(np.uint32) if with_class else None
    nd = Nodes()
    n_roots = 40
    nd.block(n_roots)
    for r in range(n_roots):
        nd.random_tree(rng, r, 3, n_classes + 3)  # some classes no key has
    sizes = rng.integers(0, 10, n_tx) if sizes is None else np.asarray(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)])
    n_sigs = int(first[-1])
    tx_idx = np.repeat(np.arange(n_tx), sizes)
    key_idx = rng.integers(0, n_keys, n_sigs)
    # a transaction signs with few distinct keys, so that leaves are often fulfilled
    key_idx = (key_idx % 6) + np.repeat(rng.integers(0, max(1, n_keys - 5), n_tx), sizes) if n_sigs else key_idx
    status = np.where(rng.random(n_sigs) < p_valid, B.VALID, rng.choice(STATUSES, n_sigs)).astype(np.uint8)
    n_req = rng.integers(0, 4, n_tx)
    first_req = np.concatenate([[0], np.cumsum(n_req)])
    reqs = rng.integers(0, n_roots, int(first_req[-1])).astype(np.uint32)
    checks = np.zeros(n_tx, B.TX_CHECK_DTYPE)
    checks["first_sig"], checks["n_sigs"] = first[:-1], sizes
    checks["first_req"], checks["n_req"] = first_req[:-1], n_req
    return case(_sig_table(stride, tx_idx, key_idx), status, keys, key_class, checks, reqs, nd.array())


def boundary_case(seed, stride, with_class):
    """The small / wave boundary and long spans: transactions of exactly 32, 33, 64 and 65 signatures, one
    of 5 000 whose only bad status is at ordinal 4 999 and one whose only bad one is at ordinal 0, among
    short ones; the long spans' requirement leaves are signed only by their last signature."""
    sizes = [3, 32, 0, 33, 5, 64, 65, 5000, 1, 5000, 31, 7]
    c = random_case(seed, len(sizes), stride, with_class, sizes=sizes, composite_every=0, p_valid=0.9)
    first = c.checks["first_sig"].astype(np.int64)
    rng = np.random.default_rng(seed + 1)
    for t, at in ((7, 4999), (9, 0)):
        c.status[first[t]:first[t] + 5000] = B.VALID
        c.status[first[t] + at] = B.INVALID if t == 7 else B.NOT_RUN
    for t in (3, 5, 6, 7, 9):  # a class only the span's last signature has, required by a leaf and a 1-of-2
        n = sizes[t]
        k = len(c.keys) - 1 - (t % 3)
        c.sigs["key_idx"][first[t]:first[t] + n] = rng.integers(0, 8, n)
        c.sigs["key_idx"][first[t] + n - 1] = k
    return c


def chain(nd, depth, cls):
    """A root with `depth` nested 1-of-2 composites above a leaf of class `cls`; returns the root index."""
    root = nd.block(1)
    at = root
    for _ in range(depth):
        first = nd.block(2)
        nd.rows[at] = [first, 2, 1, 1]
        nd.rows[first + 1] = [cls + 1000, 0, 1, 0]
        at = first
    nd.rows[at] = [cls, 0, 1, 0]
    return root


def hostile_case(stride, with_class, budget_dag=False, reserved=False):
    """Malformed and borderline tables, one transaction each (names in .names): a child index <= its
    parent's, a child range past the node table, root indices out of range, spans past the table, a
    foreign tx_idx inside a span, a requirement range past reqs, a key index past the key table,
    composites nested 8 (evaluated) and 9 deep (CG_REQ_HOST), n_missing saturation, no signatures, no
    requirements; with budget_dag the shared-subtree DAG whose paths exceed the visit budget (CPU
    only); with reserved a cg_tx_check with reserved != 0 (rejected by the host entry points)."""
    rng = np.random.default_rng(5)
    n_keys = 8
    keys = _keys(rng, n_keys)
    key_class = (np.arange(n_keys) // 2).astype(np.uint32) if with_class else None
    cls0 = 0  # the class of key 0
    nd = Nodes()
    leaf_ok, leaf_no = nd.leaf(cls0), nd.leaf(999)
    self_ref = nd.block(1)
    nd.rows[self_ref] = [self_ref, 2, 0, 1]
    back_ref = nd.block(1)
    nd.rows[back_ref] = [leaf_ok, 2, 0, 1]
    deep8, deep9 = chain(nd, 8, cls0), chain(nd, 9, cls0)
    inner_bad = nd.block(1)  # a good root whose second child points backwards
    b = nd.block(2)
    nd.rows[inner_bad] = [b, 2, 0, 1]
    nd.rows[b] = [cls0, 0, 1, 0]
    nd.rows[b + 1] = [leaf_ok, 1, 1, 1]
    wrap = nd.block(1)  # INT_MAX + INT_MAX + 1 wraps to -1... and two INT_MAX to -2: below a threshold of 1
    b = nd.block(2)
    nd.rows[wrap] = [b, 2, 0, 1]
    nd.rows[b] = [cls0, 0, INT_MAX, 0]
    nd.rows[b + 1] = [cls0, 0, INT_MAX, 0]
    dag = None
    if budget_dag:  # 7 levels of 4 nodes, each node's children the whole next level: 4^7 paths to the leaves
        dag = nd.block(1)
        level = nd.block(4)
        nd.rows[dag] = [level, 4, 0, 1]
        for _ in range(6):
            nxt = nd.block(4)
            for j in range(4):
                nd.rows[level + j] = [nxt, 4, 1, 1]
            level = nxt
        for j in range(4):
            nd.rows[level + j] = [cls0, 0, 1, 0]
    past = nd.block(1)  # last: its child range runs past the table
    nd.rows[past] = [past + 1, 3, 0, 1]
    nodes = nd.array()
    n_nodes = len(nodes)

    names, tx_idx, key_idx, rows, reqs = [], [], [], [], []

    def tx(name, n_sigs, roots, first_sig=None, n_claim=None, first_req=None, n_req=None, res=0):
        t = len(rows)
        names.append(name)
        fs = len(tx_idx) if first_sig is None else first_sig
        tx_idx.extend([t] * n_sigs)
        key_idx.extend([0] * n_sigs)
        fr = len(reqs) if first_req is None else first_req
        reqs.extend(roots)
        rows.append((fs, n_sigs if n_claim is None else n_claim, fr, len(roots) if n_req is None else n_req, res))
        return t

    tx("plain", 2, [leaf_ok, leaf_no, deep8])
    tx("child index equal to its parent", 1, [self_ref, leaf_ok])
    tx("child index below its parent", 1, [back_ref])
    tx("child range past the node table", 1, [past, leaf_ok])
    tx("backward child inside a good root", 1, [inner_bad])
    tx("root out of range", 1, [n_nodes, 0xFFFFFFFF, leaf_ok])
    tx("nested 9 deep", 1, [deep9, deep8])
    tx("weights wrap", 1, [wrap])
    tx("no signatures", 0, [leaf_ok, deep8])
    tx("no requirements", 3, [])
    t = tx("foreign tx_idx", 3, [leaf_ok])
    tx_idx[-2] = t + 1
    tx("key index past the key table", 2, [leaf_ok, leaf_no])
    key_idx[-1], key_idx[-2] = n_keys, 0xFFFFFFFF
    tx("saturation", 1, [leaf_no] * 70000 + [leaf_ok])
    if budget_dag:
        tx("visit budget", 1, [dag, leaf_ok])
    if reserved:
        tx("reserved not zero", 1, [leaf_ok], res=1)
    tx("span past the table", 0, [leaf_ok], first_sig=len(tx_idx) - 1, n_claim=5)
    tx("span far past the table", 0, [leaf_ok], first_sig=2**63, n_claim=0xFFFFFFFF)
    tx("span start past the table", 0, [leaf_ok], first_sig=2**64 - 1, n_claim=0)
    tx("requirement range past reqs", 1, [], first_req=len(reqs) - 1, n_req=3)
    tx("requirement range far past reqs", 1, [], first_req=0xFFFFFFFF, n_req=0xFFFFFFFF)
    checks = np.array(rows, dtype=B.TX_CHECK_DTYPE)
    status = np.zeros(len(tx_idx), np.uint8)
    status[1] = B.EMPTY
    c = case(_sig_table(stride, np.array(tx_idx, np.uint32), np.array(key_idx, np.uint32)), status, keys, key_class,
             checks, np.array(reqs, np.uint32), nodes, names=names)
    return c


def assert_same(got, want, names=None, what=""):
    gv, gr = got[0], got[1]
    wv, wr = want[0], want[1]
    bad = [t for t in range(len(wv)) if gv[t] != wv[t]]
    assert not bad, f"{what}: verdicts differ at {[(t, names[t] if names else '', gv[t], wv[t]) for t in bad[:5]]}"
    diff = np.flatnonzero(gr != wr)
    assert diff.size == 0, f"{what}: req_status differs at {diff[:10]}: {gr[diff[:10]]} != {wr[diff[:10]]}"
