"""A happens-before audit of the device launch schedule (corda_amd/csrc/launch_schedule.h), on the CPU.

tests/native/launch_schedule_test.cpp runs exactly the template verify.hip and cordagpu.cpp run, inside
call_scope.h's call scope, over a backend that logs every event record, stream wait and stage. This
file builds happens-before from a log and checks it against ACCESS, which says what each stage reads
and writes:
  * ops on one stream are ordered by enqueue order;
  * a wait binds to the latest record of its event enqueued before it (the events are reused per
    chunk): everything before that record precedes everything behind the wait on the waiting stream;
  * a wait for an event never recorded in the log is a no-op, as in HIP, and is reported.
The reference is single-stream execution in enqueue order:
  a. two ops that touch one resource instance, at least one writing, are ordered in enqueue order;
  b. every op on a side stream happens-before the call's `rec(done,M)`;
  c. a over a call boundary: the next call starts behind `wait(M,done)` only, and the caller's
     stream touches its buffers behind `wait(C,done)` only.
Streams: M the context's own, S0 S1 S2 its side streams (families r1, k1, ed), C the caller's.
Tokens: rec(event,stream), wait(stream,event), stage@stream, stage@stream[chunk/half].

What this cannot see: races inside one kernel, the host forms' copy-stream feed (the hooks are opaque
stages on M), error exits, and a row of ACCESS that is wrong about its kernel."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "corda_amd", "csrc")
SO = os.path.join(HERE, "native", "liblaunchscheduletest.so")
FAM = ("r1", "k1", "ed")
MODES = ("row0", "full", "wide")  # an item's table mode (quarter tables go with row 0: same stage)


# ---------------------------------------------------------------------------- the driver

def _lib():
    src = os.path.join(HERE, "native", "launch_schedule_test.cpp")
    deps = [src, os.path.join(CSRC, "launch_schedule.h"), os.path.join(CSRC, "call_scope.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO, src])
    L = ctypes.CDLL(SO)
    L.ls_run.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint]
    L.ls_stages.argtypes = [ctypes.c_char_p, ctypes.c_uint]
    return L


_LOGS = {}


def run(spec):
    if spec not in _LOGS:
        buf = ctypes.create_string_buffer(1 << 16)
        assert _lib().ls_run(spec.encode(), buf, len(buf)) == 0, spec
        _LOGS[spec] = buf.value.decode().strip()
    return _LOGS[spec]


def stages():
    buf = ctypes.create_string_buffer(1 << 12)
    assert _lib().ls_stages(buf, len(buf)) == 0
    return buf.value.decode().split()


# ---------------------------------------------------------------------------- the access table
# stage: (kernels, reads, writes, atomics). {c} the op's chunk, {h} its item workspace, {C} every
# chunk of the log, {f} / {m} every family / table mode. An atomic update commutes with another
# atomic update of the same resource and conflicts with a read or a write of it.
#
#   uses                uses / seen per key              wide_idx     a wide key's slot
#   list.<l>.<f>        the full / row0 / quart / wide list of class f with its count
#   skip_word           the SKIP_MISMATCH_AT word
#   hdr.status.<f>      the key headers of family f (EdKeyHdr but abyte)    hdr.abyte   Ed25519 Abyte
#   bases.<f> tab.<f> park.<f>   row bases, row tables and the builds' park, of family f's keys
#   wslot.<f>           the wide-pool slots of family f's keys (the ECDSA pool is split by key)
#   kc.index kc.own.<f> kc.ctr   the wide-table cache: index, owners / live / free list, counters
#   h<h>.perm .sort .slots.<f>.<m> .edcols.<m>   item workspace h: perm and ranges, the sort
#                       buffers, the per-item slots and the Ed25519 columns (both by plan position,
#                       so a family's and a mode's items never share one)
#   items.c<c> arena.c<c> msgs.c<c>   chunk c's verify items, signature / message bytes, spliced messages
#   st.c<c>.<f>.<m> st.c<c>.other   chunk c's status bytes, by the stage that gives the verdict
#   keys arena.keys sigtab   the caller's key table, key bytes and signature table
#   rsakeys rsalist     the RSA workspace

def _fam_rows(name, f):
    ec = f != "ed"
    k = "ec" if ec else "ed"
    rows = {
        "chains": (f"k_{k}_keyprep_decode k_{k}_keyprep_chain k_{k}_wide_chain",
                   f"keys arena.keys list.full.{f} list.quart.{f} list.wide.{f} wide_idx",
                   f"hdr.status.{f} bases.{f} wslot.{f}", ""),
        "wide_tabs": (f"k_{k}_wide_rows k_kc_commit",
                      f"hdr.status.{f} list.wide.{f} wide_idx wslot.{f}", f"wslot.{f} kc.own.{f}", "kc.ctr"),
        "full_tabs": (f"k_{k}_keyprep_tab",
                      f"hdr.status.{f} bases.{f} list.row0.{f} list.full.{f} list.quart.{f} park.{f}",
                      f"tab.{f} park.{f}", ""),
        "row0_ladder": (f"k_{k}_ladder<ROW0> k_{k}_ladder<QUART>", f"tab.{f}", "", ""),
        "full_ladder": (f"k_ec_ladder<FULL>" if ec else "k_ed_ladder_pf", f"tab.{f}", "", ""),
        "wide_ladder": (f"k_{k}_ladder_wide", f"wide_idx wslot.{f}", "", ""),
    }
    kern, r, w, a = rows[name]
    if name.endswith("ladder"):
        m = name.split("_")[0]
        own = f"st.c{{c}}.{f}.{m} h{{h}}.slots.{f}.{m}" + ("" if ec else f" h{{h}}.edcols.{m}")
        r += f" items.c{{c}} h{{h}}.perm hdr.status.{f} " + own
        w = own
    return kern, r, w, a


ACCESS = {
    "key_init": ("k_key_init", "", "uses wide_idx list.full.{f} list.row0.{f} list.quart.{f} list.wide.{f} skip_word", ""),
    "key_uses": ("k_key_uses", "items.c{C}", "uses", ""),
    "key_counts": ("k_key_counts", "", "uses", ""),
    "key_uses_txsig": ("k_key_uses_txsig", "sigtab", "uses", ""),
    "kc_begin": ("k_kc_begin", "", "kc.index kc.own.{f} kc.ctr", ""),
    "key_classify": ("k_key_classify", "keys arena.keys uses kc.index kc.own.{f}",
                     "uses wide_idx list.full.{f} list.row0.{f} list.quart.{f} list.wide.{f} kc.own.{f}",
                     "skip_word kc.ctr"),
    "kc_claim": ("k_kc_claim", "keys arena.keys kc.own.{f} list.wide.{f}",
                 "wide_idx kc.own.{f} list.wide.{f} list.full.{f} list.row0.{f}", "skip_word kc.ctr"),
    "ed_abyte": ("k_ed_key_abyte", "keys arena.keys", "hdr.abyte", ""),
    "misc_status": ("k_misc_status", "items.c{c} keys", "st.c{c}.{f}.{m} st.c{c}.other", ""),
    "plan": ("launch_plan (k_plan_*, the radix sort)", "items.c{c} keys uses wide_idx h{h}.sort",
             "h{h}.sort h{h}.perm", ""),
    "ed_front": ("k_ed_hash", "items.c{c} h{h}.perm hdr.abyte arena.c{c} msgs.c{c} st.c{c}.ed.{m}",
                 "st.c{c}.ed.{m} h{h}.slots.ed.{m} h{h}.edcols.{m}", ""),
    "ed_finish": ("k_ed_finish", "h{h}.perm h{h}.slots.ed.{m} h{h}.edcols.{m} st.c{c}.ed.{m}", "st.c{c}.ed.{m}", ""),
    "mode_guard": ("k_mode_guard", "h{h}.perm skip_word", "st.c{c}.{f}.row0 st.c{c}.{f}.full", ""),
    "rsa_keyprep": ("k_rsa_keyprep", "keys arena.keys", "rsakeys", ""),
    "rsa_items": ("launch_rsa_items", "items.c{C} keys arena.c{C} msgs.c{C} rsakeys rsalist st.c{C}.other",
                  "rsalist st.c{C}.other", ""),
    # the tx-signature forms' hooks, opaque: chunk c's items and spliced messages are made from the
    # signature table; the blocking form's second half lands the chunk's signature bytes
    "prepare_hook": ("launch_tx_sig_range / launch_tx_sig12_range", "sigtab", "items.c{c} msgs.c{c}", ""),
    "mid_hook": ("TxsigFeed::mid", "", "arena.c{c}", ""),
    # the caller's stream: its buffers written ahead of a call; rewritten, and the verdicts read, behind it
    "caller_fill": ("(the caller)", "", "keys arena.keys sigtab items.c{C} arena.c{C} st.c{C}.{f}.{m} st.c{C}.other", ""),
    "caller_reuse": ("(the caller)", "st.c{C}.{f}.{m} st.c{C}.other", "keys arena.keys sigtab items.c{C} arena.c{C}", ""),
}
for _f in FAM:
    for _n in ("chains", "wide_tabs", "full_tabs", "row0_ladder", "full_ladder", "wide_ladder"):
        ACCESS[f"{_n}_{_f}"] = _fam_rows(_n, _f)
for _f in ("r1", "k1"):
    _own = f"st.c{{c}}.{_f}.{{m}}"
    ACCESS[f"ec_front_{_f}"] = ("k_ec_prep k_ec_inv",
                                f"items.c{{c}} h{{h}}.perm hdr.status.{_f} arena.c{{c}} msgs.c{{c}} " + _own,
                                _own + f" h{{h}}.slots.{_f}.{{m}}", "")


def expand(pattern, chunk, half, chunks):
    """The resource instances a table entry names for one op."""
    out = set()
    for word in pattern.split():
        words = [word]
        for key, vals in (("{f}", FAM), ("{m}", MODES), ("{C}", [str(c) for c in chunks])):
            words = [w.replace(key, v) for w in words for v in (vals if key in w else [""])]
        for w in words:
            out.add(w.replace("{c}", str(chunk)).replace("{h}", str(half)))
    return out


# ---------------------------------------------------------------------------- happens-before

TOKEN = re.compile(r"(rec|wait)\((\w+),(\w+)\)$|(\w+)@(\w+)(?:\[(-?\d+)/(-?\d+)\])?$")
STREAMS = ("M", "S0", "S1", "S2", "C")


def parse(log):
    ops = []
    for t in log.split():
        m = TOKEN.match(t)
        assert m, t
        if m.group(1) == "rec":
            ops.append(("rec", m.group(3), m.group(2)))          # (kind, stream, event)
        elif m.group(1) == "wait":
            ops.append(("wait", m.group(2), m.group(3)))
        else:
            ops.append(("run", m.group(5), m.group(4), int(m.group(6) or -1), int(m.group(7) or -1)))
    return ops


def audit(log, access=None):
    """(violations, unrecorded waits) of one log. A violation is a short string."""
    access = access or ACCESS
    ops = parse(log)
    chunks = sorted({o[3] for o in ops if o[0] == "run" and o[3] >= 0}) or [0]
    now = {s: dict.fromkeys(STREAMS, 0) for s in STREAMS}  # per stream: the latest op of each stream it is behind
    recorded, unrecorded, bad = {}, [], []
    touched = {}  # resource -> [(op index, stream, clock on its own stream, mode)]
    side_ops = []  # (index, stream, own clock) of the current call's side-stream ops
    for i, o in enumerate(ops, 1):
        s = o[1]
        clock = now[s]
        clock[s] = i
        if o[0] == "rec":
            recorded[o[2]] = dict(clock)
            if o[2] == "done":  # b: the call ends here
                bad += [f"b: {ops[j - 1][2]}@{t} not joined before rec(done,M)" for j, t in side_ops if clock[t] < j]
                side_ops = []
        elif o[0] == "wait":
            if o[2] not in recorded:
                unrecorded.append((s, o[2]))
            else:
                for t, v in recorded[o[2]].items():
                    clock[t] = max(clock[t], v)
        else:
            if s in ("S0", "S1", "S2"):
                side_ops.append((i, s))
            _, r, w, a = access[o[2]]
            mine = {}
            for mode, pat in (("r", r), ("a", a), ("w", w)):
                for res in expand(pat, o[3], o[4], chunks):
                    mine[res] = mode  # w over a over r
            for res, mode in mine.items():
                for j, t, other in touched.get(res, ()):
                    if (mode == "r" and other == "r") or (mode == "a" and other == "a"):
                        continue
                    if clock[t] < j:
                        bad.append(f"a: {res}: {ops[j - 1][2]}@{t} ({other}) is not ordered before {o[2]}@{s} ({mode})")
                touched.setdefault(res, []).append((i, s, mode))
    return bad, unrecorded


# ---------------------------------------------------------------------------- the shapes

ORDERS = [dict(chunks=c, two=t, hook=h) for c in (1, 2, 3, 4) for t in (0, 1) for h in (0, 1, 2)]
KEY_CONFIGS = ([dict(skip=s) for s in range(8)] +
               [dict(wed=a, wec=b, cache=c) for a in (0, 1) for b in (0, 1) for c in (0, 1) if a or b or not c] +
               [dict(wed=1, wec=1, cache=1, skip=5), dict(rsa=1), dict(rsa=1, wed=1, wec=1, cache=1, skip=2), dict(keys=0)])


def verify_spec(order, cfg):
    d = dict(order, **cfg)
    # a hook's key uses come from the signature table (device forms) or the host's counts (host forms)
    d.setdefault("uses", {0: "items", 1: "txsig", 2: "counts"}[d["hook"]])
    return "verify " + " ".join(f"{k}={v}" for k, v in sorted(d.items()))


def single_call_specs():
    for order, cfg in itertools.product(ORDERS, KEY_CONFIGS):
        yield "fill; " + verify_spec(order, cfg) + "; reuse"
    for keys, rsa in itertools.product((0, 1), (0, 1)):
        yield f"fill; prepare keys={keys} rsa={rsa}; reuse"


HEADLINE = dict(chunks=2, two=1, hook=1, wed=1, wec=1, cache=1)


def two_call_specs():
    prep = ["prepare", "prepare rsa=1"]
    items = ["items chunks=1", "items chunks=2", "items chunks=3 rsa=1"]
    ver = [verify_spec(o, c) for o, c in ((HEADLINE, {}), (dict(chunks=1, two=0, hook=0), dict(skip=3)),
                                          (dict(chunks=3, two=0, hook=2), dict(wed=1, wec=1, cache=1)),
                                          (dict(chunks=3, two=1, hook=0), dict(rsa=1)))]
    for a, b in itertools.chain(itertools.product(prep, prep + items + ver), itertools.product(ver, ver + prep)):
        yield f"fill; {a}; reuse; fill; {b}; reuse"
    for p in prep:  # one caller, no pause: prepare A, prepare B, overwrite the key bytes, verify B's items
        yield f"fill; {p}; {p}; reuse; items chunks=2; reuse"


def all_specs():
    return list(single_call_specs()) + list(two_call_specs())


def sweep(prefix="", access=None, first_only=False):
    """spec -> violations over every shape with any."""
    found = {}
    for spec in all_specs():
        bad, _ = audit(run(prefix + spec), access)
        if bad:
            found[spec] = bad
            if first_only:
                break
    return found


# ---------------------------------------------------------------------------- the tests

def test_the_header_has_no_hip_in_it():
    src = open(os.path.join(CSRC, "launch_schedule.h")).read()
    assert "#include" not in src and not re.search(r"hip[A-Z_]|__global__|<<<", src)


def test_every_stage_has_a_row_and_every_resource_a_writer_and_a_reader():
    assert set(stages()) == set(ACCESS) - {"caller_fill", "caller_reuse"}
    read, written = set(), set()
    for kern, r, w, a in ACCESS.values():
        assert kern
        read |= expand(r + " " + a, 0, 0, [0])
        written |= expand(w + " " + a, 0, 0, [0])
    assert read == written, sorted(read ^ written)
    emitted = {o[2] for spec in all_specs() for o in parse(run(spec)) if o[0] == "run"}
    assert emitted == set(ACCESS), sorted(emitted ^ set(ACCESS))  # the shapes reach every stage


def test_no_two_conflicting_stages_are_unordered_and_every_call_joins_its_side_streams():
    """Invariants a, b and c over every shape."""
    specs = all_specs()
    assert 300 < len(specs) < 1000
    found = sweep()
    assert not found, "\n".join(f"{s}\n  " + "\n  ".join(b[:6]) for s, b in list(found.items())[:5])


def test_waits_for_events_never_recorded_are_the_known_ones():
    """HIP makes a wait for a never-recorded event a no-op: only a call without keys has any (its
    backs wait for table builds that nothing started), and a context whose first call is
    cg_verify_items_device would (the library refuses that call)."""
    tables = [("M", "ready2"), ("M", "ready0"), ("M", "ready1")]
    for spec in all_specs():
        _, unrecorded = audit(run(spec))
        if "keys=0" in spec and "verify" in spec:
            nch = int(re.search(r"chunks=(\d)", spec).group(1))
            assert unrecorded == tables * nch, spec
        else:
            assert unrecorded == [], (spec, unrecorded)
    assert audit(run("items chunks=1"))[1] == tables


# A wait the audit does not need, and why. Every other wait the schedule makes is load-bearing: the
# audit reports a violation in some shape when the fake leaves it out.
REDUNDANT = {
    # one caller stream, bridged: wait(C,done), rec(bridge,C), wait(M,bridge) imply it, and M's own order
    # does; it orders calls that run on different streams (bridge off: tests/test_call_scope.py)
    ("M", "done"): "implied by M's own order and by the bridge behind wait(C,done)",
    # the builds need their family's chains (same stream) and the classification (start); `planned`
    # places them behind the first plan sort for speed (its look-back stalls behind the builds)
    ("S0", "planned"): "scheduling: the builds follow the chains on S0, which are behind start",
    ("S1", "planned"): "scheduling: the builds follow the chains on S1, which are behind start",
    ("S2", "planned"): "scheduling: the builds follow the chains on S2, which are behind start",
    # a curve's row-0 ladders need the chunk's plan from M (ec_go, ahead of the curve's front on the
    # same stream) and nothing of the Ed25519 hashes; S2's wait for `front` is needed
    ("S0", "front"): "implied by wait(S0,ec_go) of the same chunk's front",
    ("S1", "front"): "implied by wait(S1,ec_go) of the same chunk's front",
}


def emitted_waits():
    return sorted({(o[1], o[2]) for spec in all_specs() for o in parse(run(spec)) if o[0] == "wait"})


def test_every_wait_is_needed_or_explained():
    waits = emitted_waits()
    assert len(waits) >= 20
    unexplained, wrongly_listed = [], []
    for s, e in waits:
        needed = bool(sweep(prefix=f"drop {s}:{e}; ", first_only=True))
        if not needed and (s, e) not in REDUNDANT:
            unexplained.append((s, e))
        if needed and (s, e) in REDUNDANT:
            wrongly_listed.append((s, e))
    assert not unexplained, f"the audit passes without these waits: {unexplained}"
    assert not wrongly_listed, wrongly_listed
    assert set(REDUNDANT) <= set(waits)


def _edited(stage, reads="", writes=""):
    t = dict(ACCESS)
    kern, r, w, a = t[stage]
    t[stage] = (kern, r + " " + reads, w + " " + writes, a)
    return t


@pytest.mark.parametrize("name,table,expect", [
    # the hashes read the decode's status beside Abyte: they run beside the decode
    ("a read", lambda: _edited("ed_front", reads="hdr.status.ed"), "hdr.status.ed: chains_ed@S2 (w) is not ordered before ed_front@M"),
    # Abyte clears the status word it does not own
    ("a write", lambda: _edited("ed_abyte", writes="hdr.status.ed"), "hdr.status.ed: chains_ed@S2 (w) is not ordered before ed_abyte@M"),
    # the plan sorts into the other item workspace, under the other chunk's fronts
    ("the wrong half", lambda: {**ACCESS, "plan": (ACCESS["plan"][0], ACCESS["plan"][1],
                                                   ACCESS["plan"][2].replace("h{h}.perm", "h{h}.perm h0.perm h1.perm"), "")},
     "h0.perm: ec_front_r1@S0 (r) is not ordered before plan@M (w)"),
])
def test_a_wrong_table_row_is_caught(name, table, expect):
    found = sweep(access=table())
    assert any(expect in b for bad in found.values() for b in bad), (name, list(found.items())[:2])


# ---------------------------------------------------------------------------- the pinned logs
# Written down from launch_keyprep, launch_pending_tabs, launch_items_plan / _front / _back
# (verify.hip), launch_chunked, cg_prepare_keys_device and cg_verify_items_device (cordagpu.cpp) as
# they were before the schedule moved into the template. A change of the schedule shows up here.

def FRONT(k, h, mid=""):
    return (f"{mid}rec(ec_go,M) wait(S0,ec_go) ec_front_r1@S0[{k}/{h}] rec(ec_done0,S0) wait(S1,ec_go) "
            f"ec_front_k1@S1[{k}/{h}] rec(ec_done1,S1) ed_front@M[{k}/{h}] ")


def PLAN(k, h):
    return f"misc_status@M[{k}/{h}] plan@M[{k}/{h}] "


def BACK(k, h, wide=True):
    c = f"[{k}/{h}]"
    return (f"rec(front,M) wait(S0,front) wait(S1,front) wait(S2,front) row0_ladder_ed@S2{c} row0_ladder_r1@S0{c} "
            f"row0_ladder_k1@S1{c} rec(row0_0,S0) rec(row0_1,S1) rec(row0_2,S2) wait(M,ready2) full_ladder_ed@M{c} " +
            (f"wide_ladder_ed@M{c} " if wide else "") +
            f"rec(front,M) wait(S2,front) ed_finish@S2{c} rec(row0_2,S2) wait(M,ready0) wait(M,ec_done0) "
            f"full_ladder_r1@M{c} " + (f"wide_ladder_r1@M{c} " if wide else "") +
            f"wait(M,ready1) wait(M,ec_done1) full_ladder_k1@M{c} " + (f"wide_ladder_k1@M{c} " if wide else "") +
            "wait(M,row0_0) wait(M,row0_1) wait(M,row0_2) ")


def TABS(wide=True):
    return "rec(planned,M) " + "".join(
        f"wait(S{k},planned) " + (f"wide_tabs_{FAM[k]}@S{k} " if wide else "") + f"full_tabs_{FAM[k]}@S{k} rec(ready{k},S{k}) "
        for k in (2, 0, 1))


FORK = "rec(start,M) wait(S0,start) wait(S1,start) wait(S2,start) chains_r1@S0 chains_k1@S1 chains_ed@S2 "
OPEN, CLOSE = "rec(bridge,C) wait(M,bridge) ", "rec(done,M) wait(C,done)"
PREPARE_PARENT = OPEN + "key_init@M key_classify@M " + FORK + TABS(wide=False) + "ed_abyte@M "
JOIN = "wait(M,ready0) wait(M,ready1) wait(M,ready2) "  # the fix: a prepare call ends behind its table builds
ITEMS_1 = OPEN + "wait(M,done) " + PLAN(0, 0) + FRONT(0, 0) + BACK(0, 0, wide=False) + CLOSE

PINNED = {
    # cg_verify_tx_signatures_packed_device: 2 chunks, two workspaces, all families, both pools, cache on
    verify_spec(HEADLINE, {}): (
        OPEN + "key_init@M key_uses_txsig@M kc_begin@M key_classify@M kc_claim@M " + FORK + "ed_abyte@M " +
        "prepare_hook@M[0/-1] " + PLAN(0, 0) + TABS() + FRONT(0, 0) + "prepare_hook@M[1/-1] " + PLAN(1, 1) + FRONT(1, 1) +
        BACK(0, 0) + BACK(1, 1) + CLOSE),
    # the same call as cg_verify_batch_device makes it: both plans sort ahead of the table builds
    verify_spec(dict(HEADLINE, hook=0), {}): (
        OPEN + "key_init@M key_uses@M kc_begin@M key_classify@M kc_claim@M " + FORK + "ed_abyte@M " +
        PLAN(0, 0) + PLAN(1, 1) + TABS() + FRONT(0, 0) + FRONT(1, 1) + BACK(0, 0) + BACK(1, 1) + CLOSE),
    # cg_verify_tx_signatures (host form, blocking hook): the builds start first, front k, back k
    verify_spec(dict(HEADLINE, hook=2), {}): (
        OPEN + "key_init@M key_counts@M kc_begin@M key_classify@M kc_claim@M " + FORK + "ed_abyte@M " + TABS() +
        "prepare_hook@M[0/-1] " + PLAN(0, 0) + FRONT(0, 0, "mid_hook@M[0/0] ") + BACK(0, 0) +
        "prepare_hook@M[1/-1] " + PLAN(1, 1) + FRONT(1, 1, "mid_hook@M[1/1] ") + BACK(1, 1) + CLOSE),
    # cg_prepare_keys_device + cg_verify_items_device, as the parent enqueued them and as they are now
    "prepare join=0; items chunks=1": PREPARE_PARENT + CLOSE + " " + ITEMS_1,
    "prepare; items chunks=1": PREPARE_PARENT + JOIN + CLOSE + " " + ITEMS_1,
}


@pytest.mark.parametrize("spec", sorted(PINNED))
def test_the_schedule_is_the_pinned_one(spec):
    assert run(spec) == PINNED[spec]


def test_the_parent_prepare_call_left_its_side_streams_unjoined():
    """What the audit found: cg_prepare_keys_device recorded `done` on M with the decodes, chains and
    table builds still on the side streams. Behind `done` alone the caller could rewrite the key bytes
    under the decodes, and the next call's k_key_init the lists under the builds."""
    bad, _ = audit(run("fill; prepare join=0; reuse; fill; prepare join=0; reuse"))
    text = "\n".join(bad)
    assert "b: chains_ed@S2 not joined before rec(done,M)" in text
    assert "a: arena.keys: chains_ed@S2 (r) is not ordered before caller_reuse@C (w)" in text
    assert "a: list.full.ed: full_tabs_ed@S2 (r) is not ordered before key_init@M (w)" in text
    assert audit(run("fill; prepare; reuse; fill; prepare; reuse")) == ([], [])
