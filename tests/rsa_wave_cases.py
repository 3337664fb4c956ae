"""Crafted operands for the lane-cooperative RSA primitives (corda_amd/csrc/rsa_wave.h), made at run
time from a fixed seed: tests/test_rsa_wave_model.py proves on the CPU, with tests/rsa_wave_model.py,
which path each case takes, and tests/test_gpu_rsa_wave.py runs the same cases on the device. The
expected value of every case is Python integer arithmetic.

A product whose result y has a run of zero limbs reaches the ballot ripple of rsa_resolve: with
a = y u mod n and b = u^-1 R mod n the Montgomery product is y (or y + n before the subtraction), and
a limb that ends up zero under a carry-in either generates or propagates. Which of the two a given
lane does depends on how the deferred carries happen to fall, so each class draws a few candidates
(other u, other filler limbs) and keeps the first one the model shows to reach the class's event; a
class none of whose candidates reaches it is an error.

Sizes: L in 32, 33, 63, 64 (one limb per lane) and 65, 96, 127, 128 (two). Moduli per size: see moduli().
"""
import functools
import math
import random

import rsa_wave_model as M

SIZES = (32, 33, 63, 64, 65, 96, 127, 128)
MODULI = ("random", "top1", "topff", "allones", "2^B-c", "2^(B-1)+c")
EXPONENTS = (1, 2, 3, 4, 6, 0x10000, 65537, 0x80000001, 0xFFFFFFFF)
MODEXP_MODULI = ("random", "2^B-c")
N_CONTROLS = 64
CANDIDATES = 40
SEED = 0x52A7E


def moduli(L, rng):
    B = 32 * L
    low = lambda: rng.getrandbits(B - 32) | 1  # noqa: E731
    c = rng.getrandbits(16) | 1
    return {"random": (rng.randrange(1, 1 << 32) << (B - 32)) | low(),
            "top1": (1 << (B - 32)) | low(),
            "topff": (0xFFFFFFFF << (B - 32)) | low(),
            "allones": (1 << B) - 1,
            "2^B-c": (1 << B) - c,
            "2^(B-1)+c": (1 << (B - 1)) + c}


def _set_limbs(y, start, count, value):
    for i in range(start, start + count):
        y = (y & ~(0xFFFFFFFF << (32 * i))) | (value << (32 * i))
    return y


def _below(y, n, L):
    return y if y < n else y & ((1 << (32 * (L - 1))) - 1)


class _Units:
    """u and u^-1 mod n, a fresh pair per call from one modular inversion per modulus."""

    def __init__(self, n, L, rng):
        while True:
            g = rng.randrange(2, n)
            if math.gcd(g, n) == 1:
                break
        self.n, self.R, self.g, self.gi = n, 1 << (32 * L), g, pow(g, -1, n)
        self.u, self.ui = g, self.gi

    def operands(self, y):
        """(a, b) whose Montgomery product is y."""
        self.u, self.ui = self.u * self.g % self.n, self.ui * self.gi % self.n
        return y * self.u % self.n, self.ui * self.R % self.n


def _start(L, K, length, half, rng):
    """A first limb for a run of `length` limbs that stays clear of limb 0 and limb L - 1; at K = 2 on
    the lower (half 0) or upper (half 1) limb of its lane."""
    i = rng.randrange(2, L - length - 1)
    if K == 2 and i % 2 != half:
        i += 1 if i + 1 < L - length - 1 else -1
    return i


# the classes of one (size, modulus): name -> (candidates maker, event predicate, the event in words)
def _mont_classes(L, mod, n, rng):
    K = M.k_of(L)
    full = L in (64, 128)  # lane 63 holds limbs below L: an overflow shows in `top`, not in `hi`
    out = {}
    units = _Units(n, L, rng)

    def zero_run(length, half):
        def make():
            y = _set_limbs(rng.randrange(n), _start(L, K, length, half, rng), length, 0)
            return units.operands(y) + (y,)
        return make

    def end_run():
        y = rng.randrange(n) & ((1 << (32 * (L - 6))) - 1)
        return units.operands(y) + (y,)

    def ones_run():
        y = _below(_set_limbs(rng.randrange(n), _start(L, K, 8, 0, rng), 8, 0xFFFFFFFF), n, L)
        return units.operands(y) + (y,)

    def near_n():
        a, b = n - 1 - rng.getrandbits(64), n - 1 - rng.getrandbits(64)
        return a, b, None

    gen = lambda e: e["gen"] >= 1  # noqa: E731
    gen_prop = lambda e: e["gen"] >= 1 and e["cprop"] >= 1  # noqa: E731
    inside = lambda e: e["gen"] == 0 and e["cprop"] == 0  # noqa: E731
    if K == 1:
        out["zero_run_1"] = (zero_run(1, 0), gen, "a lane generates")
        out["zero_run_2"] = (zero_run(2, 0), gen_prop, "a lane generates, the next propagates the carry")
        out["zero_run_16"] = (zero_run(16, 0), lambda e: e["gen"] >= 1 and e["chain"] >= 8,
                              "a chain of at least 8 propagating lanes")
    else:
        # two limbs per lane: a lane generates only when both of its limbs end up zero (or the lower one
        # below the carry-in); a one-limb run, and a two-limb run across two lanes, is absorbed inside
        # the lanes and must leave the ballots empty
        out["zero_run_1_lower"] = (zero_run(1, 0), inside, "absorbed inside the lane: no ballot event")
        out["zero_run_1_upper"] = (zero_run(1, 1), inside, "absorbed by the first pass: no ballot event")
        out["zero_run_2_lower"] = (zero_run(2, 0), gen, "both limbs of a lane zero: it generates")
        out["zero_run_2_upper"] = (zero_run(2, 1), inside, "a run across two lanes: no ballot event")
        out["zero_run_16_lower"] = (zero_run(16, 0), lambda e: e["gen"] >= 1 and e["chain"] >= 4,
                                    "a chain of at least 4 propagating lanes (8 limbs)")
        out["zero_run_16_upper"] = (zero_run(16, 1), lambda e: e["gen"] >= 1 and e["chain"] >= 4,
                                    "a chain of at least 4 propagating lanes, begun on an upper limb")
    out["zero_run_to_L-1"] = (end_run, gen_prop, "a chain that ends in the lane of limb L - 1")
    out["ones_run"] = (ones_run, lambda e: e["iprop"] >= 1, "lanes that propagate and receive no carry")
    if mod in ("topff", "allones", "2^B-c"):  # 2 n > 2^(32 L): elsewhere t < 2 n cannot reach it
        if full:
            out["over_top"] = (near_n, lambda e: e["sub"] >= 1 and e["top1"] + e["ripple_top"] >= 1,
                               "t >= 2^(32 L): the carry out of lane 63 (`top`)")
        else:
            out["over_hi"] = (near_n, lambda e: e["sub"] >= 1 and e["hi"] >= 1, "t >= 2^(32 L): a limb at or above L set")
    return out


def _pick(classes, run):
    """Draw CANDIDATES per class, run them as one model batch, keep the first that reaches its event."""
    cands = []
    for name, (make, pred, words) in classes.items():
        for _ in range(CANDIDATES):
            cands.append((name, make()))
    results, ev = run([c[1] for c in cands])
    chosen = []
    for name, (make, pred, words) in classes.items():
        for i, (cname, ops) in enumerate(cands):
            if cname == name and pred(ev.row(i)):
                chosen.append((name, ops, results[i], ev.row(i), words))
                break
        else:
            raise AssertionError(f"no candidate of class {name} reaches its event ({words})")
    return chosen


@functools.lru_cache(maxsize=None)
def build(modexp_model=True):
    """{"mont_mul": [...], "double_mod": [...], "geq": [...], "modexp": [...]}: each case a dict with
    name, L, mod, its operands, `want` (Python integers) and `model` / `ev` (the model's result and
    event record). modexp_model=False leaves the model out of the modexp cases (the slowest part: the
    device test needs the operands alone); the cases are the same either way."""
    rng = random.Random(SEED)
    mm, dm, gq, me = [], [], [], []
    for L in SIZES:
        K = M.k_of(L)
        R = 1 << (32 * L)
        mods = moduli(L, rng)
        for mod in MODULI:
            n = mods[mod]
            Rinv = pow(R, -1, n)
            # ---- mont_mul: the classes with an event, then a, b in {0, 1, n - 1}
            classes = _mont_classes(L, mod, n, rng)
            for name, (a, b, y), got, ev, words in _pick(
                    classes, lambda ops: M.run_mont_mul([o[0] for o in ops], [o[1] for o in ops], [n] * len(ops), L)):
                want = a * b * Rinv % n
                assert y is None or want == y
                mm.append({"name": name, "L": L, "mod": mod, "a": a, "b": b, "n": n, "want": want, "model": got,
                           "ev": ev, "event": words, "pred": classes[name][1]})
            edge = [(a, b) for a in (0, 1, n - 1) for b in (0, 1, n - 1)]
            got, ev = M.run_mont_mul([a for a, _ in edge], [b for _, b in edge], [n] * 9, L)
            for i, (a, b) in enumerate(edge):
                mm.append({"name": "edge_ab", "L": L, "mod": mod, "a": a, "b": b, "n": n, "want": a * b * Rinv % n,
                           "model": got[i], "ev": ev.row(i), "event": None, "pred": None})
            # ---- double_mod: 2 x = n + y with the top limbs of y zero, the edges, a few random x
            def chain_top():
                y = (rng.getrandbits(32 * (L - 6)) | 1)
                return ((n + y) // 2,)
            if mod in ("allones", "2^B-c"):  # the top limbs of n are all ones: 2 x = n + y passes 2^(32 L)
                full = L in (64, 128)
                dname, words = "over", "2 x >= 2^(32 L): " + ("the carry out of lane 63" if full else "a limb at or above L set")
                top_pred = (lambda e: e["sub"] >= 1 and e["top1"] >= 1) if full else (lambda e: e["sub"] >= 1 and e["hi"] >= 1)
            else:
                dname, words = "chain_into_top", "the subtraction's chain runs through the top lanes into `top`"
                top_pred = lambda e: e["sub"] >= 1 and e["ripple_top"] >= 1 and e["gen"] >= 1 and e["cprop"] >= 1  # noqa: E731
            for name, (x,), got, ev, _ in _pick({dname: (chain_top, top_pred, words)},
                                                lambda ops: M.run_double_mod([o[0] for o in ops], [n] * len(ops), L)):
                dm.append({"name": name, "L": L, "mod": mod, "x": x, "n": n, "want": 2 * x % n, "model": got, "ev": ev,
                           "event": words, "pred": top_pred})
            xs = [0, 1, n - 1, (n - 1) // 2, (n + 1) // 2] + [rng.randrange(n) for _ in range(8)]
            got, ev = M.run_double_mod(xs, [n] * len(xs), L)
            for i, x in enumerate(xs):
                dm.append({"name": "edge_x" if i < 5 else "random", "L": L, "mod": mod, "x": x, "n": n,
                           "want": 2 * x % n, "model": got[i], "ev": ev.row(i), "event": None, "pred": None})
        # ---- once per size: t == n, the largest accumulators, the random controls
        while True:
            p, q = (rng.getrandbits(16 * L) | (1 << (16 * L - 1)) | 1 for _ in range(2))
            if p != q:
                break
        n = p * q
        got, ev = M.run_mont_mul([p], [q], [n], L)
        mm.append({"name": "t_equals_n", "L": L, "mod": "p q", "a": p, "b": q, "n": n, "want": 0, "model": got[0],
                   "ev": ev.row(0), "event": "the subtraction taken on equality alone",
                   "pred": lambda e: e["sub_eq"] >= 1})
        n = R - 1
        got, ev = M.run_mont_mul([n - 1], [n - 1], [n], L)
        mm.append({"name": "largest_accumulator", "L": L, "mod": "allones", "a": n - 1, "b": n - 1, "n": n,
                   "want": (n - 1) * (n - 1) * pow(R, -1, n) % n, "model": got[0], "ev": ev.row(0),
                   "event": "every accumulator below 2^35", "pred": lambda e: e["max_acc"] < 1 << 35})
        n = mods["random"]
        ab = [(rng.randrange(n), rng.randrange(n)) for _ in range(N_CONTROLS)]
        got, ev = M.run_mont_mul([a for a, _ in ab], [b for _, b in ab], [n] * len(ab), L)
        Rinv = pow(R, -1, n)
        for i, (a, b) in enumerate(ab):
            mm.append({"name": "control", "L": L, "mod": "random", "a": a, "b": b, "n": n, "want": a * b * Rinv % n,
                       "model": got[i], "ev": ev.row(i), "event": None, "pred": None})
        # ---- geq, every pair in both orders
        base = rng.getrandbits(32 * L) | (1 << (32 * L - 1))
        limb = lambda v, i: (v >> (32 * i)) & 0xFFFFFFFF  # noqa: E731
        b0 = _set_limbs(base, 0, 1, 5)
        bt = _set_limbs(base, L - 1, 1, 0x80000005)
        lo, hi_ = 2 * (L // 6), 2 * (L // 3)  # two limbs in different lanes (even: lower limbs at K = 2)
        cross_a = _set_limbs(_set_limbs(base, lo, 1, 9), hi_, 1, 7)
        cross_b = _set_limbs(_set_limbs(base, lo, 1, 8), hi_, 1, 8)
        pairs = [("equal", base, base), ("zero_zero", 0, 0), ("limb_0", b0, _set_limbs(base, 0, 1, 6)),
                 ("top_limb", bt, _set_limbs(base, L - 1, 1, 0x80000006)),
                 ("low_lane_greater_high_lane_less", cross_a, cross_b)]
        if K == 2:
            two_a = _set_limbs(_set_limbs(base, hi_, 1, 9), hi_ + 1, 1, 7)
            two_b = _set_limbs(_set_limbs(base, hi_, 1, 8), hi_ + 1, 1, 8)
            pairs.append(("limbs_of_one_lane_disagree", two_a, two_b))
        for name, a, b in pairs:
            for x, y in ((a, b), (b, a)):
                gq.append({"name": name, "L": L, "a": x, "b": y, "want": x >= y})
        got = M.run_geq([c["a"] for c in gq if c["L"] == L], [c["b"] for c in gq if c["L"] == L], L)
        for c, g in zip([c for c in gq if c["L"] == L], got):
            c["model"] = g
        # ---- modexp: every exponent shape, random s and s in {0, 1, n - 1}
        for e in EXPONENTS:
            ss, ns, names = [], [], []
            for mod in MODEXP_MODULI:
                n = mods[mod]
                for sname, s in (("random", rng.randrange(2, n - 1)), ("0", 0), ("1", 1), ("n-1", n - 1)):
                    ss.append(s)
                    ns.append(n)
                    names.append((mod, sname))
            got, ev = M.run_modexp(ss, ns, L, e) if modexp_model else (None, None)
            for i, (mod, sname) in enumerate(names):
                me.append({"name": f"e={e:#x},s={sname}", "L": L, "mod": mod, "s": ss[i], "n": ns[i], "e": e,
                           "want": pow(ss[i], e, ns[i]), "model": got[i] if got else None,
                           "ev": ev.row(i) if ev else None})
    return {"mont_mul": mm, "double_mod": dm, "geq": gq, "modexp": me}
