"""ECDSA scalars that steer a ladder into the exceptional cases of its mixed additions (test helper).

Every ladder mode computes R = u2 Q + u1 G as all of the Q part, then the G part over the constant
wide table: one mixed addition per non-zero digit g_0 .. g_{D-1} of u1 at radix 2^w, rows 0 .. D-1
(ecdsa_rows.h ec_add_g_wide, ecdsa_ladder_check_wide). With the accumulator v G after the Q part,

    v = +g_m 2^(w m) - sum_{i<m} g_i 2^(w i)   row m adds the point the accumulator holds: a doubling
    v = -g_m 2^(w m) - sum_{i<m} g_i 2^(w i)   row m adds its negative: infinity, and the next
                                               non-zero row loads its entry

which honest signatures reach with probability ~2^-256. `specs` lists, per curve and fixed-base radix
(tests/scalar_edges.py WIDE_RADIXES), the (t1, v) pairs; tests/golden/gen_ec_exceptional.py solves a
key and a signature for each (u1 = t1, u2 Q = v G).

  dbl@m            m in {0, 1, D//2, D-2, D-1}
  neg@m            m in {0, 1, D//2, D-2}
  neg@1 gap        digit 2 of t1 is zero: the reload comes a row later, after a skipped operation
  neg@last         m = D-1: v = -t1, the ladder ends at infinity, INVALID
  dbl@1 neg@2      digits (-h, +1) at rows 1, 2 (raw fields h = 2^(w-1) and 0): the doubled
                   accumulator -2^(2w) G meets +2^(2w) G: doubling, infinity, reload
  control          seeded random (t1, v)

`EXPECT` gives, per kind, what jac_madd_w must count in the host build (doublings taken, infinities
produced, loads into an infinite accumulator: the Q part's first addition is one load)."""
import random

import scalar_edges as SE

N = SE.N
N_CONTROL = 2
# kind -> (doublings, infinities, loads)
EXPECT = {"dbl": (1, 0, 1), "neg": (0, 1, 2), "neg gap": (0, 1, 2), "neg last": (0, 1, 1), "dbl neg": (1, 1, 2),
          "control": (0, 0, 1), "filter": (0, 0, 1)}


def dbl_rows(d):
    return (0, 1, d // 2, d - 2, d - 1)


def neg_rows(d):
    return (0, 1, d // 2, d - 2)


def from_digits(g, w):
    return sum(x << (w * i) for i, x in enumerate(g))


def seeded_t1(rng, n, w, d, fixed=None):
    """t1 in (0, n) whose radix-2^w digits (scalar_edges.recode) are all non-zero and inside
    (-h, h), except the rows `fixed` names ({row: digit}); the top digit is positive."""
    h = 1 << (w - 1)
    top_max = 1 << (255 - w * (d - 1))  # t1 < 2^255 < n
    g = [rng.choice((-1, 1)) * rng.randrange(1, h) for _ in range(d - 1)] + [rng.randrange(1, top_max)]
    for row, val in (fixed or {}).items():
        g[row] = val
    t1 = from_digits(g, w)
    assert 0 < t1 < n and SE.recode(t1, w, d) == g
    return t1, g


def v_for(g, w, m, sign, n):
    """The accumulator after the Q part that makes row m add +-(its own entry)."""
    return (sign * g[m] * (1 << (w * m)) - from_digits(g[:m], w)) % n


def walk(t1, v, w, n):
    """(doublings, infinities, loads) of the G part at radix 2^w from the accumulator v G (v != 0: the
    Q part's one load), in exact integers mod n: what jac_madd_w must count. An item made for one
    radix can collide at another too (its low digits may spell the same partial sums there)."""
    dbl = infs = 0
    loads, acc, inf = 1, v % n, False
    for m, g in enumerate(SE.recode(t1, w, SE.ec_g_digits(w))):
        step = (g << (w * m)) % n
        if g == 0:
            continue
        if inf:
            loads, acc, inf = loads + 1, step, False
        elif acc == step:
            dbl, acc = dbl + 1, 2 * step % n
        elif (acc + step) % n == 0:
            infs, acc, inf = infs + 1, 0, True
        else:
            acc = (acc + step) % n
    return dbl, infs, loads


def specs():
    """[{kind, scheme, w, note, t1, v, rows}]: rows = the G rows whose addition is exceptional."""
    out = []
    for scheme in (3, 2):
        n = N[scheme]
        for w in SE.WIDE_RADIXES:
            d = SE.ec_g_digits(w)
            h = 1 << (w - 1)
            rng = random.Random(0xEC0000 + 100 * scheme + w)

            def add(kind, note, t1, v, rows):
                out.append({"kind": kind, "scheme": scheme, "w": w, "note": f"w{w} {note}", "t1": t1, "v": v,
                            "rows": rows})

            for m in dbl_rows(d):
                t1, g = seeded_t1(rng, n, w, d)
                add("dbl", f"dbl@{m}", t1, v_for(g, w, m, +1, n), [m])
            for m in neg_rows(d):
                t1, g = seeded_t1(rng, n, w, d)
                add("neg", f"neg@{m}", t1, v_for(g, w, m, -1, n), [m])
            t1, g = seeded_t1(rng, n, w, d, {2: 0})
            add("neg gap", "neg@1 gap", t1, v_for(g, w, 1, -1, n), [1])
            t1, g = seeded_t1(rng, n, w, d)
            v = v_for(g, w, d - 1, -1, n)
            assert (v + t1) % n == 0
            add("neg last", "neg@last", t1, v, [d - 1])
            t1, g = seeded_t1(rng, n, w, d, {0: rng.randrange(1, h), 1: -h, 2: 1})
            assert (t1 >> w) & (2 * h - 1) == h and (t1 >> (2 * w)) & (2 * h - 1) == 0  # the raw fields
            add("dbl neg", "dbl@1 neg@2", t1, v_for(g, w, 1, +1, n), [1, 2])
            for k in range(N_CONTROL):
                t1, g = seeded_t1(rng, n, w, d)
                add("control", f"control {k}", t1, rng.randrange(1, n), [])
    return out
