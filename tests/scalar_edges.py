"""Target scalars at the edges of the fixed-base and per-key tables (test helper).

Every ladder recodes a scalar into signed radix-2^W digits and gathers one table entry per digit
(ed25519_rows.h sc_recode_wb, ecdsa_rows.h ec_recode_wide / ec_recode_w6). A random scalar reaches
the last entry of a row (|digit| = 2^(W-1), through the recoding carry) with probability 2^-W per
row, so the lists here are built digit by digit instead:

  per row u     v 2^(W u) for v in {1, 2, h - 1, h, h + 1, 2^W - 1} (h = 2^(W-1)), and the entries on
                both sides of a build-group boundary of that row (the groups a table-build lane
                writes: their sizes are read from the headers, see `group_sizes`);
  all rows      every window h - 1, h, 2^W - 1, and alternating h / 0 (cut to the bound's bits);
  top           bound - 1, bound - 2^(W u); for the radix-2^8 per-key rows the top digits 128, 129,
                255 and 256 (ecdsa_rows.h: the 33rd row);
  small         1, 2 (and 0 for Ed25519's S);
  control       seeded random scalars.

A scalar that reaches the bound is skipped. `note` names radix, row and pattern."""
import os
import random
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "corda_amd", "csrc")
L = 2 ** 252 + 27742317777372353535851937790883648493
N = {2: 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,   # secp256k1
     3: 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551}   # secp256r1
WIDE_RADIXES = (26, 24, 22)  # the fixed-base builds: the default and Makefile VARIANTS
ED_IDENTITY_KEY = bytes([1]) + bytes(31)  # y = 1, x = 0


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def header_int(name, header):
    m = re.search(r"^#define\s+%s\s+\(?(\d+)u?\)?\s*(?://.*)?$" % re.escape(name), _src(header), re.M)
    assert m, f"{name} not a plain #define in {header}"
    return int(m.group(1))


def group_sizes():
    """Entries one build lane writes, per table, from the headers:
    ed_b     ed_bwide_group (k_ed_bwide_init): its `pts[...]` run
    ec_g     EC_MULT, the group of EC_GTAB_LANES / EC_GWIDE_LANES (ec_gwide_group_from)
    ed_row   ED_WIDE_GROUP, the per-key wide rows' group
    ec_row   EC_WIDE_MULT / EC_WIDE_ROW_LANES, a lane's share of a per-key wide ECDSA row
    ec_g_batch  lanes per k_ec_gwide_init launch (EC_GWIDE_BATCH; depends on the radix: a callable)"""
    ed = _src("ed25519_rows.h")
    body = ed[ed.index("CG_HD void ed_bwide_group("):]
    body = body[:body.index("\n}\n")]
    m = re.search(r"ge_p3 pts\[(\d+)\];", body)
    assert m and f"ed_niels_batch{m.group(1)}<" in body
    keyws = _src("keyws.h")
    for lanes in ("EC_GTAB_LANES", "EC_GWIDE_LANES"):
        assert re.search(r"#define %s \(\w+ \* \(\w+ / EC_MULT\)\)" % lanes, keyws), lanes
    ec_mult = header_int("EC_MULT", "ecdsa_rows.h")
    scratch_max = header_int("CONST_SCRATCH_MAX", "keyws.h")
    g_digits, g_mult = header_int("EC_G_DIGITS", "ecdsa_rows.h"), header_int("EC_G_MULT", "ecdsa_rows.h")
    assert "#define EC_GWIDE_BATCH (CONST_SCRATCH_LANES - 1)" in _src("verify_ec.hip")

    def ec_g_batch(w):
        lanes = ((257 + w - 1) // w) * ((1 << (w - 1)) // ec_mult)  # EC_GWIDE_LANES
        return max(min(lanes, scratch_max), g_digits * (g_mult // ec_mult)) - 1

    return {"ed_b": int(m.group(1)), "ec_g": ec_mult, "ed_row": header_int("ED_WIDE_GROUP", "ed25519_rows.h"),
            "ec_row": header_int("EC_WIDE_MULT", "ecdsa_rows.h") // header_int("EC_WIDE_ROW_LANES", "ecdsa_rows.h"),
            "ec_g_batch": ec_g_batch}


def ed_digits(w):
    """Digits of sc_recode_wb<w> / sc_recode_w16<w> (a < 2^253)."""
    return (253 + w - 1) // w + (1 if 253 % w == 0 else 0)


def ec_g_digits(w):
    """EC_WIDE_GDIGITS at radix 2^w (a < 2^256 and the carry out of bit 255)."""
    return (257 + w - 1) // w


def recode(x, w, d, top_unsigned=False):
    """The signed digits the device recodings produce (the plain statement of their loop)."""
    out, carry = [], 0
    for t in range(d):
        e = ((x >> (w * t)) & ((1 << w) - 1)) + carry
        if not top_unsigned or t + 1 < d:
            carry = (e + (1 << (w - 1))) >> w
            e -= carry << w
        out.append(e)
    return out


def _pow2(v):
    return f"2^{v.bit_length() - 1}" if v & (v - 1) == 0 else None


def targets(w, d, bound, groups=(), row_edges=None, per_row=True, top_digits=(), zero=False, n_random=4, seed=0):
    """[(note, scalar)] for radix 2^w, d digits, scalars in [1, bound) (0 too with `zero`).
    groups: build-group sizes g (entries g | g + 1 straddle a boundary, in every row);
    row_edges(u): further entries e of row u whose successor e + 1 another lane or launch writes."""
    h, m = 1 << (w - 1), (1 << w) - 1
    out = []

    def add(note, x):
        if (0 if zero else 1) <= x < bound:
            out.append((f"w{w} {note}", x))

    if per_row:
        for u in range(d):
            vals = [("1", 1), ("2", 2), ("h-1", h - 1), ("h", h), ("h+1", h + 1), ("max", m)]
            for g in groups:
                if g + 1 <= h:
                    vals += [(f"g{g}", g), (f"g{g}+1", g + 1)]
            for e in (row_edges(u) if row_edges else ()):
                vals += [(f"e{e}", e), (f"e{e}+1", e + 1)]
            for name, v in vals:
                add(f"r{u} {name}", v << (w * u))
    bits = bound.bit_length()

    def fit(x):  # cut to the bound's bit length, then below the bound
        x &= (1 << bits) - 1
        return x if x < bound else x & ~(1 << (bits - 1))

    rows = range(d)
    add("all h-1", fit(sum((h - 1) << (w * u) for u in rows)))
    add("all h", fit(sum(h << (w * u) for u in rows)))
    add("all max", fit(sum(m << (w * u) for u in rows)))
    add("alt h/0", fit(sum(h << (w * u) for u in rows if u % 2 == 0)) % bound)
    add("alt 0/h", fit(sum(h << (w * u) for u in rows if u % 2 == 1)) % bound)
    add("bound-1", bound - 1)
    for u in range(d):
        add(f"bound-2^(w*{u})", bound - (1 << (w * u)))
    for name, x in top_digits:
        add(name, x)
    if zero:
        add("zero", 0)
    add("one", 1)
    add("two", 2)
    rng = random.Random(seed * 1000 + w)
    for k in range(n_random):
        add(f"random {k}", rng.randrange(1, bound))
    return out


def ed_s_targets(w, per_row=True, n_random=4):
    g = group_sizes()
    return targets(w, ed_digits(w), L, groups=(g["ed_b"],) if w in WIDE_RADIXES else (), per_row=per_row, zero=True,
                   n_random=n_random, seed=1)


def ec_u1_targets(scheme, w, per_row=True, n_random=4):
    g = group_sizes()
    if w not in WIDE_RADIXES:  # the radix-2^10 rows (EcGTab): 26 digits, groups of EC_MULT
        return targets(w, 26, N[scheme], groups=(g["ec_g"],), per_row=per_row, n_random=n_random, seed=scheme)
    per_row_groups, batch = (1 << (w - 1)) // g["ec_g"], g["ec_g_batch"](w)

    def launch_edges(u):  # the last entry a k_ec_gwide_init launch writes in row u, if one ends inside it
        first = -(-(u * per_row_groups + 1) // batch) * batch  # first launch start >= the row's lane 1
        if first < (u + 1) * per_row_groups:
            return [(first - u * per_row_groups) * g["ec_g"]]
        return []

    return targets(w, ec_g_digits(w), N[scheme], groups=(g["ec_g"],), row_edges=launch_edges, per_row=per_row,
                   n_random=n_random, seed=scheme)


def ec_u2_targets(scheme, w, n_random=4):
    """Per-key rows: radix 2^6 (43 signed digits, ec_recode_w6) or radix 2^8 (32 digits, the top one
    unsigned in [0, 256]: rows 31 and 32 of EcWideTab)."""
    g = group_sizes()
    n = N[scheme]
    if w == 6:
        return targets(6, header_int("EC_DIGITS", "ecdsa_rows.h"), n, n_random=n_random, seed=10 + scheme)
    assert w == 8
    top = [("top digit 128", (0x80 << 248) | 1), ("top digit 129", (0x81 << 248) | 1),
           ("top digit 128+g", ((0x80 + g["ec_row"]) << 248) | 1), ("top digit 128+g+1", ((0x81 + g["ec_row"]) << 248) | 1),
           ("top digit 255", (0xFF << 248) | 1), ("top digit 256", 0xFF80 << 240)]
    return targets(8, header_int("EC_WIDE_DIGITS", "ecdsa_rows.h"), n, groups=sorted({g["ed_row"], g["ec_row"]}),
                   top_digits=top, n_random=n_random, seed=10 + scheme)


def ed_s_above_l():
    """S the i2p engine accepts above L: [L, 2^253), [2^253, 2^255) and from 2^255 up (the expected
    verdict is the oracle's). L + t recodes as t: the row edges of every wide radix again."""
    out = [("S=L", L), ("S=L+5", L + 5), ("S=2^253-1", 2 ** 253 - 1), ("S=2^253+3", 2 ** 253 + 3),
           ("S=2^254+2^252-1", 2 ** 254 + 2 ** 252 - 1), ("S=2^255-1", 2 ** 255 - 1), ("S=2^255", 2 ** 255),
           ("S=2^255+9", 2 ** 255 + 9), ("S=2^256-L", 2 ** 256 - L), ("S=2^256-1", 2 ** 256 - 1), ("S=8L-1", 8 * L - 1),
           ("S=15L", 15 * L)]
    for w in WIDE_RADIXES:
        h = 1 << (w - 1)
        out += [(f"S=L+w{w} r0 h", L + h), (f"S=L+w{w} r3 h", L + (h << (3 * w))), (f"S=2L+w{w} r1 max", 2 * L + ((2 * h - 1) << w))]
    return [("above L: " + n, s) for n, s in out if s < 2 ** 256]
