"""A bit-exact model of corda_amd/csrc/rsa_wave.h (and of the wave form of the key preparation in
verify_rsa.hip), lane by lane: the per-lane 64-bit accumulators, the three passes of rsa_resolve, the
two ballots as 64-bit integers, and the `over` / `hi` / `geq` decisions. It says which path a case
takes; it is never the reference for a value (that is Python's integers).

The model runs a batch of N cases at once: a number is a list of K numpy arrays of shape (N, 64),
dtype uint64, array k holding limb K * lane + k of every case. L, K and e are the same for the whole
batch; n and n0inv are per case. Every function takes an `Events` record and adds to it what the
call reached, counted **only in lanes that hold a limb below L** (lane l with K l < L):

  gen         lanes that generate a carry in the second pass (bit of G) for a lane that also holds a
              limb below L, or for `top`: a carry into a lane at or above L lands in limbs that
              rsa_finish overwrites with zero (the top lane of a 1025-bit key does that in every
              subtraction), so it witnesses nothing
  cprop       lanes that propagate (bit of P) and receive a carry (bit of C)
  iprop       lanes that propagate and receive none
  chain       the longest run of adjacent cprop lanes
  ripple_top  the ripple carries out of lane 63 into `top` (any lane: lane 63 is below L only at L > 63 K)
  top1        `top` != 0 from the first pass (the carry lane 63 held back)
  hi          a limb at or above L set after the resolve
  sub         the subtraction of n taken
  sub_eq      taken on equality alone (t == n)
  max_acc     the largest accumulator any lane held
"""
import numpy as np

U = np.uint64
M32 = U(0xFFFFFFFF)
S32 = U(32)
ONE = U(1)
LANES = np.arange(64, dtype=np.uint64)[None, :]


def k_of(L):
    """The kernels' choice: one limb per lane up to 64 limbs, two above."""
    return 1 if L <= 64 else 2


class Events:
    COUNTS = ("gen", "cprop", "iprop", "ripple_top", "top1", "hi", "sub", "sub_eq")
    MAXES = ("chain", "max_acc")

    def __init__(self, n):
        for f in self.COUNTS + self.MAXES:
            setattr(self, f, np.zeros(n, dtype=np.uint64))

    def row(self, i):
        return {f: int(getattr(self, f)[i]) for f in self.COUNTS + self.MAXES}

    def total(self):
        out = {f: int(getattr(self, f).sum()) for f in self.COUNTS}
        out.update({f: int(getattr(self, f).max()) if len(getattr(self, f)) else 0 for f in self.MAXES})
        return out


def to_lanes(vals, K):
    """Python integers (below 2^(2048 K)) -> K arrays (N, 64)."""
    out = [np.zeros((len(vals), 64), dtype=np.uint64) for _ in range(K)]
    for i, v in enumerate(vals):
        raw = np.frombuffer(int(v).to_bytes(256 * K, "little"), dtype="<u4").astype(np.uint64)
        for k in range(K):
            out[k][i] = raw[k::K]
    return out


def from_lanes(w):
    K = len(w)
    out = []
    for i in range(w[0].shape[0]):
        raw = np.zeros(64 * K, dtype="<u4")
        for k in range(K):
            raw[k::K] = w[k][i].astype("<u4")
        out.append(int.from_bytes(raw.tobytes(), "little"))
    return out


def n0inv_of(n):
    """-n^-1 mod 2^32 (rsa.h rsa_n0inv)."""
    return (-pow(n, -1, 1 << 32)) % (1 << 32)


def ballot(mask):
    return (mask.astype(np.uint64) << LANES).sum(axis=1, dtype=np.uint64)


def _longest_run(bits):
    run = np.zeros(bits.shape[0], dtype=np.uint64)
    best = run.copy()
    for lane in range(64):
        run = (run + ONE) * bits[:, lane].astype(np.uint64)
        best = np.maximum(best, run)
    return best


def resolve(acc, L, ev, act):
    """rsa_resolve: (r, top). `act`: the cases whose events count (the others' results are discarded)."""
    K = len(acc)
    live = (U(K) * LANES < U(L))
    into = (U(K) * (LANES + ONE) < U(L)) | (LANES == U(63))  # the lane (or `top`) its carry goes to
    a64 = act.astype(np.uint64)
    for k in range(K):
        ev.max_acc = np.maximum(ev.max_acc, acc[k].max(axis=1) * a64)
    c = np.zeros_like(acc[0])
    r = []
    for k in range(K):
        v = acc[k] + c
        r.append(v & M32)
        c = v >> S32
    cin = np.zeros_like(c)
    cin[:, 1:] = c[:, :-1]  # __shfl_up by one; lane 0 takes 0
    top = c[:, 63] & M32
    top1 = top != 0
    g = cin
    p = np.ones(c.shape, dtype=bool)
    for k in range(K):
        v = r[k] + g
        r[k] = v & M32
        g = v >> S32
        p &= r[k] == M32
    gm = g != 0
    G, P = ballot(gm), ballot(p)
    C = ((G << ONE) + P) ^ P  # 64-bit, wraps as on the device
    rt = (G >> U(63)) | ((P >> U(63)) & (C >> U(63)))
    top = (top + rt) & M32
    cm = ((C[:, None] >> LANES) & ONE)
    ci = cm.copy()
    for k in range(K):
        v = r[k] + ci
        r[k] = v & M32
        ci = v >> S32
    cb = cm.astype(bool)
    ev.gen += (gm & live & into).sum(axis=1).astype(np.uint64) * a64
    ev.cprop += (p & cb & live).sum(axis=1).astype(np.uint64) * a64
    ev.iprop += (p & ~cb & live).sum(axis=1).astype(np.uint64) * a64
    ev.chain = np.maximum(ev.chain, _longest_run(p & cb & live) * a64)
    ev.ripple_top += rt * a64
    ev.top1 += top1.astype(np.uint64) * a64
    return r, top


def geq(a, b):
    """rsa_geq: a >= b, one bool per case."""
    K = len(a)
    gt = np.zeros(a[0].shape, dtype=bool)
    lt = np.zeros(a[0].shape, dtype=bool)
    for k in range(K - 1, -1, -1):
        und = ~gt & ~lt
        gt = np.where(und, a[k] > b[k], gt)
        lt = np.where(und, a[k] < b[k], lt)
    return ballot(gt) >= ballot(lt)


def finish(acc, n, L, ev):
    """rsa_finish: acc (below 2 n, carries deferred) -> acc mod n over L limbs."""
    K = len(acc)
    N = acc[0].shape[0]
    every = np.ones(N, dtype=bool)
    r, top = resolve(acc, L, ev, every)
    hi_lane = np.zeros(acc[0].shape, dtype=bool)
    for k in range(K):
        hi_lane |= (U(K) * LANES + U(k) >= U(L)) & (r[k] != 0)
    hi = ballot(hi_lane) != 0
    over = (top != 0) | hi
    ge = geq(r, n)
    take = over | ge
    equal = np.ones(N, dtype=bool)
    for k in range(K):
        equal &= (r[k] == n[k]).all(axis=1)
    d = []
    for k in range(K):
        dk = r[k] + (~n[k] & M32)
        if k == 0:
            dk = dk.copy()
            dk[:, 0] += ONE
        d.append(dk)
    r2, _ = resolve(d, L, ev, take)
    out = []
    for k in range(K):
        v = np.where(take[:, None], r2[k], r[k])
        out.append(np.where(U(K) * LANES + U(k) >= U(L), U(0), v))
    ev.hi += hi.astype(np.uint64)
    ev.sub += take.astype(np.uint64)
    ev.sub_eq += (take & ~over & equal).astype(np.uint64)
    return out


def mont_mul(a, b, n, n0inv, L, ev):
    """rsa_mont_mul: a b R^-1 mod n, R = 2^(32 L). n0inv: (N,) uint64."""
    K = len(a)
    acc = [np.zeros_like(a[0]) for _ in range(K)]
    nl = (L + K - 1) // K
    n0 = n0inv.astype(np.uint64)
    for li in range(nl):
        for kk in range(K):
            if K * li + kk >= L:
                break
            ai = a[kk][:, li:li + 1]  # v_readlane: uniform over the wave
            p = [ai * b[k] + (acc[k] & M32) for k in range(K)]
            m = ((p[0][:, 0] & M32) * n0 & M32)[:, None]  # lane 0's product, v_readfirstlane
            q = [m * n[k] + (p[k] & M32) for k in range(K)]
            dn = np.zeros_like(q[0])
            dn[:, :-1] = q[0][:, 1:] & M32  # the DPP wave shift: lane l reads lane l + 1, lane 63 reads 0
            for k in range(K):
                nxt = (q[k + 1] & M32) if k + 1 < K else dn
                acc[k] = nxt + (p[k] >> S32) + (q[k] >> S32) + (acc[k] >> S32)
                ev.max_acc = np.maximum(ev.max_acc, acc[k].max(axis=1))
    return finish(acc, n, L, ev)


def double_mod(x, n, L, ev):
    """rsa_double_mod_wave: 2 x mod n."""
    return finish([U(2) * xk for xk in x], n, L, ev)


def modexp(s, rr, n, n0inv, L, e, ev):
    """The exponent branches of rsa_wave_verify: s for e = 1, rsa_wave_modexp above."""
    K = len(s)
    if e <= 1:
        return [sk.copy() for sk in s]
    x = mont_mul(s, rr, n, n0inv, L, ev)
    acc = [xk.copy() for xk in x]
    top = e.bit_length() - 1
    for bit in range(top - 1, 0, -1):
        acc = mont_mul(acc, acc, n, n0inv, L, ev)
        if (e >> bit) & 1:
            acc = mont_mul(acc, x, n, n0inv, L, ev)
    acc = mont_mul(acc, acc, n, n0inv, L, ev)
    if e & 1:
        return mont_mul(acc, s, n, n0inv, L, ev)
    one = [np.zeros_like(s[0]) for _ in range(K)]
    one[0][:, 0] = ONE
    return mont_mul(acc, one, n, n0inv, L, ev)


def keyprep(n_int):
    """The wave form of the key preparation (verify_rsa.hip rsa_keyprep_wave) for one modulus:
    (R^2 mod n as an integer, Events of one case)."""
    bits = n_int.bit_length()
    L = (bits + 31) // 32
    K = k_of(L)
    ev = Events(1)
    n = to_lanes([n_int], K)
    n0 = np.array([n0inv_of(n_int)], dtype=np.uint64)
    x = to_lanes([1 << (bits - 1)], K)
    for _ in range(32 * L - (bits - 1)):
        x = double_mod(x, n, L, ev)  # R mod n
    x = double_mod(x, n, L, ev)      # 2 R: "2"
    E = 32 * L
    for bit in range(E.bit_length() - 2, -1, -1):
        x = mont_mul(x, x, n, n0, L, ev)
        if (E >> bit) & 1:
            x = double_mod(x, n, L, ev)
    return from_lanes(x)[0], ev


# ---- convenience over Python integers (one batch: the same L for every case)
def run_mont_mul(a, b, n, L):
    K = k_of(L)
    ev = Events(len(a))
    n0 = np.array([n0inv_of(v) for v in n], dtype=np.uint64)
    r = mont_mul(to_lanes(a, K), to_lanes(b, K), to_lanes(n, K), n0, L, ev)
    return from_lanes(r), ev


def run_double_mod(x, n, L):
    K = k_of(L)
    ev = Events(len(x))
    return from_lanes(double_mod(to_lanes(x, K), to_lanes(n, K), L, ev)), ev


def run_geq(a, b, L):
    K = k_of(L)
    return [bool(v) for v in geq(to_lanes(a, K), to_lanes(b, K))]


def run_modexp(s, n, L, e):
    K = k_of(L)
    ev = Events(len(s))
    n0 = np.array([n0inv_of(v) for v in n], dtype=np.uint64)
    rr = [pow(2, 64 * L, v) for v in n]
    r = modexp(to_lanes(s, K), to_lanes(rr, K), to_lanes(n, K), n0, L, e, ev)
    return from_lanes(r), ev
