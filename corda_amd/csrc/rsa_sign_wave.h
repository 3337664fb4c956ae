// Lane code of RSA-PSS signing (sign_rsa.hip and the test-only harness tests/native_rsa_sign): the
// private-key operation over CRT parts on one wavefront. The two half-size exponentiations
// EM^dP mod p and EM^dQ mod q run at once, one in each half of the wave: lanes 0-31 hold the limbs of
// the p side, lanes 32-63 those of the q side, limb K * (lane & 31) + k in w[k] (K = 1 up to 32 limbs
// per prime, 2 up to 64). Both sides use one limb count Lh = limbs(max(p, q)) and R = 2^(32 Lh), so a
// value below q is a legal operand on the p side (and the other way round) whichever prime is longer.
// The "rsa2_" functions are the paired forms of rsa_wave.h's; every function is called by all 64
// lanes together with wave-uniform Lh. Full-width steps (recombination, s^e) use rsa_wave.h as it is.
#pragma once
#include "rsa.h"
#include "rsa_wave.h"

#define RSA_HALF_LIMBS 64u  // limbs of a prime: at most 2048 bits
#define CG_RSA_SIG_SLOT 512
#define RSA_SIGN_TAB_WORDS 2048u  // per wave: 16 powers x 2 sides x 64 limbs (K = 2); 4 KB used at K = 1

// A loaded signer as k_rsa_signer_expand leaves it. Everything but n, e and the sizes is secret.
struct RsaSignerRec {
  uint32_t ok;  // 1: loaded, 0: refused (its requests are CG_NOT_RUN)
  uint32_t bits, L, Lh, K, k, em_bits, block_len, e;
  uint32_t n0inv_n, n0inv_p, n0inv_q;
  uint32_t n[RSA_MAX_LIMBS];     // little-endian limbs, zero above L
  uint32_t rr_n[RSA_MAX_LIMBS];  // R_n^2 mod n, R_n = 2^(32 L)
  uint32_t qr_n[RSA_MAX_LIMBS];  // q R_n mod n
  uint32_t p[RSA_HALF_LIMBS], q[RSA_HALF_LIMBS], dp[RSA_HALF_LIMBS], dq[RSA_HALF_LIMBS];
  uint32_t rr_p[RSA_HALF_LIMBS], rr_q[RSA_HALF_LIMBS];  // R^2 mod p, mod q, R = 2^(32 Lh)
  uint32_t r3_p[RSA_HALF_LIMBS], r3_q[RSA_HALF_LIMBS];  // R^3
  uint32_t qinv[RSA_HALF_LIMBS];                        // q^-1 mod p, plain
};

namespace cg {

__device__ __forceinline__ void rsa_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// rsa_resolve per half: no carry crosses from lane 31 into lane 32; `top` is the half's own.
template <int K>
__device__ __forceinline__ void rsa2_resolve(uint32_t r[K], const uint64_t acc[K], uint32_t lane, uint32_t& top) {
  const uint32_t hl = lane & 31u;
  const bool up = lane >= 32u;
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint64_t v = acc[k] + c;
    r[k] = (uint32_t)v;
    c = v >> 32;
  }
  uint32_t cin = __shfl_up((uint32_t)c, 1, 64);
  if (hl == 0) cin = 0;
  top += __shfl((uint32_t)c, (int)(lane | 31u), 64);
  uint32_t g = cin;
  bool p = true;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint64_t v = (uint64_t)r[k] + g;
    r[k] = (uint32_t)v;
    g = (uint32_t)(v >> 32);
    p = p && r[k] == 0xffffffffu;
  }
  const uint64_t G = __ballot(g != 0), P = __ballot(p);
  const uint64_t Gh = up ? G >> 32 : G & 0xffffffffull, Ph = up ? P >> 32 : P & 0xffffffffull;
  const uint64_t C = ((Gh << 1) + Ph) ^ Ph;  // carry into lane l of the half at bit l, out of it at bit 32
  top += (uint32_t)(C >> 32) & 1u;
  uint32_t ci = (uint32_t)(C >> hl) & 1u;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint64_t v = (uint64_t)r[k] + ci;
    r[k] = (uint32_t)v;
    ci = (uint32_t)(v >> 32);
  }
}

// a >= b, each half for itself
template <int K>
__device__ __forceinline__ bool rsa2_geq(const uint32_t a[K], const uint32_t b[K], uint32_t lane) {
  bool gt = false, lt = false;
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    if (!gt && !lt) {
      gt = a[k] > b[k];
      lt = a[k] < b[k];
    }
  }
  const uint64_t g = __ballot(gt), l = __ballot(lt);
  const bool up = lane >= 32u;
  return (up ? (uint32_t)(g >> 32) : (uint32_t)g) >= (up ? (uint32_t)(l >> 32) : (uint32_t)l);
}

// acc (below 2 m in each half, carries deferred) -> r = acc mod m over Lh limbs. The subtraction is
// computed by the whole wave when either half needs it and kept by the halves that do.
template <int K>
__device__ __forceinline__ void rsa2_finish(uint32_t r[K], const uint64_t acc[K], const uint32_t m[K], uint32_t Lh,
                                            uint32_t lane) {
  const uint32_t hl = lane & 31u;
  uint32_t top = 0;
  rsa2_resolve<K>(r, acc, lane, top);
  bool hi = false;
#pragma unroll
  for (int k = 0; k < K; ++k) hi = hi || (K * hl + k >= Lh && r[k] != 0);
  const uint64_t hb = __ballot(hi);
  const uint32_t hh = lane >= 32u ? (uint32_t)(hb >> 32) : (uint32_t)hb;
  const bool need = top != 0 || hh != 0 || rsa2_geq<K>(r, m, lane);
  if (__ballot(need) != 0) {
    uint64_t d[K];
    uint32_t s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = (uint64_t)r[k] + (uint32_t)~m[k] + ((hl == 0 && k == 0) ? 1u : 0u);
    uint32_t t2 = 0;
    rsa2_resolve<K>(s, d, lane, t2);
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = need ? s[k] : r[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (K * hl + k >= Lh) r[k] = 0;
}

// r = a b R^-1 mod m in each half, R = 2^(32 Lh). One of a, b below m, the other below R. m and
// n0inv are the half's own. r may alias a or b.
template <int K>
__device__ __forceinline__ void rsa2_mont_mul(uint32_t r[K], const uint32_t a[K], const uint32_t b[K],
                                              const uint32_t m[K], uint32_t n0inv, uint32_t Lh, uint32_t lane) {
  const bool up = lane >= 32u;
  const bool last = (lane & 31u) == 31u;
  uint64_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0;
  const uint32_t nl = (Lh + K - 1) / K;
  for (uint32_t li = 0; li < nl; ++li) {
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      if (K * li + kk >= Lh) break;
      const uint32_t a_lo = __builtin_amdgcn_readlane(a[kk], li);
      const uint32_t a_hi = __builtin_amdgcn_readlane(a[kk], 32u + li);
      const uint32_t ai = up ? a_hi : a_lo;
      uint64_t p[K], q[K];
#pragma unroll
      for (int k = 0; k < K; ++k) p[k] = (uint64_t)ai * b[k] + (uint32_t)acc[k];
      const uint32_t t = (uint32_t)p[0] * n0inv;
      const uint32_t t_lo = __builtin_amdgcn_readlane(t, 0);
      const uint32_t t_hi = __builtin_amdgcn_readlane(t, 32);
      const uint32_t mq = up ? t_hi : t_lo;
#pragma unroll
      for (int k = 0; k < K; ++k) q[k] = (uint64_t)mq * m[k] + (uint32_t)p[k];
      // lane l reads lane l + 1; the top lane of the lower half must not take the upper half's limb 0
      uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)q[0], 0x130, 0xf, 0xf, false);
      dn = last ? 0u : dn;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const uint32_t next = k + 1 < K ? (uint32_t)q[k + 1 < K ? k + 1 : 0] : dn;
        acc[k] = (uint64_t)next + (p[k] >> 32) + (q[k] >> 32) + (acc[k] >> 32);
      }
    }
  }
  rsa2_finish<K>(r, acc, m, Lh, lane);
}

// r = a + b mod m (a, b < m)
template <int K>
__device__ __forceinline__ void rsa2_add_mod(uint32_t r[K], const uint32_t a[K], const uint32_t b[K],
                                             const uint32_t m[K], uint32_t Lh, uint32_t lane) {
  uint64_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = (uint64_t)a[k] + b[k];
  rsa2_finish<K>(r, acc, m, Lh, lane);
}

// r = a - b mod m (a, b < m): a + (m - b), m - b in (0, m]
template <int K>
__device__ __forceinline__ void rsa2_sub_mod(uint32_t r[K], const uint32_t a[K], const uint32_t b[K],
                                             const uint32_t m[K], uint32_t Lh, uint32_t lane) {
  uint64_t acc[K];
  uint32_t nb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = (uint64_t)m[k] + (uint32_t)~b[k] + (((lane & 31u) == 0 && k == 0) ? 1u : 0u);
  uint32_t t = 0;
  rsa2_resolve<K>(nb, acc, lane, t);  // the carry out of the half (2^(32 * 32 K)) is dropped
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = (uint64_t)a[k] + nb[k];
  rsa2_finish<K>(r, acc, m, Lh, lane);
}

// Digit w (4 bits, w = 0 the lowest) of each half's exponent e.
template <int K>
__device__ __forceinline__ uint32_t rsa2_digit(const uint32_t e[K], uint32_t w, uint32_t lane) {
  const uint32_t limb = w >> 3;
  const uint32_t ev = (K == 2 && (limb & 1u)) ? e[K - 1] : e[0];
  const uint32_t li = limb / K;
  const uint32_t lo = __builtin_amdgcn_readlane(ev, li);
  const uint32_t hi = __builtin_amdgcn_readlane(ev, 32u + li);
  return ((lane >= 32u ? hi : lo) >> (4u * (w & 7u))) & 15u;
}

// acc = x^e in each half, Montgomery form in and out: xm = x R mod m, one = R mod m; e padded to
// 32 Lh bits. Fixed 4-bit windows, every window followed by a product (digit 0: by `one`), so the
// instruction sequence does not depend on e; the table address does. tab: the wave's
// RSA_SIGN_TAB_WORDS of LDS, power d of lane l at tab[(64 d + l) K + k]: a lane reads what it wrote.
template <int K>
__device__ __forceinline__ void rsa2_modexp_win(uint32_t acc[K], const uint32_t xm[K], const uint32_t one[K],
                                                const uint32_t e[K], const uint32_t m[K], uint32_t n0inv,
                                                uint32_t Lh, uint32_t lane, uint32_t* tab) {
  uint32_t t[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    tab[lane * K + k] = one[k];
    tab[(64u + lane) * K + k] = xm[k];
    t[k] = xm[k];
  }
  for (uint32_t d = 2; d < 16; ++d) {
    rsa2_mont_mul<K>(t, t, xm, m, n0inv, Lh, lane);
#pragma unroll
    for (int k = 0; k < K; ++k) tab[(64u * d + lane) * K + k] = t[k];
  }
  rsa_wave_sync();
  const uint32_t nw = 8u * Lh;
  {
    const uint32_t d = rsa2_digit<K>(e, nw - 1, lane);
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = tab[(64u * d + lane) * K + k];
  }
  for (int w = (int)nw - 2; w >= 0; --w) {
#pragma unroll 1
    for (int s = 0; s < 4; ++s) rsa2_mont_mul<K>(acc, acc, acc, m, n0inv, Lh, lane);
    const uint32_t d = rsa2_digit<K>(e, (uint32_t)w, lane);
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = tab[(64u * d + lane) * K + k];
    rsa2_mont_mul<K>(acc, acc, t, m, n0inv, Lh, lane);
  }
}

// One side's constants in the paired layout: the p side in lanes 0-31, the q side in lanes 32-63.
template <int K>
__device__ __forceinline__ void rsa2_load(uint32_t w[K], const uint32_t* lo, const uint32_t* hi, uint32_t lane) {
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = (lane >= 32u ? hi : lo)[K * (lane & 31u) + k];
}

// m1 = x^dP mod p (lanes 0-31) and m2 = x^dQ mod q (lanes 32-63), plain, for x < n in the full-width
// layout (limb K lane + k). `m1m` is m1 in Montgomery form. Uses tab[0, 128) for the layout change.
template <int K>
__device__ __forceinline__ void rsa_crt_halves(uint32_t m12[K], uint32_t m1m[K], const uint32_t x[K],
                                               const RsaSignerRec* rec, const uint32_t mod[K], uint32_t n0inv,
                                               uint32_t L, uint32_t Lh, uint32_t lane, uint32_t* tab) {
  const uint32_t hl = lane & 31u;
  uint32_t lo[K], hi[K], rr[K], r3[K], ex[K], one[K], xm[K], t[K];
#pragma unroll
  for (int k = 0; k < K; ++k) tab[K * lane + k] = x[k];
  rsa_wave_sync();
#pragma unroll
  for (int k = 0; k < K; ++k) {  // x = lo + hi R, both below R (L <= 2 Lh)
    const uint32_t j = K * hl + k;
    lo[k] = j < Lh ? tab[j] : 0u;
    hi[k] = (j < Lh && Lh + j < L) ? tab[Lh + j] : 0u;
    one[k] = j == 0 ? 1u : 0u;
  }
  rsa_wave_sync();
  rsa2_load<K>(rr, rec->rr_p, rec->rr_q, lane);
  rsa2_load<K>(r3, rec->r3_p, rec->r3_q, lane);
  rsa2_load<K>(ex, rec->dp, rec->dq, lane);
  rsa2_mont_mul<K>(xm, lo, rr, mod, n0inv, Lh, lane);  // lo R
  rsa2_mont_mul<K>(t, hi, r3, mod, n0inv, Lh, lane);   // hi R R
  rsa2_add_mod<K>(xm, xm, t, mod, Lh, lane);           // (x mod m) R
  rsa2_mont_mul<K>(t, rr, one, mod, n0inv, Lh, lane);  // R mod m
  rsa2_modexp_win<K>(m1m, xm, t, ex, mod, n0inv, Lh, lane, tab);
  rsa2_mont_mul<K>(m12, m1m, one, mod, n0inv, Lh, lane);
}

// h = qInv (m1 - m2) mod p in lanes 0-31 (the q side computes along and is not used). m2 may be >= p.
template <int K>
__device__ __forceinline__ void rsa_crt_h(uint32_t h[K], const uint32_t m12[K], const uint32_t m1m[K],
                                          const RsaSignerRec* rec, const uint32_t mod[K], uint32_t n0inv, uint32_t Lh,
                                          uint32_t lane) {
  uint32_t m2[K], rr[K], qi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    m2[k] = __shfl(m12[k], (int)(lane | 32u), 64);
    qi[k] = lane < 32u ? rec->qinv[K * lane + k] : 0u;
  }
  rsa2_load<K>(rr, rec->rr_p, rec->rr_q, lane);
  rsa2_mont_mul<K>(m2, m2, rr, mod, n0inv, Lh, lane);  // m2 R mod p: m2 < q < R
  rsa2_sub_mod<K>(m2, m1m, m2, mod, Lh, lane);         // (m1 - m2) R
  rsa2_mont_mul<K>(h, m2, qi, mod, n0inv, Lh, lane);   // plain
}

// s = m2 + h q (< n) in the full-width layout, from the paired h (lanes 0-31) and m2 (lanes 32-63).
// Uses tab[0, 256).
template <int K>
__device__ __forceinline__ void rsa_crt_join(uint32_t s[K], const uint32_t h[K], const uint32_t m12[K],
                                             const RsaSignerRec* rec, const uint32_t n[K], uint32_t n0inv_n,
                                             uint32_t L, uint32_t lane, uint32_t* tab) {
  uint32_t hf[K], m2f[K], qr[K];
#pragma unroll
  for (int k = 0; k < K; ++k) tab[(lane >= 32u ? 128u : 0u) + K * (lane & 31u) + k] = lane >= 32u ? m12[k] : h[k];
  rsa_wave_sync();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t j = K * lane + k;
    hf[k] = j < 32u * K ? tab[j] : 0u;
    m2f[k] = j < 32u * K ? tab[128u + j] : 0u;
    qr[k] = rec->qr_n[j];
  }
  rsa_wave_sync();
  rsa_mont_mul<K>(s, hf, qr, n, n0inv_n, L, lane);  // h q mod n
  uint64_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = (uint64_t)s[k] + m2f[k];
  rsa_finish<K>(s, acc, n, L, lane);
}

// The private-key operation with its consistency check: s = x^d mod n through the CRT parts for
// x < n (full-width layout), then s^e mod n recomputed and compared with x. Returns whether it came
// back (wave-uniform); s is zero when it did not. A CRT result that is wrong modulo one prime gives
// away the factorisation, so such an s must never leave the device. The table region is zeroed.
template <int K>
__device__ __forceinline__ bool rsa_crt_sign_wave(uint32_t s[K], const uint32_t x[K], const RsaSignerRec* rec,
                                                  uint32_t lane, uint32_t* tab) {
  const uint32_t L = __builtin_amdgcn_readfirstlane(rec->L);
  const uint32_t Lh = __builtin_amdgcn_readfirstlane(rec->Lh);
  const uint32_t e = __builtin_amdgcn_readfirstlane(rec->e);
  const uint32_t n0inv_n = __builtin_amdgcn_readfirstlane(rec->n0inv_n);
  const uint32_t n0inv = lane >= 32u ? rec->n0inv_q : rec->n0inv_p;
  uint32_t mod[K], m12[K], m1m[K], h[K], n[K], c[K];
  rsa2_load<K>(mod, rec->p, rec->q, lane);
  rsa_crt_halves<K>(m12, m1m, x, rec, mod, n0inv, L, Lh, lane, tab);
  rsa_crt_h<K>(h, m12, m1m, rec, mod, n0inv, Lh, lane);
  rsa_wave_sync();
  for (uint32_t i = lane; i < RSA_SIGN_TAB_WORDS; i += 64u) tab[i] = 0u;  // the powers of x
  rsa_wave_sync();
#pragma unroll
  for (int k = 0; k < K; ++k) n[k] = rec->n[K * lane + k];
  rsa_crt_join<K>(s, h, m12, rec, n, n0inv_n, L, lane, tab);
  for (uint32_t i = lane; i < 256u; i += 64u) tab[i] = 0u;
  rsa_wave_sync();
  if (e > 1) {
    uint32_t rr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) rr[k] = rec->rr_n[K * lane + k];
    RSA_WAVE_LADDER(K, c, s, rr, n, n0inv_n, L, e, lane)
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) c[k] = s[k];
  }
  bool diff = false;
#pragma unroll
  for (int k = 0; k < K; ++k) diff = diff || c[k] != x[k];
  const bool ok = __ballot(diff) == 0;
  if (!ok) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0;
  }
  return ok;
}

// R^2 mod m over L limbs, R = 2^(32 L), for an odd m of `bits` bits in the full-width layout:
// k_rsa_keyprep's chain (R mod m by doublings from 2^(bits - 1), then square-and-double over the bits
// of 32 L).
template <int K>
__device__ __forceinline__ void rsa_rr_wave(uint32_t x[K], const uint32_t m[K], uint32_t n0inv, uint32_t L,
                                            uint32_t bits, uint32_t lane) {
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = (K * lane + k == (bits - 1) >> 5) ? 1u << ((bits - 1) & 31u) : 0u;
  for (uint32_t s = 32 * L - (bits - 1); s > 0; --s) rsa_double_mod_wave<K>(x, m, L, lane);
  rsa_double_mod_wave<K>(x, m, L, lane);
  const uint32_t E = 32 * L;
  for (int bit = 30 - __builtin_clz(E); bit >= 0; --bit) {
    rsa_mont_mul<K>(x, x, x, m, n0inv, L, lane);
    if ((E >> bit) & 1u) rsa_double_mod_wave<K>(x, m, L, lane);
  }
}

}  // namespace cg
