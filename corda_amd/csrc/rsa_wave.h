// Lane-cooperative big numbers for the RSA kernels (verify_rsa.hip) and the test-only harness
// (tests/native/rsa_wave_gpu.hip): a number of up to 128 limbs spread over one wavefront, limb
// K * lane + k in w[k] of each lane (K = 1 up to 64 limbs, 2 above). Every function below is called
// by all 64 lanes of the wave together, with wave-uniform L, n0inv and e.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cg {

// Deferred carries -> limbs. acc[k] < 2^35; the carry out of the top limb (limb 64 K) adds to `top`.
template <int K>
__device__ __forceinline__ void rsa_resolve(uint32_t r[K], const uint64_t acc[K], uint32_t lane, uint32_t& top) {
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint64_t v = acc[k] + c;
    r[k] = (uint32_t)v;
    c = v >> 32;
  }
  uint32_t cin = __shfl_up((uint32_t)c, 1, 64);
  if (lane == 0) cin = 0;
  top += __shfl((uint32_t)c, 63, 64);
  uint32_t g = cin;
  bool p = true;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint64_t v = (uint64_t)r[k] + g;
    r[k] = (uint32_t)v;
    g = (uint32_t)(v >> 32);
    p = p && r[k] == 0xffffffffu;
  }
  // what is left is a 0/1 ripple: lane l generates (g) or propagates (p: all ones), never both
  const uint64_t G = __ballot(g != 0), P = __ballot(p);
  const uint64_t C = ((G << 1) + P) ^ P;  // carry into lane l at bit l
  top += (uint32_t)((G >> 63) | ((P >> 63) & (C >> 63)));
  uint32_t ci = (uint32_t)(C >> lane) & 1u;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint64_t v = (uint64_t)r[k] + ci;
    r[k] = (uint32_t)v;
    ci = (uint32_t)(v >> 32);
  }
}

// a >= b over all limbs
template <int K>
__device__ __forceinline__ bool rsa_geq(const uint32_t a[K], const uint32_t b[K]) {
  bool gt = false, lt = false;
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    if (!gt && !lt) {
      gt = a[k] > b[k];
      lt = a[k] < b[k];
    }
  }
  return __ballot(gt) >= __ballot(lt);
}

// acc (a value below 2 n, carries deferred) -> r = acc mod n over L limbs
template <int K>
__device__ __forceinline__ void rsa_finish(uint32_t r[K], const uint64_t acc[K], const uint32_t n[K], uint32_t L,
                                           uint32_t lane) {
  uint32_t top = 0;
  rsa_resolve<K>(r, acc, lane, top);
  bool hi = false;  // a limb at or above L set: the value is >= 2^(32 L) > n
#pragma unroll
  for (int k = 0; k < K; ++k) hi = hi || (K * lane + k >= L && r[k] != 0);
  const bool over = top != 0 || __ballot(hi) != 0;
  if (over || rsa_geq<K>(r, n)) {
    uint64_t d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = (uint64_t)r[k] + (uint32_t)~n[k] + ((lane == 0 && k == 0) ? 1u : 0u);
    uint32_t t2 = 0;
    rsa_resolve<K>(r, d, lane, t2);
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (K * lane + k >= L) r[k] = 0;
}

// r = a b R^-1 mod n, R = 2^(32 L); a, b < n. r may alias a or b.
template <int K>
__device__ __forceinline__ void rsa_mont_mul(uint32_t r[K], const uint32_t a[K], const uint32_t b[K],
                                             const uint32_t n[K], uint32_t n0inv, uint32_t L, uint32_t lane) {
  uint64_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0;
  const uint32_t nl = (L + K - 1) / K;
  for (uint32_t li = 0; li < nl; ++li) {
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      if (K * li + kk >= L) break;
      const uint32_t ai = __builtin_amdgcn_readlane(a[kk], li);
      uint64_t p[K], q[K];
#pragma unroll
      for (int k = 0; k < K; ++k) p[k] = (uint64_t)ai * b[k] + (uint32_t)acc[k];
      const uint32_t m = __builtin_amdgcn_readfirstlane((uint32_t)p[0] * n0inv);
#pragma unroll
      for (int k = 0; k < K; ++k) q[k] = (uint64_t)m * n[k] + (uint32_t)p[k];
      // the next lane's lowest limb: a DPP wave shift (lane l reads lane l + 1, lane 63 reads 0), a
      // VALU move instead of a round trip through the LDS crossbar on the per-step critical path
      const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)q[0], 0x130, 0xf, 0xf, false);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const uint32_t next = k + 1 < K ? (uint32_t)q[k + 1 < K ? k + 1 : 0] : dn;
        acc[k] = (uint64_t)next + (p[k] >> 32) + (q[k] >> 32) + (acc[k] >> 32);
      }
    }
  }
  rsa_finish<K>(r, acc, n, L, lane);
}

// x = 2 x mod n (x < n)
template <int K>
__device__ __forceinline__ void rsa_double_mod_wave(uint32_t x[K], const uint32_t n[K], uint32_t L, uint32_t lane) {
  uint64_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 2ull * x[k];
  rsa_finish<K>(x, acc, n, L, lane);
}

// acc = s^e mod n for e > 1 (s < n; x holds R^2 mod n on entry and s R afterwards): left-to-right
// square-and-multiply over Montgomery products; the last product takes the value out of Montgomery
// form. One text for both users: k_rsa_verify expands it in place, everything else calls
// rsa_wave_modexp below. (As a call, even a force-inlined one, the same text gave the verify kernel
// another schedule of the product loops: 1.2% slower at 2048 bits, 2.5% at 4096; expanded in place
// the kernel's code is what it was when the ladder stood in verify_rsa.hip.)
#define RSA_WAVE_LADDER(K, acc, s, x, n, n0inv, L, e, lane)                                            \
  {                                                                                                    \
    rsa_mont_mul<K>(x, s, x, n, n0inv, L, lane); /* s R */                                             \
    _Pragma("unroll") for (int k = 0; k < K; ++k) acc[k] = x[k];                                       \
    const int top = 31 - __builtin_clz(e);                                                             \
    for (int bit = top - 1; bit >= 1; --bit) {                                                         \
      rsa_mont_mul<K>(acc, acc, acc, n, n0inv, L, lane);                                               \
      if ((e >> bit) & 1u) rsa_mont_mul<K>(acc, acc, x, n, n0inv, L, lane);                            \
    }                                                                                                  \
    rsa_mont_mul<K>(acc, acc, acc, n, n0inv, L, lane);                                                 \
    if (e & 1u) {                                                                                      \
      rsa_mont_mul<K>(acc, acc, s, n, n0inv, L, lane); /* times plain s: out of Montgomery form */     \
    } else {                                                                                           \
      uint32_t one[K];                                                                                 \
      _Pragma("unroll") for (int k = 0; k < K; ++k) one[k] = (lane == 0 && k == 0) ? 1u : 0u;          \
      rsa_mont_mul<K>(acc, acc, one, n, n0inv, L, lane);                                               \
    }                                                                                                  \
  }

template <int K>
__device__ __forceinline__ void rsa_wave_modexp(uint32_t acc[K], const uint32_t s[K], const uint32_t rr[K],
                                                const uint32_t n[K], uint32_t n0inv, uint32_t L, uint32_t e,
                                                uint32_t lane) {
  uint32_t x[K];
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = rr[k];
  RSA_WAVE_LADDER(K, acc, s, x, n, n0inv, L, e, lane)
}

}  // namespace cg
