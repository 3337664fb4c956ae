// The LDS staging of a wide-table entry one op ahead of its addition, shared by the Ed25519 ladders
// (verify_ed.hip), the signer (sign_ed.hip) and key derivation (derive_keys.hip), and the two lane
// functions the latter two share: the fixed-base walk ed_fixed_base_pf and the batched encode
// ed_encode_run. The staging: the entry is gathered straight into
// LDS (global_load_lds, no VGPR destination) while the previous op's addition runs. LDS image per wave:
// 16-B chunk c of lane l at wave_base + 64 * 16 * c + 16 * l (the DMA's lane-linear destination).
#pragma once
#include <hip/hip_runtime.h>

#include "ed25519_rows.h"

namespace cg {

typedef __attribute__((address_space(3))) void* cg_lds_ptr;
typedef __attribute__((address_space(1))) void* cg_gbl_ptr;

// wave_lds_off: the wave's LDS image as a wave-uniform LDS byte offset (readfirstlane'd once
// by the caller), so the per-chunk M0 values are scalar adds, not VALU readfirstlanes
__device__ __forceinline__ cg_lds_ptr ed_lds_at(uint32_t wave_lds_off, uint32_t b) {
  return (cg_lds_ptr)(uintptr_t)(wave_lds_off + b);
}

// the radix-2^29 wide-table entries (fe9.h, 112 B): 7 x 16-B chunks, the same lane-linear image
__device__ __forceinline__ void ed_glds_niels9(const ge9_niels* src, uint32_t wave_lds_off) {
  const uint8_t* s = (const uint8_t*)src;
#pragma unroll
  for (int c = 0; c < 7; ++c)
    __builtin_amdgcn_global_load_lds((cg_gbl_ptr)(s + 16 * c), ed_lds_at(wave_lds_off, 64 * 16 * c), 16, 0, 0);
}
__device__ __forceinline__ void ed_lds_niels9(ge9_niels& n, const uint8_t* wave_lds, uint32_t lane) {
  uint32_t* d = (uint32_t*)&n;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    const uint4 v = *(const uint4*)(wave_lds + 64 * 16 * c + 16 * lane);
    d[4 * c] = v.x;
    d[4 * c + 1] = v.y;
    d[4 * c + 2] = v.z;
    if (c < 6) d[4 * c + 3] = v.w;  // the pad dword stays unread
  }
}

constexpr uint32_t kNiels9WaveBytes = 64 * 7 * 16;  // one wave's image of radix-2^29 entries

__device__ __forceinline__ const ge9_niels* ed_b_src(const EdBWideTab& TB, int row, int d) {
  const int a = d < 0 ? -d : d;
  return a > 0 ? &TB.t[row][a - 1] : &TB.ident;  // a zero digit adds the identity entry
}

// ed_fixed_base9 with each row's entry gathered into LDS one op ahead (the idiom of
// ed_double_scalar_pf's B tail): op u's addition runs while op u + 1's entry is in flight and op
// u + 2's digit word is loaded. The signer's r B (sign_ed.hip) and a derived key's a B (derive_keys.hip).
__device__ __forceinline__ void ed_fixed_base_pf(ge_p2& out, const uint32_t* __restrict__ dw, const EdBWideTab& TB,
                                                 uint8_t* wave_lds, uint32_t lane) {
  constexpr int N = EdWideCfg::kBDigits;
  const uint32_t wl = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(cg_lds_ptr)wave_lds);
  int d_cur = (int)dw[0];
  ed_glds_niels9(ed_b_src(TB, 0, d_cur), wl);
  uint32_t w_next = dw[1];
  ge9_p3 R;
  // op u's entry from LDS into n, then op u + 1's gather and op u + 2's digit word issued
  auto next = [&](int u, ge9_niels& n, bool& neg) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // op u's entry and op u + 1's digit word
    ed_lds_niels9(n, wave_lds, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot read before the next DMA lands
    neg = d_cur < 0;
    d_cur = (int)w_next;
    ed_glds_niels9(ed_b_src(TB, u + 1, d_cur), wl);
    if (u + 2 < N) w_next = dw[u + 2];
  };
  {  // op 0: identity + q0 (fe9.h ge9_from_niels_half: one product instead of an addition's seven)
    ge9_niels n;
    bool neg;
    next(0, n, neg);
    ge9_from_niels_half(R, n, neg);
  }
  for (int u = 1; u + 1 < N; ++u) {
    ge9_niels n;
    bool neg;
    next(u, n, neg);
    ge9_madd_half<true>(R, R, n, neg);
  }
  {  // the last addition: projective output
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ge9_niels n;
    ed_lds_niels9(n, wave_lds, lane);
    ge9_madd_half<false>(R, R, n, d_cur < 0);
  }
  ge9_to_p2(out, R);
}

// Encode for K items per lane, one inversion per lane (k_ed_finish's batching: a wave takes 64 x K
// consecutive items, lane l the items l, l + 64, ... of them). Item p of rin is encoded into
// out[16 p, +8) when pend[p] == want.
template <int K>
__device__ __forceinline__ void ed_encode_run(uint64_t unit, uint64_t end, uint32_t* __restrict__ out,
                                              const ge_p2* __restrict__ rin, const uint8_t* __restrict__ pend,
                                              uint8_t want) {
  const uint64_t base = (unit >> 6) * (64 * K) + (unit & 63);
  fe acc[K];
  fe run;
  fe_1(run);
  uint32_t todo = 0;
  for (uint32_t k = 0; k < (uint32_t)K; ++k) {
    const uint64_t p = base + 64 * k;
    const bool pd = p < end && pend[p] == want;
    todo |= (uint32_t)pd << k;
    if (pd) fe_mul(run, run, rin[p].Z);
    fe_copy(acc[k], run);
  }
  if (!todo) return;
  fe inv;
  fe_invert(inv, run);
  for (int k = K - 1; k >= 0; --k) {
    if (!((todo >> k) & 1u)) continue;
    const uint64_t p = base + 64 * (uint32_t)k;
    const ge_p2 P = rin[p];
    fe zi, t;
    if (k > 0) fe_mul(zi, inv, acc[k - 1]);
    else fe_copy(zi, inv);
    fe_mul(t, inv, P.Z);
    fe_copy(inv, t);
    uint32_t enc[8];
    ed_encode(enc, P, zi);
#pragma unroll
    for (int w = 0; w < 8; ++w) out[16 * p + w] = enc[w];
  }
}

}  // namespace cg
