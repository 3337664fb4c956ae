// The LDS staging of a wide-table entry one op ahead of its addition, shared by the Ed25519 ladders
// (verify_ed.hip) and the signer's fixed-base kernel (sign_ed.hip): the entry is gathered straight into
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

}  // namespace cg
