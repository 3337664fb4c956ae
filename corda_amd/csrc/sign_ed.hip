// Ed25519 (EDDSA_ED25519_SHA512) signing kernels: i2p 0.2.0 EdDSAEngine.engineSign, RFC 8032's
// deterministic signature, behind Crypto.doSign (core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:
// 395-402, 415-422; NotaryService.kt:77-80).
//   k_ed_signer_expand   one lane per signer: EdDSAPrivateKeySpec(seed) -> (a, prefix, Abyte) into the
//                        context's signer store, Abyte to the caller
//   k_ed_sign_nonce      one lane per item: range and empty checks, r = SHA-512(prefix || M) mod L into
//                        the r column, its fixed-base table digits into the item slot
//   k_ed_sign_rb         R' = r B: 10 / 11 / 12 mixed additions over the constant radix-2^26 / 2^24 /
//                        2^22 table, no doublings; each entry gathered into LDS one op ahead
//   k_ed_sign_encode     ED_FINISH_K items per lane: one inversion per lane, Rbytes to sigs[64 i, +32)
//   k_ed_sign_s          k = SHA-512(Rbytes || Abyte || M) mod L, S = (r + k a) mod L to
//                        sigs[64 i + 32, +32), the status byte
// One lane per item, persistent walk_units grids, one stream. The signer store, the r column and the
// digit slots are secret (given one r, a = (S - r) / k); the host zeroes the workspace behind the last
// kernel. The table gathers are indexed by digits of r: not constant-time (Signing).
#include "ed_lds.h"
#include "keyws.h"

namespace cg {

#ifndef ED_FINISH_K
#define ED_FINISH_K 16
#endif

// Sign workspace of a chunk of n items: [slots: n x ITEM_SLOT (digits, then R')][r: 8 x n u32, word w
// of item p at r[w * n + p]][pend: n bytes]
struct SignWs {
  void* slots;
  uint32_t* r;
  uint8_t* pend;
  uint64_t n;
};
static inline SignWs sign_ws(void* base, uint64_t n_items) {
  const size_t n = n_items ? n_items : 1;
  uint8_t* p = (uint8_t*)base;
  SignWs w;
  w.n = n;
  w.slots = p;
  p += al256(n * ITEM_SLOT);
  w.r = (uint32_t*)p;
  p += al256(8 * n * sizeof(uint32_t));
  w.pend = p;
  return w;
}
size_t sign_ws_bytes(uint64_t n_items) {
  const size_t n = n_items ? n_items : 1;
  return al256(n * ITEM_SLOT) + al256(8 * n * sizeof(uint32_t)) + al256(n);
}
size_t signer_bytes() { return sizeof(EdSigner); }
static_assert(4 * EdWideCfg::kBPackedWords <= ITEM_SLOT, "the digits fit the item slot");
static_assert(EdWideCfg::kBBits == 32, "k_ed_sign_rb reads one digit per word");

__global__ void __launch_bounds__(64) k_ed_signer_expand(const uint32_t* __restrict__ seeds, uint32_t n,
                                                         EdSigner* __restrict__ store, uint32_t* __restrict__ pub,
                                                         const EdBWideTab* __restrict__ btab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t seed[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) seed[w] = seeds[8 * (size_t)i + w];
  EdSigner sg;
  ed_signer_expand(sg, seed, *btab);
  store[i] = sg;
#pragma unroll
  for (int w = 0; w < 8; ++w) pub[8 * (size_t)i + w] = sg.abyte[w];
}

// SHA-512(prefix (PW words) || M) for the item's message. A wave whose items share one template reads
// the image with scalar addresses (keyws.h tmpl_splice); the 64-byte prefix then runs block 1 from the
// template's precomputed schedule, as k_ed_hash does. The secret 32-byte prefix never takes a schedule.
template <bool Fused, int PW>
__device__ __forceinline__ void sign_hash(uint32_t hw[16], const uint32_t* prefix, const SignMsg& m,
                                          const uint8_t* __restrict__ arena, uint64_t arena_len,
                                          const uint8_t* __restrict__ msgs) {
  if (Fused) {
    const uint32_t t0 = __builtin_amdgcn_readfirstlane(m.tmpl);
    if (__builtin_amdgcn_ballot_w64(m.tmpl != t0) == 0) {
      const uint64_t* wk1 = nullptr;
      if (PW == 16) {
        const TmplMid* m0 = (const TmplMid*)(msgs + SPLICE_HDR_BYTES) + t0;
        if (m0->ed_mid) wk1 = ((const TmplW512*)(msgs + ((const SpliceHdr*)msgs)->w512_off) + t0)->wk;
      }
      sha512_prefix_splice<PW>(hw, prefix, tmpl_splice(t0, m.at, msgs), __builtin_amdgcn_readfirstlane(m.len), wk1);
    } else {
      sha512_prefix_splice<PW>(hw, prefix, tmpl_splice(m.tmpl, m.at, msgs), m.len, (const uint64_t*)nullptr);
    }
  } else {
    sha512_prefix_ld<PW>(hw, prefix, ArenaLd{arena, round4(arena_len)}, m.at, m.len);
  }
}

#ifndef ED_SIGN_HASH_WAVES  // as k_ed_hash: the SHA-512 rounds are a dependent chain per lane
#define ED_SIGN_HASH_WAVES 4
#endif
template <bool Fused>
__global__ void __launch_bounds__(256, ED_SIGN_HASH_WAVES) k_ed_sign_nonce(
    const void* __restrict__ reqs, uint64_t n, const EdSigner* __restrict__ store, uint32_t n_signers,
    const cg_signable_tmpl* __restrict__ tmpls, uint32_t n_tmpls, uint64_t n_ids, const uint8_t* __restrict__ arena,
    uint64_t arena_len, const uint8_t* __restrict__ msgs, uint32_t* __restrict__ sigs, uint8_t* __restrict__ status,
    SignWs ws) {
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    const SignMsg m = sign_msg<Fused>(reqs, p, n_signers, tmpls, n_tmpls, n_ids, arena_len);
    ws.pend[p] = m.st == 0;
    if (m.st != 0) {  // not signed: the status and 64 zero bytes, never stale memory
      status[p] = m.st;
#pragma unroll
      for (int k = 0; k < 16; ++k) sigs[16 * p + k] = 0u;
      continue;
    }
    uint32_t pre[8], hw[16], r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) pre[k] = store[m.signer].prefix[k];
    sign_hash<Fused, 8>(hw, pre, m, arena, arena_len, msgs);
    sc_reduce512(r, hw);
#pragma unroll
    for (int k = 0; k < 8; ++k) ws.r[(size_t)k * ws.n + p] = r[k];
    uint32_t es[EdWideCfg::kBPackedWords];
    sc_recode_wb<ED_WIDE_BW, EdWideCfg::kBBits>(es, EdWideCfg::kBPackedWords, r);
    uint32_t* o = (uint32_t*)((uint8_t*)ws.slots + (size_t)p * ITEM_SLOT);
#pragma unroll
    for (int k = 0; k < EdWideCfg::kBPackedWords; ++k) o[k] = es[k];
  }
}

#ifndef ED_SIGN_RB_WAVES
#define ED_SIGN_RB_WAVES 2  // k_ed_ladder_wide's bound: the fe9 additions need ~106 VGPRs
#endif
#ifndef ED_SIGN_RB_OCC  // the waves per SIMD the register use allows (the persistent grid's cap)
#define ED_SIGN_RB_OCC 4
#endif
__global__ void __launch_bounds__(256, ED_SIGN_RB_WAVES) k_ed_sign_rb(uint64_t n, const EdBWideTab* __restrict__ btab,
                                                                      SignWs ws) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[4 * kNiels9WaveBytes];
  uint8_t* wave_lds = stage + (threadIdx.x >> 6) * kNiels9WaveBytes;
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    if (!ws.pend[p]) continue;
    // every lane still here runs the same DMA sequence; the LDS image is per lane: no barrier
    ge_p2 q;
    ed_fixed_base_pf(q, (const uint32_t*)((const uint8_t*)ws.slots + (size_t)p * ITEM_SLOT), *btab, wave_lds,
                     __lane_id());
    ((ge_p2*)ws.slots)[p] = q;
  }
}

__global__ void __launch_bounds__(256) k_ed_sign_encode(uint64_t n, uint32_t* __restrict__ sigs, SignWs ws) {
  const uint64_t units = (n + 64 * ED_FINISH_K - 1) / (64 * ED_FINISH_K) * 64;
  for (Walk w = walk_units(units); w.u < w.end; w.u += w.step) ed_encode_run<ED_FINISH_K>(w.u, n, sigs, (const ge_p2*)ws.slots, ws.pend, 1);
}

template <bool Fused>
__global__ void __launch_bounds__(256, ED_SIGN_HASH_WAVES) k_ed_sign_s(
    const void* __restrict__ reqs, uint64_t n, const EdSigner* __restrict__ store, uint32_t n_signers,
    const cg_signable_tmpl* __restrict__ tmpls, uint32_t n_tmpls, uint64_t n_ids, const uint8_t* __restrict__ arena,
    uint64_t arena_len, const uint8_t* __restrict__ msgs, uint32_t* __restrict__ sigs, uint8_t* __restrict__ status,
    SignWs ws) {
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    if (!ws.pend[p]) continue;
    const SignMsg m = sign_msg<Fused>(reqs, p, n_signers, tmpls, n_tmpls, n_ids, arena_len);
    const EdSigner* sg = store + m.signer;
    uint32_t pre[16], hw[16], k[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      pre[q] = sigs[16 * p + q];
      pre[8 + q] = sg->abyte[q];
    }
    sign_hash<Fused, 16>(hw, pre, m, arena, arena_len, msgs);
    sc_reduce512(k, hw);
    uint32_t a[8], r[8], S[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      a[q] = sg->a[q];
      r[q] = ws.r[(size_t)q * ws.n + p];
    }
    sc_muladd(S, k, a, r);
#pragma unroll
    for (int q = 0; q < 8; ++q) sigs[16 * p + 8 + q] = S[q];
    status[p] = 0;
  }
}

hipError_t launch_signer_expand(const uint8_t* d_seeds, uint32_t n, void* d_signers, uint8_t* d_pubkeys,
                                const void* d_btab, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t B = 64;  // signers are few: spread them over CUs
  hipLaunchKernelGGL(k_ed_signer_expand, dim3((n + B - 1) / B), dim3(B), 0, stream, (const uint32_t*)d_seeds, n,
                     (EdSigner*)d_signers, (uint32_t*)d_pubkeys, bwide(d_btab));
  return hipGetLastError();
}

hipError_t launch_sign(const SignArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const uint32_t B = 256;
  const SignWs ws = sign_ws(a.d_ws, a.n);
  const EdSigner* store = (const EdSigner*)a.d_signers;
  uint32_t* sigs = (uint32_t*)a.d_sigs;
  const unsigned hgrid = walk_grid(a.n, B, WALK_CAP(ED_SIGN_HASH_WAVES));
  if (a.fused)
    hipLaunchKernelGGL(k_ed_sign_nonce<true>, dim3(hgrid), dim3(B), 0, stream, a.d_reqs, a.n, store, a.n_signers,
                       a.d_tmpls, a.n_tmpls, a.n_ids, a.d_arena, a.arena_len, a.d_msgs, sigs, a.d_status, ws);
  else
    hipLaunchKernelGGL(k_ed_sign_nonce<false>, dim3(hgrid), dim3(B), 0, stream, a.d_reqs, a.n, store, a.n_signers,
                       a.d_tmpls, a.n_tmpls, a.n_ids, a.d_arena, a.arena_len, a.d_msgs, sigs, a.d_status, ws);
  hipLaunchKernelGGL(k_ed_sign_rb, dim3(walk_grid(a.n, B, WALK_CAP(ED_SIGN_RB_OCC))), dim3(B), 0, stream, a.n,
                     bwide(a.d_btab), ws);
  const uint64_t units = (a.n + 64 * ED_FINISH_K - 1) / (64 * ED_FINISH_K) * 64;
  hipLaunchKernelGGL(k_ed_sign_encode, dim3(walk_grid(units, B, WALK_CAP(2))), dim3(B), 0, stream, a.n, sigs, ws);
  if (a.fused)
    hipLaunchKernelGGL(k_ed_sign_s<true>, dim3(hgrid), dim3(B), 0, stream, a.d_reqs, a.n, store, a.n_signers,
                       a.d_tmpls, a.n_tmpls, a.n_ids, a.d_arena, a.arena_len, a.d_msgs, sigs, a.d_status, ws);
  else
    hipLaunchKernelGGL(k_ed_sign_s<false>, dim3(hgrid), dim3(B), 0, stream, a.d_reqs, a.n, store, a.n_signers,
                       a.d_tmpls, a.n_tmpls, a.n_ids, a.d_arena, a.arena_len, a.d_msgs, sigs, a.d_status, ws);
  return hipGetLastError();
}

}  // namespace cg
