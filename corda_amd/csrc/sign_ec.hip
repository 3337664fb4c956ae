// ECDSA (ECDSA_SECP256K1_SHA256 / ECDSA_SECP256R1_SHA256) signing kernels: BC 1.57 ECDSASigner.
// generateSignature behind Crypto.doSign (core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:395-402,
// 415-422; NotaryService.kt:73-80), the nonce k drawn by the caller. Lane code: sign_ec.h.
//   k_ec_signer_expand   one lane per signer: 0 < d < n, d into the context's signer store in the form
//                        the finish kernel multiplies with, Q = d G (ec_fixed_base), X || Y to the caller
//   k_ec_sign_prep       one lane per item: the empty and range checks, e = SHA-256(M) (the splice form
//                        from the template's midstate, no message in HBM), 0 < k < n, k into the item
//                        slot and the k column, e and the signer into theirs
//   k_ec_sign_mul<C>     curve C's items: k G over the constant G table (ec_slot_fixed_base, the code of
//                        k_derive_ec_mul), Jacobian into the slot
//   k_ec_sign_finish<C>  SIGN_EC_RUN_K items per lane, two inversions per lane, each through prefix
//                        products: Z mod p (r = x mod n into the slot), then k mod n; s = k^-1 (e + r d),
//                        the refusals r = 0 / s = 0, BC's DER bytes, the length and status bytes
// One lane per item, persistent walk_units grids, one stream. Each curve's kernels pass over the other
// curve's items (the class byte `pend`). The signer store and the workspace (k, k G, e) are secret; the
// host zeroes the workspace behind the last kernel. The table gathers are indexed by digits of k: not
// constant-time (Signing (ECDSA)).
#include "keyws.h"

#include "sign_ec.h"

namespace cg {

#ifndef SIGN_EC_RUN_K
#define SIGN_EC_RUN_K 16
#endif

__constant__ EcConsts c_se_ec[2];  // [CG_CURVE_K1], [CG_CURVE_R1]: this translation unit's copy

hipError_t sign_ec_upload_constants() {
  EcConsts k[2];
  ec_consts_init<CG_CURVE_K1>(k[CG_CURVE_K1]);
  ec_consts_init<CG_CURVE_R1>(k[CG_CURVE_R1]);
  return hipMemcpyToSymbol(HIP_SYMBOL(c_se_ec), k, sizeof k, 0, hipMemcpyHostToDevice);
}

// Item classes in `pend`: 0 nothing to do (the status byte is final), else 1 + curve
enum { SE_NONE = 0, SE_EC = 1 /* + curve */ };

// Workspace of a chunk of n items: [slots: n x ITEM_SLOT (k, then k G, then r)][k: 8 x n u32, word w of
// item p at k[w * n + p]][e: the same][signer: n u32][pend: n bytes]
struct SignEcWs {
  void* slots;
  uint32_t *k, *e, *signer;
  uint8_t* pend;
  uint64_t n;
};
static inline SignEcWs sign_ec_ws(void* base, uint64_t n_items) {
  const size_t n = n_items ? n_items : 1;
  uint8_t* p = (uint8_t*)base;
  SignEcWs w;
  w.n = n;
  w.slots = p;
  p += al256(n * ITEM_SLOT);
  w.k = (uint32_t*)p;
  p += al256(8 * n * sizeof(uint32_t));
  w.e = (uint32_t*)p;
  p += al256(8 * n * sizeof(uint32_t));
  w.signer = (uint32_t*)p;
  p += al256(n * sizeof(uint32_t));
  w.pend = p;
  return w;
}
size_t sign_ec_ws_bytes(uint64_t n_items) {
  const size_t n = n_items ? n_items : 1;
  return al256(n * ITEM_SLOT) + 2 * al256(8 * n * sizeof(uint32_t)) + al256(n * sizeof(uint32_t)) + al256(n);
}
size_t ec_signer_bytes() { return sizeof(EcSigner); }
static_assert(sizeof(Jac) <= ITEM_SLOT && sizeof(u256w) <= ITEM_SLOT, "an ECDSA item fits the item slot");

template <int C>
__device__ __forceinline__ void se_expand(EcSigner& sg, uint32_t xy[16], const u256w& d, const EcGWideTab& tg) {
  const EcConsts& K = c_se_ec[C];
  ec_signer_init<C>(sg, d, K);
  Jac Q;
  if (!ec_fixed_base<C>(Q, d, tg, K)) {  // not reachable for 0 < d < n: G has prime order n
    sg.cls = 0;
    return;
  }
  f29 zi;
  m29_inv<C, 0>(zi, Q.Z, K.one_p);
  ec_affine_be<C>(xy, Q, zi);
}

__global__ void __launch_bounds__(64) k_ec_signer_expand(const uint8_t* __restrict__ schemes,
                                                         const uint32_t* __restrict__ secrets, uint32_t n,
                                                         EcSigner* __restrict__ store, uint32_t* __restrict__ pubs,
                                                         uint8_t* __restrict__ status,
                                                         const EcGWideTab* __restrict__ gk1,
                                                         const EcGWideTab* __restrict__ gr1) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t scheme = schemes[i];
  const int curve = scheme == CG_ECDSA_SECP256R1_SHA256 ? CG_CURVE_R1 : scheme == CG_ECDSA_SECP256K1_SHA256 ? CG_CURVE_K1 : -1;
  uint32_t b[8], xy[16];
#pragma unroll
  for (int w = 0; w < 8; ++w) b[w] = secrets[8 * (size_t)i + w];
#pragma unroll
  for (int w = 0; w < 16; ++w) xy[w] = 0;
  u256w d;
  ec_secret_from_be(d, b);
  EcSigner sg;
  f29_zero(sg.d_m);
  sg.cls = 0;
  uint8_t st = 0;
  if (curve < 0) st = CG_UNSUPPORTED;
  else if (!ec_scalar_in_range(curve, d)) st = CG_KEY_INVALID;
  else if (curve == CG_CURVE_R1) se_expand<CG_CURVE_R1>(sg, xy, d, *gr1);
  else se_expand<CG_CURVE_K1>(sg, xy, d, *gk1);
  if (st == 0 && sg.cls == 0) st = CG_KEY_INVALID;
  if (st != 0) {
    f29_zero(sg.d_m);
#pragma unroll
    for (int w = 0; w < 16; ++w) xy[w] = 0;
  }
  store[i] = sg;
  status[i] = st;
#pragma unroll
  for (int w = 0; w < 16; ++w) pubs[16 * (size_t)i + w] = xy[w];
}

// not signed: the status, 72 zero bytes and length 0, never stale memory
__device__ __forceinline__ void se_refuse(uint64_t p, uint8_t st, uint32_t* __restrict__ sigs,
                                          uint8_t* __restrict__ sig_len, uint8_t* __restrict__ status) {
#pragma unroll
  for (int k = 0; k < CG_EC_SIG_WORDS; ++k) sigs[CG_EC_SIG_WORDS * p + k] = 0u;
  sig_len[p] = 0;
  status[p] = st;
}

#ifndef SIGN_EC_HASH_WAVES  // as k_ed_sign_nonce: the SHA-256 rounds are a dependent chain per lane
#define SIGN_EC_HASH_WAVES 4
#endif
template <bool Fused>
__global__ void __launch_bounds__(256, SIGN_EC_HASH_WAVES) k_ec_sign_prep(
    const void* __restrict__ reqs, uint64_t n, const EcSigner* __restrict__ store, uint32_t n_signers,
    const cg_signable_tmpl* __restrict__ tmpls, uint32_t n_tmpls, uint64_t n_ids, const uint8_t* __restrict__ arena,
    uint64_t arena_len, const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ nonces,
    uint32_t* __restrict__ sigs, uint8_t* __restrict__ sig_len, uint8_t* __restrict__ status, SignEcWs ws) {
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    const SignMsg m = sign_msg<Fused>(reqs, p, n_signers, tmpls, n_tmpls, n_ids, arena_len);
    uint8_t st = m.st;
    uint32_t cls = 0;
    if (st == 0) {
      cls = store[m.signer].cls;
      if (cls == 0) st = CG_NOT_RUN;  // refused at load
    }
    u256w k;
    if (st == 0) {
      uint32_t b[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) b[q] = nonces[8 * p + q];
      ec_secret_from_be(k, b);
      if (!ec_scalar_in_range((int)cls - 1, k)) st = CG_NONCE_REJECTED;
    }
    if (st != 0) {
      ws.pend[p] = SE_NONE;
      se_refuse(p, st, sigs, sig_len, status);
      continue;
    }
    uint32_t h[8];
    if (Fused) {
      const TmplMid* mid = (const TmplMid*)(msgs + SPLICE_HDR_BYTES) + m.tmpl;
      sha256_ld_suffix(h, tmpl_splice(m.tmpl, m.at, msgs), 0, m.len, (const uint32_t*)nullptr, mid->state, mid->blocks);
    } else {
      sha256_ld_suffix(h, ArenaLd{arena, round4(arena_len)}, m.at, m.len, (const uint32_t*)nullptr);
    }
    u256w e;
    ec_sign_e(e, h);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      ws.k[(size_t)q * ws.n + p] = k.w[q];
      ws.e[(size_t)q * ws.n + p] = e.w[q];
    }
    ws.signer[p] = m.signer;
    *(u256w*)((uint8_t*)ws.slots + (size_t)p * ITEM_SLOT) = k;
    ws.pend[p] = (uint8_t)cls;  // SE_EC + curve
  }
}

template <int C>
__global__ void __launch_bounds__(256) k_ec_sign_mul(uint64_t n, const EcGWideTab* __restrict__ gtab,
                                                     uint32_t* __restrict__ sigs, uint8_t* __restrict__ sig_len,
                                                     uint8_t* __restrict__ status, SignEcWs ws) {
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    if (ws.pend[p] != SE_EC + C) continue;
    if (!ec_slot_fixed_base<C>((uint8_t*)ws.slots + (size_t)p * ITEM_SLOT, *gtab, c_se_ec[C])) {
      ws.pend[p] = SE_NONE;  // k G infinite: not reachable for 0 < k < n; BC would redraw (r = 0)
      se_refuse(p, CG_NONCE_REJECTED, sigs, sig_len, status);
    }
  }
}

// SIGN_EC_RUN_K items per lane with dk_ec_affine_run's walk, twice: the prefix products of Z mod p
// (r = x mod n parked in the slot), then of k mod n. The two runs share the K prefix products' registers.
template <int C>
__device__ __forceinline__ void se_finish_run(uint64_t unit, uint64_t end, const EcSigner* __restrict__ store,
                                              uint32_t* __restrict__ sigs, uint8_t* __restrict__ sig_len,
                                              uint8_t* __restrict__ status, const SignEcWs& ws) {
  const EcConsts& K = c_se_ec[C];
  uint8_t* slots = (uint8_t*)ws.slots;
  const uint64_t base = (unit >> 6) * (64 * SIGN_EC_RUN_K) + (unit & 63);
  f29 acc[SIGN_EC_RUN_K];
  f29 run = K.one_p;
  uint32_t todo = 0;
  for (uint32_t k = 0; k < SIGN_EC_RUN_K; ++k) {
    const uint64_t p = base + 64 * k;
    const bool pd = p < end && ws.pend[p] == SE_EC + C;
    todo |= (uint32_t)pd << k;
    if (pd) m29_mul<C, 0>(run, run, ((const Jac*)(slots + (size_t)p * ITEM_SLOT))->Z);
    acc[k] = run;
  }
  if (!todo) return;
  f29 inv;
  m29_inv<C, 0>(inv, run, K.one_p);
  for (int k = SIGN_EC_RUN_K - 1; k >= 0; --k) {
    if (!((todo >> k) & 1u)) continue;
    const uint64_t p = base + 64 * (uint32_t)k;
    const Jac P = *(const Jac*)(slots + (size_t)p * ITEM_SLOT);
    f29 zi;
    if (k > 0) m29_mul<C, 0>(zi, inv, acc[k - 1]);
    else zi = inv;
    m29_mul<C, 0>(inv, inv, P.Z);
    u256w r;
    ec_sign_r<C>(r, P, zi);
    *(u256w*)(slots + (size_t)p * ITEM_SLOT) = r;
  }
  // k^-1 mod n
  run = K.one_n;
  for (uint32_t k = 0; k < SIGN_EC_RUN_K; ++k) {
    if ((todo >> k) & 1u) {
      const uint64_t p = base + 64 * k;
      u256w kk;
#pragma unroll
      for (int q = 0; q < 8; ++q) kk.w[q] = ws.k[(size_t)q * ws.n + p];
      f29 km;
      m29_from_plain<C, 1>(km, kk, K.r2_n);
      m29_mul<C, 1>(run, run, km);
    }
    acc[k] = run;
  }
  m29_inv<C, 1>(inv, run, K.one_n);
  for (int k = SIGN_EC_RUN_K - 1; k >= 0; --k) {
    if (!((todo >> k) & 1u)) continue;
    const uint64_t p = base + 64 * (uint32_t)k;
    u256w kk, e;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      kk.w[q] = ws.k[(size_t)q * ws.n + p];
      e.w[q] = ws.e[(size_t)q * ws.n + p];
    }
    f29 km, kinv;
    m29_from_plain<C, 1>(km, kk, K.r2_n);
    if (k > 0) m29_mul<C, 1>(kinv, inv, acc[k - 1]);
    else kinv = inv;
    m29_mul<C, 1>(inv, inv, km);
    const u256w r = *(const u256w*)(slots + (size_t)p * ITEM_SLOT);
    const f29 d_m = store[ws.signer[p]].d_m;
    uint32_t out[CG_EC_SIG_WORDS], len;
    const uint8_t st = ec_sign_finish<C>(out, len, r, e, d_m, kinv);
#pragma unroll
    for (int q = 0; q < CG_EC_SIG_WORDS; ++q) sigs[CG_EC_SIG_WORDS * p + q] = out[q];
    sig_len[p] = (uint8_t)len;
    status[p] = st;
  }
}
template <int C>
__global__ void __launch_bounds__(256) k_ec_sign_finish(uint64_t n, const EcSigner* __restrict__ store,
                                                        uint32_t* __restrict__ sigs, uint8_t* __restrict__ sig_len,
                                                        uint8_t* __restrict__ status, SignEcWs ws) {
  const uint64_t units = (n + 64 * SIGN_EC_RUN_K - 1) / (64 * SIGN_EC_RUN_K) * 64;
  for (Walk w = walk_units(units); w.u < w.end; w.u += w.step) se_finish_run<C>(w.u, n, store, sigs, sig_len, status, ws);
}

hipError_t launch_ec_signer_expand(const uint8_t* d_schemes, const uint8_t* d_secrets, uint32_t n, void* d_signers,
                                   uint8_t* d_pubs, uint8_t* d_status, const void* d_btab, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t B = 64;  // signers are few: spread them over CUs
  hipLaunchKernelGGL(k_ec_signer_expand, dim3((n + B - 1) / B), dim3(B), 0, stream, d_schemes,
                     (const uint32_t*)d_secrets, n, (EcSigner*)d_signers, (uint32_t*)d_pubs, d_status,
                     gwide(d_btab, CG_CURVE_K1), gwide(d_btab, CG_CURVE_R1));
  return hipGetLastError();
}

hipError_t launch_sign_ec(const SignEcArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const uint32_t B = 256;
  const SignEcWs ws = sign_ec_ws(a.d_ws, a.n);
  const EcSigner* store = (const EcSigner*)a.d_signers;
  uint32_t* sigs = (uint32_t*)a.d_sigs;
  const unsigned hgrid = walk_grid(a.n, B, WALK_CAP(SIGN_EC_HASH_WAVES));
  if (a.fused)
    hipLaunchKernelGGL(k_ec_sign_prep<true>, dim3(hgrid), dim3(B), 0, stream, a.d_reqs, a.n, store, a.n_signers,
                       a.d_tmpls, a.n_tmpls, a.n_ids, a.d_arena, a.arena_len, a.d_msgs, (const uint32_t*)a.d_nonces,
                       sigs, a.d_sig_len, a.d_status, ws);
  else
    hipLaunchKernelGGL(k_ec_sign_prep<false>, dim3(hgrid), dim3(B), 0, stream, a.d_reqs, a.n, store, a.n_signers,
                       a.d_tmpls, a.n_tmpls, a.n_ids, a.d_arena, a.arena_len, a.d_msgs, (const uint32_t*)a.d_nonces,
                       sigs, a.d_sig_len, a.d_status, ws);
  const uint64_t units = (a.n + 64 * SIGN_EC_RUN_K - 1) / (64 * SIGN_EC_RUN_K) * 64;
  const unsigned rgrid = walk_grid(units, B, WALK_CAP(2)), mgrid = walk_grid(a.n, B, WALK_CAP(2));
  hipLaunchKernelGGL(k_ec_sign_mul<CG_CURVE_K1>, dim3(mgrid), dim3(B), 0, stream, a.n, gwide(a.d_btab, CG_CURVE_K1),
                     sigs, a.d_sig_len, a.d_status, ws);
  hipLaunchKernelGGL(k_ec_sign_finish<CG_CURVE_K1>, dim3(rgrid), dim3(B), 0, stream, a.n, store, sigs, a.d_sig_len,
                     a.d_status, ws);
  hipLaunchKernelGGL(k_ec_sign_mul<CG_CURVE_R1>, dim3(mgrid), dim3(B), 0, stream, a.n, gwide(a.d_btab, CG_CURVE_R1),
                     sigs, a.d_sig_len, a.d_status, ws);
  hipLaunchKernelGGL(k_ec_sign_finish<CG_CURVE_R1>, dim3(rgrid), dim3(B), 0, stream, a.n, store, sigs, a.d_sig_len,
                     a.d_status, ws);
  return hipGetLastError();
}

}  // namespace cg
