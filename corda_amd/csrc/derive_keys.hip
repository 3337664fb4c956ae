// Key derivation kernels: Crypto.deriveKeyPair (core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:
// 646-771) and, for cg_public_keys, its second half alone (private key -> public key). Lane code: derive.h.
//   k_derive_parents     one lane per parent: the checks, then the SHA-512 midstates after K xor ipad and
//                        after K xor opad (two of an item's four compressions, once per parent)
//   k_derive_mac         one lane per item: the range checks, HMAC-SHA512 over the seed bytes (inner hash
//                        resumed from the ipad midstate, one outer block); Ed25519: the child seed out,
//                        SHA-512(child seed), clamp, the table digits into the item slot; ECDSA: d, the
//                        accept rule and the bounded rehash loop in the lane, d out and into the slot
//   k_public_prep        the same hand-off for cg_public_keys: the secrets are given
//   k_derive_ed_ab       Ed25519 items: a B over the constant table (ed_lds.h ed_fixed_base_pf)
//   k_derive_ed_encode   DERIVE_RUN_K items per lane, one inversion per lane: Abyte, then 32 zero bytes
//   k_derive_ec_mul<C>   curve C's items: d G over the constant G table (ec_add_g_wide), Jacobian
//   k_derive_ec_affine<C> DERIVE_RUN_K items per lane, one inversion per lane (m29_invert_run's prefix
//                        products, Z re-read in the back pass): X || Y big-endian, the status byte
// One lane per item, persistent walk_units grids, one stream. Each scheme's kernels pass over the
// other schemes' items (the class byte `pend`). The workspace (midstates, slots) is secret; the host
// zeroes it behind the last kernel. The table gathers are indexed by digits of the child scalar: not
// constant-time (Key derivation).
#include "ed_lds.h"
#include "keyws.h"

#include "derive.h"

namespace cg {

#ifndef DERIVE_RUN_K
#define DERIVE_RUN_K 16
#endif

__constant__ EcConsts c_dk_ec[2];  // [CG_CURVE_K1], [CG_CURVE_R1]: this translation unit's copy

hipError_t derive_upload_constants() {
  EcConsts k[2];
  ec_consts_init<CG_CURVE_K1>(k[CG_CURVE_K1]);
  ec_consts_init<CG_CURVE_R1>(k[CG_CURVE_R1]);
  return hipMemcpyToSymbol(HIP_SYMBOL(c_dk_ec), k, sizeof k, 0, hipMemcpyHostToDevice);
}

// Item classes in `pend`: 0 nothing to do (the status byte is final), else the scheme's kernels run
enum { DK_NONE = 0, DK_ED = 1, DK_EC = 2 /* + curve */ };

// Workspace of a call with n_parents parents and chunks of at most n items:
// [mids: n_parents x HmacMid][pst: n_parents status bytes][slots: n x ITEM_SLOT][pend: n bytes]
// slots: Ed25519 the digits, then a B (ge_p2); ECDSA d (u256w), then d G (Jac).
struct DeriveWs {
  HmacMid* mids;
  uint8_t* pst;
  void* slots;
  uint8_t* pend;
};
static inline DeriveWs derive_ws(void* base, uint32_t n_parents, uint64_t n_items) {
  const size_t np = n_parents ? n_parents : 1, n = n_items ? n_items : 1;
  uint8_t* p = (uint8_t*)base;
  DeriveWs w;
  w.mids = (HmacMid*)p;
  p += al256(np * sizeof(HmacMid));
  w.pst = p;
  p += al256(np);
  w.slots = p;
  p += al256(n * ITEM_SLOT);
  w.pend = p;
  return w;
}
size_t derive_ws_bytes(uint32_t n_parents, uint64_t n_items) {
  const size_t np = n_parents ? n_parents : 1, n = n_items ? n_items : 1;
  return al256(np * sizeof(HmacMid)) + al256(np) + al256(n * ITEM_SLOT) + al256(n);
}
static_assert(sizeof(Jac) <= ITEM_SLOT && sizeof(u256w) <= ITEM_SLOT, "an ECDSA item fits the item slot");
static_assert(4 * EdWideCfg::kBPackedWords <= ITEM_SLOT, "the digits fit the item slot");

__device__ __forceinline__ int dk_curve(uint8_t scheme) {  // -1: not an ECDSA scheme
  return scheme == CG_ECDSA_SECP256R1_SHA256 ? CG_CURVE_R1 : scheme == CG_ECDSA_SECP256K1_SHA256 ? CG_CURVE_K1 : -1;
}

__global__ void __launch_bounds__(64) k_derive_parents(const cg_derive_parent* __restrict__ parents, uint32_t n,
                                                       const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                       DeriveWs ws) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const cg_derive_parent k = parents[i];
  uint8_t st = 0;
  if (k.scheme != CG_EDDSA_ED25519_SHA512 && dk_curve(k.scheme) < 0) st = CG_UNSUPPORTED;
  else if (k.key_len == 0 || k.key_len > 128) st = CG_DERIVE_BAD_PARENT;
  else if (!in_arena(k.key_off, k.key_len, arena_len)) st = CG_NOT_RUN;
  ws.pst[i] = st;
  if (st != 0) return;
  HmacMid m;
  hmac512_midstates(m, ArenaLd{arena, round4(arena_len)}, k.key_off, k.key_len);
  ws.mids[i] = m;
}

// The hand-off of an accepted item to its scheme's kernels; everything else gets its final bytes here.
__device__ __forceinline__ void dk_zero_out(uint32_t* __restrict__ secrets, uint32_t* __restrict__ pubs, uint64_t p,
                                            bool secret_too) {
#pragma unroll
  for (int k = 0; k < 16; ++k) pubs[16 * p + k] = 0u;
  if (secret_too) {
#pragma unroll
    for (int k = 0; k < 8; ++k) secrets[8 * p + k] = 0u;
  }
}
// Ed25519: EdDSAPrivateKeySpec(seed)'s scalar as table digits into the slot; the second half of the
// 64 output bytes is zero
__device__ __forceinline__ void dk_ed_handoff(const uint32_t seed[8], uint32_t* __restrict__ pubs, uint64_t p,
                                              const DeriveWs& ws) {
  EdSigner sg;
  uint32_t es[EdWideCfg::kBPackedWords];
  ed_signer_scalars(sg, es, seed);
  uint32_t* o = (uint32_t*)((uint8_t*)ws.slots + (size_t)p * ITEM_SLOT);
#pragma unroll
  for (int k = 0; k < EdWideCfg::kBPackedWords; ++k) o[k] = es[k];
#pragma unroll
  for (int k = 8; k < 16; ++k) pubs[16 * p + k] = 0u;
  ws.pend[p] = DK_ED;
}
__device__ __forceinline__ void dk_ec_handoff(const u256w& d, int curve, uint64_t p, const DeriveWs& ws) {
  *(u256w*)((uint8_t*)ws.slots + (size_t)p * ITEM_SLOT) = d;
  ws.pend[p] = (uint8_t)(DK_EC + curve);
}

#ifndef DERIVE_HASH_WAVES  // as k_ed_hash and k_ed_sign_nonce: the SHA-512 rounds are a dependent chain per lane
#define DERIVE_HASH_WAVES 4
#endif
__global__ void __launch_bounds__(256, DERIVE_HASH_WAVES) k_derive_mac(
    const cg_derive_parent* __restrict__ parents, uint32_t n_parents, const cg_derive_req* __restrict__ reqs,
    uint64_t n, const uint8_t* __restrict__ arena, uint64_t arena_len, uint32_t force, uint32_t* __restrict__ secrets,
    uint32_t* __restrict__ pubs, uint8_t* __restrict__ status, uint8_t* __restrict__ retries, DeriveWs ws) {
  const ArenaLd ld{arena, round4(arena_len)};
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    const cg_derive_req q = reqs[p];
    uint8_t st = CG_NOT_RUN, scheme = 0;
    if (q.parent < n_parents && in_arena(q.seed_off, q.seed_len, arena_len)) {
      st = ws.pst[q.parent];
      scheme = parents[q.parent].scheme;
    }
    uint32_t tries = 0;
    uint32_t mac[16];
    if (st == 0) {
      const HmacMid& m = ws.mids[q.parent];
      const int curve = dk_curve(scheme);
      if (curve < 0) {
        hmac512_ld(mac, m, ld, q.seed_off, q.seed_len);
        dk_ed_handoff(mac, pubs, p, ws);
      } else {
        u256w d;
        st = ec_derive_scalar(d, mac, tries, curve, force, m, ld, q.seed_off, q.seed_len);
        if (st == 0) dk_ec_handoff(d, curve, p, ws);
      }
    }
    if (retries) retries[p] = (uint8_t)tries;
    status[p] = st;  // an ECDSA item's byte is final unless d G comes out infinite (k_derive_ec_mul)
    if (st != 0) {
      ws.pend[p] = DK_NONE;
      dk_zero_out(secrets, pubs, p, true);
      continue;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) secrets[8 * p + k] = mac[k];
  }
}

// cg_public_keys: secrets in (32 bytes each, one scheme), the same hand-off
__global__ void __launch_bounds__(256, DERIVE_HASH_WAVES) k_public_prep(uint8_t scheme,
                                                                        const uint32_t* __restrict__ secrets,
                                                                        uint64_t n, uint32_t* __restrict__ pubs,
                                                                        uint8_t* __restrict__ status, DeriveWs ws) {
  const int curve = dk_curve(scheme);
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    uint32_t s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = secrets[8 * p + k];
    if (curve < 0) {
      dk_ed_handoff(s, pubs, p, ws);
      status[p] = 0;
      continue;
    }
    u256w d;
    ec_secret_from_be(d, s);
    const bool ok = ec_secret_accept(curve, d);
    status[p] = ok ? 0 : CG_KEY_REJECTED;
    if (ok) {
      dk_ec_handoff(d, curve, p, ws);
    } else {
      ws.pend[p] = DK_NONE;
      dk_zero_out(nullptr, pubs, p, false);
    }
  }
}

#ifndef DERIVE_AB_WAVES
#define DERIVE_AB_WAVES 2  // k_ed_sign_rb's bound: the fe9 additions need ~106 VGPRs
#endif
#ifndef DERIVE_AB_OCC  // the waves per SIMD the register use allows (the persistent grid's cap)
#define DERIVE_AB_OCC 4
#endif
__global__ void __launch_bounds__(256, DERIVE_AB_WAVES) k_derive_ed_ab(uint64_t n, const EdBWideTab* __restrict__ btab,
                                                                       DeriveWs ws) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[4 * kNiels9WaveBytes];
  uint8_t* wave_lds = stage + (threadIdx.x >> 6) * kNiels9WaveBytes;
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    if (ws.pend[p] != DK_ED) continue;
    // every lane still here runs the same DMA sequence; the LDS image is per lane: no barrier
    ge_p2 q;
    ed_fixed_base_pf(q, (const uint32_t*)((const uint8_t*)ws.slots + (size_t)p * ITEM_SLOT), *btab, wave_lds,
                     __lane_id());
    ((ge_p2*)ws.slots)[p] = q;
  }
}

__global__ void __launch_bounds__(256) k_derive_ed_encode(uint64_t n, uint32_t* __restrict__ pubs, DeriveWs ws) {
  const uint64_t units = (n + 64 * DERIVE_RUN_K - 1) / (64 * DERIVE_RUN_K) * 64;
  for (Walk w = walk_units(units); w.u < w.end; w.u += w.step)
    ed_encode_run<DERIVE_RUN_K>(w.u, n, pubs, (const ge_p2*)ws.slots, ws.pend, DK_ED);
}

template <int C>
__global__ void __launch_bounds__(256) k_derive_ec_mul(uint64_t n, const EcGWideTab* __restrict__ gtab,
                                                       uint32_t* __restrict__ secrets, uint32_t* __restrict__ pubs,
                                                       uint8_t* __restrict__ status, DeriveWs ws) {
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    if (ws.pend[p] != DK_EC + C) continue;
    if (!ec_slot_fixed_base<C>((uint8_t*)ws.slots + (size_t)p * ITEM_SLOT, *gtab, c_dk_ec[C])) {
      // Crypto.kt:729-731 (pointQ.isInfinity): not reachable for 2 <= d < n; left to the host
      ws.pend[p] = DK_NONE;  // (secrets: null in the public-key form, where they are the caller's input)
      status[p] = secrets ? CG_DERIVE_HOST : CG_KEY_REJECTED;
      dk_zero_out(secrets, pubs, p, secrets != nullptr);
    }
  }
}

// Affine X || Y for DERIVE_RUN_K items per lane with one inversion per lane: the prefix products of
// m29_invert_run, with ed_encode_run's walk (Z is read again in the back pass, so only the K prefix
// products live in the lane).
template <int C>
__device__ __forceinline__ void dk_ec_affine_run(uint64_t unit, uint64_t end, uint32_t* __restrict__ pubs,
                                                 const DeriveWs& ws) {
  const EcConsts& K = c_dk_ec[C];
  const uint8_t* slots = (const uint8_t*)ws.slots;
  const uint64_t base = (unit >> 6) * (64 * DERIVE_RUN_K) + (unit & 63);
  f29 acc[DERIVE_RUN_K];
  f29 run = K.one_p;
  uint32_t todo = 0;
  for (uint32_t k = 0; k < DERIVE_RUN_K; ++k) {
    const uint64_t p = base + 64 * k;
    const bool pd = p < end && ws.pend[p] == DK_EC + C;
    todo |= (uint32_t)pd << k;
    if (pd) m29_mul<C, 0>(run, run, ((const Jac*)(slots + (size_t)p * ITEM_SLOT))->Z);
    acc[k] = run;
  }
  if (!todo) return;
  f29 inv;
  m29_inv<C, 0>(inv, run, K.one_p);
  for (int k = DERIVE_RUN_K - 1; k >= 0; --k) {
    if (!((todo >> k) & 1u)) continue;
    const uint64_t p = base + 64 * (uint32_t)k;
    const Jac P = *(const Jac*)(slots + (size_t)p * ITEM_SLOT);
    f29 zi;
    if (k > 0) m29_mul<C, 0>(zi, inv, acc[k - 1]);
    else zi = inv;
    m29_mul<C, 0>(inv, inv, P.Z);
    uint32_t xy[16];
    ec_affine_be<C>(xy, P, zi);
#pragma unroll
    for (int w = 0; w < 16; ++w) pubs[16 * p + w] = xy[w];
  }
}
template <int C>
__global__ void __launch_bounds__(256) k_derive_ec_affine(uint64_t n, uint32_t* __restrict__ pubs, DeriveWs ws) {
  const uint64_t units = (n + 64 * DERIVE_RUN_K - 1) / (64 * DERIVE_RUN_K) * 64;
  for (Walk w = walk_units(units); w.u < w.end; w.u += w.step) dk_ec_affine_run<C>(w.u, n, pubs, ws);
}

hipError_t launch_derive_parents(const DeriveArgs& a, hipStream_t stream) {
  if (a.n_parents == 0) return hipSuccess;
  const uint32_t B = 64;  // parents are few: spread them over CUs
  hipLaunchKernelGGL(k_derive_parents, dim3((a.n_parents + B - 1) / B), dim3(B), 0, stream, a.d_parents, a.n_parents,
                     a.d_arena, a.arena_len, derive_ws(a.d_ws, a.n_parents, a.n));
  return hipGetLastError();
}

// One chunk: a.d_reqs != null derives (a.d_secrets is written), else a.d_secrets holds the private
// keys of a.scheme. Only the kernels of schemes the chunk can hold are launched when that is known.
hipError_t launch_derive(const DeriveArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const uint32_t B = 256;
  const DeriveWs ws = derive_ws(a.d_ws, a.n_parents, a.n);
  uint32_t *secrets = a.d_reqs ? (uint32_t*)a.d_secrets : nullptr, *pubs = (uint32_t*)a.d_pubs;
  const unsigned hgrid = walk_grid(a.n, B, WALK_CAP(DERIVE_HASH_WAVES));
  bool ed = true, k1 = true, r1 = true;
  if (a.d_reqs) {
    hipLaunchKernelGGL(k_derive_mac, dim3(hgrid), dim3(B), 0, stream, a.d_parents, a.n_parents, a.d_reqs, a.n,
                       a.d_arena, a.arena_len, a.force_retries, secrets, pubs, a.d_status, a.d_retries, ws);
  } else {
    ed = a.scheme == CG_EDDSA_ED25519_SHA512;
    k1 = a.scheme == CG_ECDSA_SECP256K1_SHA256;
    r1 = a.scheme == CG_ECDSA_SECP256R1_SHA256;
    hipLaunchKernelGGL(k_public_prep, dim3(hgrid), dim3(B), 0, stream, a.scheme, (const uint32_t*)a.d_secrets, a.n,
                       pubs, a.d_status, ws);
  }
  const uint64_t units = (a.n + 64 * DERIVE_RUN_K - 1) / (64 * DERIVE_RUN_K) * 64;
  const unsigned rgrid = walk_grid(units, B, WALK_CAP(2)), mgrid = walk_grid(a.n, B, WALK_CAP(2));
  if (ed) {
    hipLaunchKernelGGL(k_derive_ed_ab, dim3(walk_grid(a.n, B, WALK_CAP(DERIVE_AB_OCC))), dim3(B), 0, stream, a.n,
                       bwide(a.d_btab), ws);
    hipLaunchKernelGGL(k_derive_ed_encode, dim3(rgrid), dim3(B), 0, stream, a.n, pubs, ws);
  }
  if (k1) {
    hipLaunchKernelGGL(k_derive_ec_mul<CG_CURVE_K1>, dim3(mgrid), dim3(B), 0, stream, a.n,
                       gwide(a.d_btab, CG_CURVE_K1), secrets, pubs, a.d_status, ws);
    hipLaunchKernelGGL(k_derive_ec_affine<CG_CURVE_K1>, dim3(rgrid), dim3(B), 0, stream, a.n, pubs, ws);
  }
  if (r1) {
    hipLaunchKernelGGL(k_derive_ec_mul<CG_CURVE_R1>, dim3(mgrid), dim3(B), 0, stream, a.n,
                       gwide(a.d_btab, CG_CURVE_R1), secrets, pubs, a.d_status, ws);
    hipLaunchKernelGGL(k_derive_ec_affine<CG_CURVE_R1>, dim3(rgrid), dim3(B), 0, stream, a.n, pubs, ws);
  }
  return hipGetLastError();
}

}  // namespace cg
