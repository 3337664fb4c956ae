// RSA_SHA256 (RSASSA-PSS) batch verification for gfx950, run only by contexts opened with CG_FLAG_RSA.
//
//   k_rsa_keyprep  one wave per key of the table: strict DER decode (rsa.h rsa_key_decode), n as limbs,
//                  -n^-1 mod 2^32, R^2 mod n, or a "not accepted" mark.
//   k_rsa_select   the indices of the items whose key was accepted, compacted into a list; the count
//                  stays in device memory.
//   k_rsa_verify   one signature per wavefront, limbs spread over the lanes (lane l holds limbs
//                  K l .. K l + K - 1; K = 1 up to 2048 bits, 2 above). s^e mod n by left-to-right
//                  square-and-multiply over operand-scanning Montgomery products: per step the
//                  multiplier limb a_i and the quotient digit m are wave-uniform (v_readlane), each
//                  limb product is one v_mad_u64_u32 into a per-lane 64-bit accumulator, the
//                  accumulator moves down one limb by a DPP wave shift, and the carries the lanes
//                  hold back are resolved once per product with two ballots (generate / propagate).
//                  The messages of a wave's G signatures are hashed first, one lane each, so the
//                  SHA-256 of the clear data runs lane-parallel; G = count / waves, between 1 and 64,
//                  from the device-side count. EMSA-PSS (rsa.h): EM goes to LDS, the MGF1 blocks are
//                  one lane each, the final compare on lane 0.
// The pass overwrites the CG_UNSUPPORTED k_misc_status gave these items and nothing else.
#include "keyws.h"
#include "rsa.h"
#include "rsa_wave.h"

namespace cg {

#define RSA_PENDING 249u
#define RSA_NONE 255u
#define RSA_EM_LDS 528u  // 512 EM bytes + slack, per wave

__global__ void __launch_bounds__(256) k_rsa_select(const cg_item* __restrict__ items, uint32_t n_items,
                                                    const cg_key* __restrict__ keys, uint32_t n_keys,
                                                    const RsaKeyRec* __restrict__ recs, uint32_t* __restrict__ list,
                                                    uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool take = false;
  if (i < n_items) {
    const uint32_t ki = items[i].key_idx;
    take = ki < n_keys && keys[ki].scheme == CG_RSA_SHA256 && recs[ki].ok != 0;
  }
  const uint64_t m = __ballot(take);
  if (m == 0) return;
  const uint32_t lane = threadIdx.x & 63u;
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if ((int)lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = __shfl(base, leader, 64);
  if (take) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
}

// The per-key constants on one wave (limbs over the lanes as in the verify kernel): n, then R mod n
// from 2^(bits - 1) < n by 32 L - bits + 1 modular doublings, then R^2 = 2^(32 L) R mod n as the
// Montgomery form of 2^(32 L): square-and-double over the bits of 32 L (at most 12 products), where
// the scalar form (rsa.h rsa_rr, kept for the host) needs 64 L doublings of L limbs on one lane.
template <int K>
__device__ __forceinline__ void rsa_keyprep_wave(RsaKeyRec* __restrict__ rec, const RsaKeyView& v,
                                                 const uint8_t* __restrict__ arena, uint64_t lr, uint32_t lane) {
  const uint32_t bits = v.bits, L = (bits + 31) / 32;
  uint32_t n[K], x[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    n[k] = rsa_be_limb(arena, lr, v.n_off, v.n_len, K * lane + k);
    x[k] = (K * lane + k == (bits - 1) >> 5) ? 1u << ((bits - 1) & 31u) : 0u;
  }
  const uint32_t n0inv = rsa_n0inv(__shfl(n[0], 0, 64));
  for (uint32_t s = 32 * L - (bits - 1); s > 0; --s) rsa_double_mod_wave<K>(x, n, L, lane);  // R mod n
  rsa_double_mod_wave<K>(x, n, L, lane);                                                    // 2 R: "2"
  const uint32_t E = 32 * L;
  for (int bit = 30 - __builtin_clz(E); bit >= 0; --bit) {
    rsa_mont_mul<K>(x, x, x, n, n0inv, L, lane);
    if ((E >> bit) & 1u) rsa_double_mod_wave<K>(x, n, L, lane);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    rec->n[K * lane + k] = n[k];
    rec->rr[K * lane + k] = x[k];
    if (K == 1) rec->n[64 + lane] = rec->rr[64 + lane] = 0;
  }
  if (lane == 0) {
    rec->bits = bits;
    rec->L = L;
    rec->k = (bits + 7) / 8;
    rec->em_bits = bits - 1;
    rec->block_len = (bits + 6) / 8;
    rec->e = v.e;
    rec->n0inv = n0inv;
    rec->ok = 1;
  }
}

// One wave per key. Every lane runs the (uniform) decode; the constants are lane-cooperative.
__global__ void __launch_bounds__(64) k_rsa_keyprep(const cg_key* __restrict__ keys, uint32_t n_keys,
                                                    const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                    RsaKeyRec* __restrict__ recs) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= n_keys) return;
  const cg_key k = keys[i];
  RsaKeyRec* rec = recs + i;
  const uint64_t lr = round4(arena_len);
  RsaKeyView v;
  const bool ok = k.scheme == CG_RSA_SHA256 && k.fmt == CG_KEY_SPKI && in_arena(k.off, k.len, arena_len) &&
                  rsa_key_decode(v, arena, lr, k.off, k.len);
  if (!ok) {
    if (lane == 0) rec->ok = 0;
    return;
  }
  if (v.bits <= 2048) rsa_keyprep_wave<1>(rec, v, arena, lr, lane);
  else rsa_keyprep_wave<2>(rec, v, arena, lr, lane);
}

// One signature on one wave: s^e mod n, the fit and EMSA-PSS checks. All 64 lanes call it with
// wave-uniform arguments; returns CG_VALID or CG_INVALID (uniform).
template <int K>
__device__ __forceinline__ uint32_t rsa_wave_verify(const RsaKeyRec* __restrict__ rec, uint32_t L, uint32_t e,
                                                    uint32_t n0inv, uint32_t block_len, uint32_t em_bits,
                                                    const uint8_t* __restrict__ arena, uint64_t lr, uint64_t sig_off,
                                                    uint32_t sig_len, const uint32_t mhash[8], uint8_t* em,
                                                    uint32_t lane) {
  uint32_t n[K], s[K], x[K], acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    n[k] = rec->n[K * lane + k];
    x[k] = rec->rr[K * lane + k];
    s[k] = rsa_be_limb(arena, lr, sig_off, sig_len, K * lane + k);
  }
  if (rsa_geq<K>(s, n)) return CG_INVALID;  // RSACoreEngine.convertInput: input too large for RSA cipher
  if (e > 1) {
    RSA_WAVE_LADDER(K, acc, s, x, n, n0inv, L, e, lane)  // rsa_wave.h: rsa_wave_modexp's text, in place
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = s[k];
  }
  // m as block_len big-endian bytes; a set byte above them: the block does not fit (false)
  bool wide = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t j = 4 * (K * lane + k) + b;  // byte j from the least significant end
      const uint32_t v = (acc[k] >> (8 * b)) & 0xffu;
      if (j < block_len) em[block_len - 1 - j] = (uint8_t)v;
      else wide = wide || v != 0;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (__ballot(wide) != 0) return CG_INVALID;
  uint32_t ok = lane == 0 ? (rsa_pss_pre(em, block_len) ? 1u : 0u) : 0u;
  ok = __builtin_amdgcn_readfirstlane(ok);
  if (!ok) return CG_INVALID;
  const uint32_t db_len = block_len - RSA_HASH_LEN - 1u;
  if (32u * lane < db_len) rsa_pss_unmask_block(em, db_len, lane);  // db_len <= 479: at most 15 lanes
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  ok = lane == 0 ? (rsa_pss_post(em, block_len, em_bits, mhash) ? 1u : 0u) : 0u;
  ok = __builtin_amdgcn_readfirstlane(ok);
  return ok ? CG_VALID : CG_INVALID;
}

__global__ void __launch_bounds__(256) k_rsa_verify(const cg_item* __restrict__ items,
                                                    const uint32_t* __restrict__ list,
                                                    const uint32_t* __restrict__ count_p,
                                                    const RsaKeyRec* __restrict__ recs,
                                                    const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                    const uint8_t* __restrict__ msgs, uint64_t msgs_len, uint32_t mode,
                                                    uint8_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint8_t em_all[4 * RSA_EM_LDS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  uint8_t* em = em_all + wv * RSA_EM_LDS;
  const uint32_t count = *count_p;
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  const uint32_t wave_id = blockIdx.x * (blockDim.x >> 6) + wv;
  uint32_t G = count / waves;  // signatures a wave takes per round: their messages hash lane-parallel
  G = G < 1 ? 1 : G > 64 ? 64 : G;
  const uint64_t lr = round4(arena_len);
  for (uint64_t base = (uint64_t)wave_id * G; base < count; base += (uint64_t)waves * G) {
    uint32_t st = RSA_NONE, idx = 0, key = 0, sig_len = 0;
    uint64_t sig_off = 0;
    uint32_t mh[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) mh[q] = 0;
    if (lane < G && base + lane < count) {
      idx = list[base + lane];
      const cg_item it = items[idx];
      key = it.key_idx;
      sig_off = it.sig_off;
      sig_len = it.sig_len;
      if (mode == CG_MODE_DOVERIFY && (it.sig_len == 0 || it.msg_len == 0)) {
        st = CG_EMPTY;
      } else if (!in_arena(it.sig_off, it.sig_len, arena_len) ||
                 (msgs ? !item_fused(it, msgs) : !in_arena(it.msg_off, it.msg_len, arena_len))) {
        st = CG_NOT_RUN;
      } else if (it.sig_len == 0 || it.sig_len > recs[key].k) {
        st = CG_INVALID;  // longer than the modulus: DataLengthException, caught; empty: s = 0
      } else {
        if (msgs) {
          const TmplMid* mid = item_tmpl_mid(it, msgs);
          sha256_ld_suffix(mh, item_splice(it, msgs), 0, it.msg_len, nullptr, mid->state, mid->blocks);
        } else {
          sha256_ld_suffix(mh, ArenaLd{arena, lr}, it.msg_off, it.msg_len, nullptr);
        }
        st = RSA_PENDING;
      }
      if (st != RSA_PENDING) status[idx] = (uint8_t)st;
    }
    for (uint32_t t = 0; t < G; ++t) {
      if ((uint32_t)__shfl((int)st, (int)t, 64) != RSA_PENDING) continue;
      const uint32_t idx_t = __shfl(idx, t, 64);
      const uint32_t key_t = __shfl(key, t, 64);
      const uint32_t sl_t = __shfl(sig_len, t, 64);
      const uint64_t so_t = ((uint64_t)__shfl((uint32_t)(sig_off >> 32), t, 64) << 32) | __shfl((uint32_t)sig_off, t, 64);
      uint32_t mh_t[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) mh_t[q] = __shfl(mh[q], t, 64);
      const RsaKeyRec* rec = recs + key_t;
      const uint32_t L = __builtin_amdgcn_readfirstlane(rec->L);
      const uint32_t e = __builtin_amdgcn_readfirstlane(rec->e);
      const uint32_t n0inv = __builtin_amdgcn_readfirstlane(rec->n0inv);
      const uint32_t block_len = __builtin_amdgcn_readfirstlane(rec->block_len);
      const uint32_t em_bits = __builtin_amdgcn_readfirstlane(rec->em_bits);
      uint32_t v;
      if (L <= 64)
        v = rsa_wave_verify<1>(rec, L, e, n0inv, block_len, em_bits, arena, lr, so_t, sl_t, mh_t, em, lane);
      else
        v = rsa_wave_verify<2>(rec, L, e, n0inv, block_len, em_bits, arena, lr, so_t, sl_t, mh_t, em, lane);
      if (lane == 0) status[idx_t] = (uint8_t)v;
      __builtin_amdgcn_wave_barrier();  // the next signature reuses the wave's EM bytes
    }
  }
}

size_t rsa_keys_bytes(uint32_t n_keys) { return al256((size_t)(n_keys ? n_keys : 1) * sizeof(RsaKeyRec)); }
size_t rsa_list_bytes(uint64_t n_items) {
  const uint64_t n = n_items < kRsaSegment ? n_items : kRsaSegment;
  return 256 + al256((size_t)(n ? n : 1) * sizeof(uint32_t));
}

hipError_t launch_rsa_keyprep(const VerifyReq& r, void* d_rsakeys, hipStream_t stream) {
  if (r.n_keys == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rsa_keyprep, dim3(r.n_keys), dim3(64), 0, stream, r.d_keys, r.n_keys, r.d_arena, r.arena_len,
                     (RsaKeyRec*)d_rsakeys);
  return hipGetLastError();
}

hipError_t launch_rsa_items(const VerifyReq& r, const void* d_rsakeys, void* d_rsalist, hipStream_t stream) {
  if (r.n_keys == 0) return hipSuccess;
  uint32_t* count = (uint32_t*)d_rsalist;
  uint32_t* list = (uint32_t*)((uint8_t*)d_rsalist + 256);
  for (uint64_t f = 0; f < r.n_items; f += kRsaSegment) {
    const uint32_t cnt = (uint32_t)(kRsaSegment < r.n_items - f ? kRsaSegment : r.n_items - f);
    hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rsa_select, dim3((cnt + 255) / 256), dim3(256), 0, stream, r.d_items + f, cnt, r.d_keys,
                       r.n_keys, (const RsaKeyRec*)d_rsakeys, list, count);
    // one wave per listed signature at most; the count is read on the device (no host round trip)
    const unsigned grid = walk_grid(((uint64_t)cnt + 3) / 4 * 256, 256, WALK_CAP(4));
    hipLaunchKernelGGL(k_rsa_verify, dim3(grid), dim3(256), 0, stream, r.d_items + f, (const uint32_t*)list,
                       (const uint32_t*)count, (const RsaKeyRec*)d_rsakeys, r.d_arena, r.arena_len, r.d_msgs,
                       r.msgs_len, r.mode, r.d_status + f);
  }
  return hipGetLastError();
}

}  // namespace cg
