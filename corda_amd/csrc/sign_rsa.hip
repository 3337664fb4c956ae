// RSA_SHA256 (RSASSA-PSS) signing kernels for gfx950: BC 1.57 PSSSigner.generateSignature behind
// Crypto.doSign (core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:395-402, 415-422), the 32-byte
// salt drawn by the caller. Lane code: rsa_sign_wave.h (the CRT exponentiations), rsa.h (EMSA-PSS).
//   k_rsa_signer_expand  one wave per signer: the range checks, limbs of n, p, q, dP, dQ, qInv, the
//                        Montgomery constants of n, p and q (R = 2^(32 Lh) for both primes), q R mod n,
//                        and a self-test: a fixed value signed through the CRT path must come back under e
//   k_rsa_sign_prep      one lane per request: the empty and range checks, mHash = SHA-256(M) (the splice
//                        form from the template's midstate), H = SHA-256(0^8 || mHash || salt); H, the
//                        salt, the signer and a pending mark go to the workspace
//   k_rsa_sign           one request per wavefront, persistent grid: EM in LDS (one MGF1 block per lane),
//                        EM^dP mod p and EM^dQ mod q at once in the two halves of the wave (fixed 4-bit
//                        windows, 16 powers per half in LDS), h = qInv (m1 - m2) mod p, s = m2 + h q, then
//                        s^e mod n compared with EM: a signature that fails it is never written
// The signer store, the workspace (H, salt) and the LDS table are secret; the kernels zero their LDS, the
// host zeroes the workspace behind the last kernel. The LDS address of a table read depends on a window
// digit and the conditional subtraction branches on the operands: not constant-time (Signing
// (RSA-PSS)).
#include "keyws.h"

#include "rsa_sign_wave.h"

namespace cg {

#define RSA_SIGN_PENDING 1u
#define RSA_SIGN_EM_LDS 528u  // 512 EM / signature bytes + slack, per wave
static_assert(CG_RSA_SIG_SLOT == CG_RSA_SIG_MAX, "slot size");
static_assert(sizeof(cg_rsa_signer) == 52, "cg_rsa_signer layout");

// Workspace of a chunk of n requests: [H 8 words x n][salt 8 words x n][signer u32 x n][pend bytes n]
struct SignRsaWs {
  uint32_t *h, *salt, *signer;
  uint8_t* pend;
};
static inline SignRsaWs sign_rsa_ws(void* base, uint64_t n_items) {
  const size_t n = n_items ? n_items : 1;
  uint8_t* p = (uint8_t*)base;
  SignRsaWs w;
  w.h = (uint32_t*)p;
  p += al256(32 * n);
  w.salt = (uint32_t*)p;
  p += al256(32 * n);
  w.signer = (uint32_t*)p;
  p += al256(4 * n);
  w.pend = p;
  return w;
}
size_t sign_rsa_ws_bytes(uint64_t n_items) {
  const size_t n = n_items ? n_items : 1;
  return 2 * al256(32 * n) + al256(4 * n) + al256(n);
}
size_t rsa_signer_bytes() { return sizeof(RsaSignerRec); }

// One big-endian unsigned byte string of a signer inside `secrets`: leading zero bytes dropped.
struct RsaNum {
  uint64_t off;
  uint32_t len, bits;
  bool ok;
};
__device__ __forceinline__ RsaNum rsa_num(const uint8_t* sec, uint64_t sec_len, uint32_t off, uint32_t len,
                                          uint32_t max_len) {
  RsaNum v;
  v.off = off;
  v.len = len;
  v.bits = 0;
  v.ok = in_arena(off, len, sec_len) && len <= max_len + 1u;  // BigInteger.toByteArray's sign byte
  if (!v.ok) return v;
  const uint64_t lr = round4(sec_len);
  while (v.len > 0 && rsa_byte(sec, lr, v.off) == 0) {
    ++v.off;
    --v.len;
  }
  if (v.len == 0) return v;
  const uint32_t top = rsa_byte(sec, lr, v.off);
  v.bits = 8u * (v.len - 1u) + (32u - (uint32_t)__builtin_clz(top));
  v.ok = v.len <= max_len;
  return v;
}

// The full-width limbs of a number (K = 1: up to 64 limbs)
template <int K>
__device__ __forceinline__ void rsa_num_limbs(uint32_t w[K], const uint8_t* sec, uint64_t sec_len, const RsaNum& v,
                                              uint32_t lane) {
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = rsa_be_limb(sec, round4(sec_len), v.off, v.len, K * lane + k);
}

// Constants of n at width K and the self-test. Returns whether the signer signs.
template <int K>
__device__ __forceinline__ bool rsa_signer_finish(RsaSignerRec* rec, const uint8_t* sec, uint64_t sec_len,
                                                  const RsaNum& vn, const uint32_t q1[1], uint32_t lane,
                                                  uint32_t* tab) {
  const uint32_t L = (vn.bits + 31) / 32;
  uint32_t n[K], rr[K], qf[K];
  rsa_num_limbs<K>(n, sec, sec_len, vn, lane);
  const uint32_t n0inv = rsa_n0inv(__shfl(n[0], 0, 64));
  rsa_rr_wave<K>(rr, n, n0inv, L, vn.bits, lane);
  // q from the K = 1 layout (limb `lane`) to this one
  tab[lane] = q1[0];
  rsa_wave_sync();
#pragma unroll
  for (int k = 0; k < K; ++k) qf[k] = K * lane + k < 64u ? tab[K * lane + k] : 0u;
  rsa_wave_sync();
  rsa_mont_mul<K>(qf, qf, rr, n, n0inv, L, lane);  // q R_n mod n (q < n)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    rec->n[K * lane + k] = n[k];
    rec->rr_n[K * lane + k] = rr[k];
    rec->qr_n[K * lane + k] = qf[k];
    if (K == 1) rec->n[64 + lane] = rec->rr_n[64 + lane] = rec->qr_n[64 + lane] = 0;
  }
  if (lane == 0) {
    rec->n0inv_n = n0inv;
    rec->K = K;
  }
  __threadfence();
  rsa_wave_sync();
  // the self-test value: below 2^(32 (L - 1)) < n
  uint32_t x[K], s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = K * lane + k < L - 1 ? 0x9E3779B9u * (K * lane + k + 1u) : 0u;
  return rsa_crt_sign_wave<K>(s, x, rec, lane, tab);
}

__global__ void __launch_bounds__(64) k_rsa_signer_expand(const cg_rsa_signer* __restrict__ signers, uint32_t n_signers,
                                                          const uint8_t* __restrict__ sec, uint64_t sec_len,
                                                          RsaSignerRec* recs, uint8_t* __restrict__ status) {
  __shared__ uint32_t tab[RSA_SIGN_TAB_WORDS];
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= n_signers) return;
  const cg_rsa_signer sg = signers[i];
  RsaSignerRec* rec = recs + i;
  // every lane runs the (uniform) checks
  const RsaNum vn = rsa_num(sec, sec_len, sg.n_off, sg.n_len, RSA_MAX_BITS / 8);
  const RsaNum vp = rsa_num(sec, sec_len, sg.p_off, sg.p_len, RSA_MAX_BITS / 16);
  const RsaNum vq = rsa_num(sec, sec_len, sg.q_off, sg.q_len, RSA_MAX_BITS / 16);
  const RsaNum vdp = rsa_num(sec, sec_len, sg.dp_off, sg.dp_len, RSA_MAX_BITS / 16);
  const RsaNum vdq = rsa_num(sec, sec_len, sg.dq_off, sg.dq_len, RSA_MAX_BITS / 16);
  const RsaNum vqi = rsa_num(sec, sec_len, sg.qinv_off, sg.qinv_len, RSA_MAX_BITS / 16);
  const bool inside = in_arena(sg.n_off, sg.n_len, sec_len) && in_arena(sg.p_off, sg.p_len, sec_len) &&
                      in_arena(sg.q_off, sg.q_len, sec_len) && in_arena(sg.dp_off, sg.dp_len, sec_len) &&
                      in_arena(sg.dq_off, sg.dq_len, sec_len) && in_arena(sg.qinv_off, sg.qinv_len, sec_len);
  const uint64_t lr = round4(sec_len);
  uint32_t st = 0;
  if (!inside) st = CG_KEY_INVALID;
  else if (vn.bits < RSA_MIN_BITS || vn.bits > RSA_MAX_BITS || vp.bits > RSA_MAX_BITS / 2 || vq.bits > RSA_MAX_BITS / 2)
    st = CG_UNSUPPORTED;
  else if (!vn.ok || !vp.ok || !vq.ok || !vdp.ok || !vdq.ok || !vqi.ok || sg.e == 0 || vp.bits < 2 || vq.bits < 2)
    st = CG_KEY_INVALID;
  else if (!(rsa_byte(sec, lr, vn.off + vn.len - 1) & rsa_byte(sec, lr, vp.off + vp.len - 1) &
             rsa_byte(sec, lr, vq.off + vq.len - 1) & 1u))
    st = CG_KEY_INVALID;  // n, p or q even
  const uint32_t L = (vn.bits + 31) / 32;
  const uint32_t Lh = ((vp.bits > vq.bits ? vp.bits : vq.bits) + 31) / 32;
  if (st == 0 && L > 2 * Lh) st = CG_KEY_INVALID;  // p q < n
  bool ok = st == 0;
  if (ok) {
    // the halves at K = 1 over the whole wave (Lh <= 64 limbs)
    uint32_t p[1], q[1], dp[1], dq[1], qi[1], rr[1], r3[1];
    rsa_num_limbs<1>(p, sec, sec_len, vp, lane);
    rsa_num_limbs<1>(q, sec, sec_len, vq, lane);
    rsa_num_limbs<1>(dp, sec, sec_len, vdp, lane);
    rsa_num_limbs<1>(dq, sec, sec_len, vdq, lane);
    rsa_num_limbs<1>(qi, sec, sec_len, vqi, lane);
    if (rsa_geq<1>(dp, p) || rsa_geq<1>(dq, q) || rsa_geq<1>(qi, p)) {
      st = CG_KEY_INVALID;
      ok = false;
    } else {
      const uint32_t n0p = rsa_n0inv(__shfl(p[0], 0, 64)), n0q = rsa_n0inv(__shfl(q[0], 0, 64));
      rec->p[lane] = p[0];
      rec->q[lane] = q[0];
      rec->dp[lane] = dp[0];
      rec->dq[lane] = dq[0];
      rec->qinv[lane] = qi[0];
      rsa_rr_wave<1>(rr, p, n0p, Lh, vp.bits, lane);
      rsa_mont_mul<1>(r3, rr, rr, p, n0p, Lh, lane);
      rec->rr_p[lane] = rr[0];
      rec->r3_p[lane] = r3[0];
      rsa_rr_wave<1>(rr, q, n0q, Lh, vq.bits, lane);
      rsa_mont_mul<1>(r3, rr, rr, q, n0q, Lh, lane);
      rec->rr_q[lane] = rr[0];
      rec->r3_q[lane] = r3[0];
      if (lane == 0) {
        rec->bits = vn.bits;
        rec->L = L;
        rec->Lh = Lh;
        rec->k = (vn.bits + 7) / 8;
        rec->em_bits = vn.bits - 1;
        rec->block_len = (vn.bits + 6) / 8;
        rec->e = sg.e;
        rec->n0inv_p = n0p;
        rec->n0inv_q = n0q;
      }
      if (L > 64 || Lh > 32) ok = rsa_signer_finish<2>(rec, sec, sec_len, vn, q, lane, tab);
      else ok = rsa_signer_finish<1>(rec, sec, sec_len, vn, q, lane, tab);
      if (!ok) st = CG_KEY_INVALID;  // p q != n or wrong CRT parts
    }
  }
  rsa_wave_sync();
  if (!ok) {  // nothing of a refused key stays
    uint32_t* w = (uint32_t*)rec;
    for (uint32_t j = lane; j < sizeof(RsaSignerRec) / 4; j += 64) w[j] = 0u;
  }
  for (uint32_t j = lane; j < RSA_SIGN_TAB_WORDS; j += 64) tab[j] = 0u;
  __threadfence();
  rsa_wave_sync();
  if (lane == 0) {
    rec->ok = ok ? 1u : 0u;
    status[i] = (uint8_t)st;
  }
}

// not signed: the status, 512 zero bytes and length 0, never stale memory
__device__ __forceinline__ void sr_refuse(uint64_t p, uint8_t st, uint32_t* __restrict__ sigs,
                                          uint16_t* __restrict__ sig_len, uint8_t* __restrict__ status) {
  for (int k = 0; k < CG_RSA_SIG_SLOT / 4; ++k) sigs[(CG_RSA_SIG_SLOT / 4) * p + k] = 0u;
  sig_len[p] = 0;
  status[p] = st;
}

template <bool Fused>
__global__ void __launch_bounds__(256) k_rsa_sign_prep(
    const void* __restrict__ reqs, uint64_t n, const RsaSignerRec* __restrict__ store, uint32_t n_signers,
    const cg_signable_tmpl* __restrict__ tmpls, uint32_t n_tmpls, uint64_t n_ids, const uint8_t* __restrict__ arena,
    uint64_t arena_len, const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ salts,
    uint32_t* __restrict__ sigs, uint16_t* __restrict__ sig_len, uint8_t* __restrict__ status, SignRsaWs ws) {
  for (Walk w = walk_units(n); w.u < w.end; w.u += w.step) {
    const uint64_t p = w.u;
    const SignMsg m = sign_msg<Fused>(reqs, p, n_signers, tmpls, n_tmpls, n_ids, arena_len);
    uint8_t st = m.st;
    if (st == 0 && store[m.signer].ok == 0) st = CG_NOT_RUN;  // refused at load
    if (st != 0) {
      ws.pend[p] = 0;
      sr_refuse(p, st, sigs, sig_len, status);
      continue;
    }
    uint32_t mh[8], salt[8], h[8];
    if (Fused) {
      const TmplMid* mid = (const TmplMid*)(msgs + SPLICE_HDR_BYTES) + m.tmpl;
      sha256_ld_suffix(mh, tmpl_splice(m.tmpl, m.at, msgs), 0, m.len, (const uint32_t*)nullptr, mid->state, mid->blocks);
    } else {
      sha256_ld_suffix(mh, ArenaLd{arena, round4(arena_len)}, m.at, m.len, (const uint32_t*)nullptr);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) salt[q] = CG_BSWAP32(salts[8 * p + q]);
    rsa_pss_h(h, mh, salt);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      ws.h[8 * p + q] = h[q];
      ws.salt[8 * p + q] = salt[q];
    }
    ws.signer[p] = m.signer;
    ws.pend[p] = RSA_SIGN_PENDING;
  }
}

// One request on one wave. em: the wave's RSA_SIGN_EM_LDS bytes, tab: its RSA_SIGN_TAB_WORDS.
template <int K>
__device__ __forceinline__ void rsa_sign_wave(const RsaSignerRec* rec, const uint32_t* __restrict__ h,
                                              const uint32_t* __restrict__ salt, uint32_t* __restrict__ sig,
                                              uint16_t* __restrict__ sig_len, uint8_t* __restrict__ status, uint8_t* em,
                                              uint32_t* tab, uint32_t lane) {
  const uint32_t block_len = __builtin_amdgcn_readfirstlane(rec->block_len);
  const uint32_t em_bits = __builtin_amdgcn_readfirstlane(rec->em_bits);
  const uint32_t kbytes = __builtin_amdgcn_readfirstlane(rec->k);
  for (uint32_t pos = lane; pos < block_len; pos += 64) em[pos] = (uint8_t)rsa_pss_plain_byte(pos, block_len, salt, h);
  rsa_wave_sync();
  const uint32_t db_len = block_len - RSA_HASH_LEN - 1u;
  if (32u * lane < db_len) rsa_pss_unmask_block(em, db_len, lane);  // db_len <= 479: at most 15 lanes
  rsa_wave_sync();
  if (lane == 0) rsa_pss_clear_top(em, block_len, em_bits);
  rsa_wave_sync();
  uint32_t x[K], s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t j = 4 * (K * lane + k) + b;  // byte j from the least significant end
      if (j < block_len) v |= (uint32_t)em[block_len - 1 - j] << (8 * b);
    }
    x[k] = v;
  }
  rsa_wave_sync();
  const bool ok = rsa_crt_sign_wave<K>(s, x, rec, lane, tab);
  // k big-endian bytes, zeros to the end of the slot
  for (uint32_t j = lane; j < CG_RSA_SIG_SLOT / 4; j += 64) ((uint32_t*)em)[j] = 0u;
  rsa_wave_sync();
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t j = 4 * (K * lane + k) + b;
      if (j < kbytes) em[kbytes - 1 - j] = (uint8_t)(s[k] >> (8 * b));
    }
  }
  rsa_wave_sync();
  for (uint32_t j = lane; j < CG_RSA_SIG_SLOT / 4; j += 64) sig[j] = ((const uint32_t*)em)[j];
  rsa_wave_sync();
  for (uint32_t j = lane; j < RSA_SIGN_EM_LDS / 4; j += 64) ((uint32_t*)em)[j] = 0u;
  if (lane == 0) {
    *sig_len = ok ? (uint16_t)kbytes : (uint16_t)0;
    *status = ok ? 0 : CG_SIGN_CHECK_FAILED;
  }
  rsa_wave_sync();
}

__global__ void __launch_bounds__(256) k_rsa_sign(uint64_t n, const RsaSignerRec* store, uint32_t* __restrict__ sigs,
                                                  uint16_t* __restrict__ sig_len, uint8_t* __restrict__ status,
                                                  SignRsaWs ws) {
  __shared__ __attribute__((aligned(16))) uint32_t tab_all[4 * RSA_SIGN_TAB_WORDS];
  __shared__ __attribute__((aligned(16))) uint8_t em_all[4 * RSA_SIGN_EM_LDS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  uint32_t* tab = tab_all + wv * RSA_SIGN_TAB_WORDS;
  uint8_t* em = em_all + wv * RSA_SIGN_EM_LDS;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t p = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv; p < n; p += waves) {
    if (__builtin_amdgcn_readfirstlane((uint32_t)ws.pend[p]) != RSA_SIGN_PENDING) continue;
    const RsaSignerRec* rec = store + __builtin_amdgcn_readfirstlane(ws.signer[p]);
    const uint32_t K = __builtin_amdgcn_readfirstlane(rec->K);
    uint32_t* sig = sigs + (CG_RSA_SIG_SLOT / 4) * p;
    if (K == 1) rsa_sign_wave<1>(rec, ws.h + 8 * p, ws.salt + 8 * p, sig, sig_len + p, status + p, em, tab, lane);
    else rsa_sign_wave<2>(rec, ws.h + 8 * p, ws.salt + 8 * p, sig, sig_len + p, status + p, em, tab, lane);
  }
}

hipError_t launch_rsa_signer_expand(const void* d_signers_in, uint32_t n, const uint8_t* d_secrets, uint64_t secrets_len,
                                    void* d_store, uint8_t* d_status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rsa_signer_expand, dim3(n), dim3(64), 0, stream, (const cg_rsa_signer*)d_signers_in, n, d_secrets,
                     secrets_len, (RsaSignerRec*)d_store, d_status);
  return hipGetLastError();
}

hipError_t launch_sign_rsa(const SignRsaArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const uint32_t B = 256;
  const SignRsaWs ws = sign_rsa_ws(a.d_ws, a.n);
  const RsaSignerRec* store = (const RsaSignerRec*)a.d_signers;
  uint32_t* sigs = (uint32_t*)a.d_sigs;
  const unsigned hgrid = walk_grid(a.n, B, WALK_CAP(4));
  if (a.fused)
    hipLaunchKernelGGL(k_rsa_sign_prep<true>, dim3(hgrid), dim3(B), 0, stream, a.d_reqs, a.n, store, a.n_signers,
                       a.d_tmpls, a.n_tmpls, a.n_ids, a.d_arena, a.arena_len, a.d_msgs, (const uint32_t*)a.d_salts, sigs,
                       a.d_sig_len, a.d_status, ws);
  else
    hipLaunchKernelGGL(k_rsa_sign_prep<false>, dim3(hgrid), dim3(B), 0, stream, a.d_reqs, a.n, store, a.n_signers,
                       a.d_tmpls, a.n_tmpls, a.n_ids, a.d_arena, a.arena_len, a.d_msgs, (const uint32_t*)a.d_salts, sigs,
                       a.d_sig_len, a.d_status, ws);
  // one wave per request at most
  const unsigned grid = walk_grid((a.n + 3) / 4 * 256, B, WALK_CAP(4));
  hipLaunchKernelGGL(k_rsa_sign, dim3(grid), dim3(B), 0, stream, a.n, store, sigs, a.d_sig_len, a.d_status, ws);
  return hipGetLastError();
}

}  // namespace cg
