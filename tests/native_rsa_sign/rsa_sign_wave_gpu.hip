// Test-only device library over corda_amd/csrc/rsa_sign_wave.h (tests/rsasignwave.py,
// tests/test_gpu_rsa_sign_wave.py): the paired product, the windowed ladder and the CRT private-key
// operation with its consistency check, called with chosen operands and chosen signer records, which
// no key that passes cg_rsa_signers_load can steer. One kernel, launched as k_rsa_sign is: 256-thread
// blocks, one wave per case, K taken from the record as the sign kernel takes it. A case is one
// RsaSignerRec (made by the test from Python integers), two operands of 128 limbs and 128 limbs of
// result. Paired operands: the p side's limb j at [j], the q side's at [64 + j]. Nothing of this file
// goes into libcordagpu.so; the kernel below is a second instantiation of the same header.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cordagpu.h"
#include "../../corda_amd/csrc/rsa_sign_wave.h"

#define RS_LIMBS 128u
enum { RS_MONT2 = 0, RS_MODEXP2 = 1, RS_CRT = 2 };

namespace {

template <int K>
__device__ __forceinline__ void rs_case(uint32_t op, const RsaSignerRec* rec, const uint32_t* __restrict__ a,
                                        const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                                        uint32_t* __restrict__ status, uint32_t lane, uint32_t* tab) {
  const uint32_t Lh = __builtin_amdgcn_readfirstlane(rec->Lh);
  const uint32_t side = lane >> 5, hl = lane & 31u;
  if (op == RS_CRT) {
    uint32_t x[K], s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = a[K * lane + k];
    const bool ok = cg::rsa_crt_sign_wave<K>(s, x, rec, lane, tab);
#pragma unroll
    for (int k = 0; k < K; ++k) out[K * lane + k] = s[k];
    if (K == 1) out[64 + lane] = 0;
    if (lane == 0) *status = ok ? 0u : (uint32_t)CG_SIGN_CHECK_FAILED;
    return;
  }
  const uint32_t n0inv = side ? rec->n0inv_q : rec->n0inv_p;
  uint32_t x[K], y[K], m[K], r[K];
  cg::rsa2_load<K>(m, rec->p, rec->q, lane);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    x[k] = a[64 * side + K * hl + k];
    y[k] = b[64 * side + K * hl + k];
  }
  if (op == RS_MONT2) {
    cg::rsa2_mont_mul<K>(r, x, y, m, n0inv, Lh, lane);
  } else {  // x^e in each half, as rsa_crt_halves runs it: into Montgomery form, the ladder, out of it
    uint32_t rr[K], ex[K], one[K], xm[K], t[K];
    cg::rsa2_load<K>(rr, rec->rr_p, rec->rr_q, lane);
    cg::rsa2_load<K>(ex, rec->dp, rec->dq, lane);
#pragma unroll
    for (int k = 0; k < K; ++k) one[k] = (K * hl + k == 0) ? 1u : 0u;
    cg::rsa2_mont_mul<K>(xm, x, rr, m, n0inv, Lh, lane);
    cg::rsa2_mont_mul<K>(t, rr, one, m, n0inv, Lh, lane);
    cg::rsa2_modexp_win<K>(r, xm, t, ex, m, n0inv, Lh, lane, tab);
    cg::rsa2_mont_mul<K>(r, r, one, m, n0inv, Lh, lane);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[64 * side + K * hl + k] = r[k];
  if (K == 1) out[64 * side + 32 + hl] = 0;
  if (lane == 0) *status = 0;
}

__global__ void __launch_bounds__(256) k_rsa_sign_wave_op(uint32_t op, uint32_t count, const RsaSignerRec* recs,
                                                          const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                          uint32_t* __restrict__ out, uint32_t* __restrict__ status) {
  __shared__ uint32_t tab_all[4 * RSA_SIGN_TAB_WORDS];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t c = blockIdx.x * (blockDim.x >> 6) + wv;  // one wave per case
  if (c >= count) return;                                  // the whole wave leaves
  const RsaSignerRec* rec = recs + c;
  const uint32_t K = __builtin_amdgcn_readfirstlane(rec->K);
  const size_t o = (size_t)c * RS_LIMBS;
  uint32_t* tab = tab_all + wv * RSA_SIGN_TAB_WORDS;
  if (K == 1) rs_case<1>(op, rec, a + o, b + o, out + o, status + c, lane, tab);
  else rs_case<2>(op, rec, a + o, b + o, out + o, status + c, lane, tab);
}

}  // namespace

extern "C" {

unsigned rs_rec_bytes() { return (unsigned)sizeof(RsaSignerRec); }

// count cases (host memory): recs of count records, a, b, out of count * 128 limbs, status of count words.
// Returns the HIP error (0: success), or -1 for arguments the kernel must not see.
int rs_run(uint32_t op, uint32_t count, const void* recs, const uint32_t* a, const uint32_t* b, uint32_t* out,
           uint32_t* status) {
  if (count == 0) return 0;
  if (count > (1u << 16) || op > RS_CRT) return -1;
  const RsaSignerRec* r = (const RsaSignerRec*)recs;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t K = r[i].K, L = r[i].L, Lh = r[i].Lh;
    if ((K != 1 && K != 2) || Lh < 1 || Lh > 32 * K || L < 1 || L > 64 * K || L > 2 * Lh) return -1;
  }
  const size_t big = (size_t)count * RS_LIMBS * sizeof(uint32_t), small = (size_t)count * sizeof(uint32_t);
  const size_t rb = (size_t)count * sizeof(RsaSignerRec);
  uint8_t* d = nullptr;  // a | b | out | status | recs
  hipError_t err = hipMalloc((void**)&d, 3 * big + small + rb);
  if (err != hipSuccess) return (int)err;
  uint32_t* da = (uint32_t*)d;
  uint32_t* db = (uint32_t*)(d + big);
  uint32_t* dout = (uint32_t*)(d + 2 * big);
  uint32_t* dst = (uint32_t*)(d + 3 * big);
  RsaSignerRec* dr = (RsaSignerRec*)(d + 3 * big + small);
  static_assert(sizeof(RsaSignerRec) % 4 == 0, "record alignment");
  err = hipMemcpy(da, a, big, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(db, b, big, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(dr, recs, rb, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemset(dout, 0xA5, big + small);  // every limb of the result is written
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_rsa_sign_wave_op, dim3((count + 3) / 4), dim3(256), 0, 0, op, count, dr, da, db, dout, dst);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out, dout, big, hipMemcpyDeviceToHost);
  if (err == hipSuccess) err = hipMemcpy(status, dst, small, hipMemcpyDeviceToHost);
  (void)hipMemset(d, 0, 3 * big + small + rb);
  hipFree(d);
  return (int)err;
}

}  // extern "C"
