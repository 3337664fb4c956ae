// Test-only device library over corda_amd/csrc/rsa_wave.h (tests/rsawave.py, tests/test_gpu_rsa_wave.py):
// the lane-cooperative primitives of the RSA kernels called with chosen operands, which no valid
// signature can steer. One kernel, launched as k_rsa_verify is: 256-thread blocks, one wave per
// case, K chosen from L as the verify kernel chooses it, all 64 lanes calling. A case is 128 limbs
// per operand (little-endian, zero above L). Nothing of this file goes into libcordagpu.so; the
// kernel below is a separate instantiation of the same header.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../corda_amd/csrc/rsa_wave.h"

#define RW_LIMBS 128u
enum { RW_MONT_MUL = 0, RW_DOUBLE_MOD = 1, RW_GEQ = 2, RW_MODEXP = 3 };

namespace {

template <int K>
__device__ __forceinline__ void rw_case(uint32_t op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                        const uint32_t* __restrict__ n, uint32_t n0inv, uint32_t L, uint32_t e,
                                        uint32_t* __restrict__ out, uint32_t lane) {
  uint32_t x[K], y[K], m[K], r[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    x[k] = a[K * lane + k];
    y[k] = b[K * lane + k];
    m[k] = n[K * lane + k];
    r[k] = 0;
  }
  if (op == RW_MONT_MUL) {
    cg::rsa_mont_mul<K>(r, x, y, m, n0inv, L, lane);
  } else if (op == RW_DOUBLE_MOD) {
    cg::rsa_double_mod_wave<K>(x, m, L, lane);
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = x[k];
  } else if (op == RW_GEQ) {
    const bool ge = cg::rsa_geq<K>(x, y);
    if (lane == 0) r[0] = ge ? 1u : 0u;
  } else {  // the exponent branches of rsa_wave_verify: b holds R^2 mod n
    if (e > 1) {
      cg::rsa_wave_modexp<K>(r, x, y, m, n0inv, L, e, lane);
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) r[k] = x[k];
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[K * lane + k] = r[k];
  if (K == 1) out[64 + lane] = 0;
}

__global__ void __launch_bounds__(256) k_rsa_wave_op(uint32_t op, uint32_t count, const uint32_t* __restrict__ a,
                                                     const uint32_t* __restrict__ b, const uint32_t* __restrict__ n,
                                                     const uint32_t* __restrict__ n0inv, const uint32_t* __restrict__ Ls,
                                                     const uint32_t* __restrict__ es, uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // one wave per case
  if (c >= count) return;                                                  // the whole wave leaves
  const uint32_t L = __builtin_amdgcn_readfirstlane(Ls[c]);
  const uint32_t e = __builtin_amdgcn_readfirstlane(es[c]);
  const uint32_t ni = __builtin_amdgcn_readfirstlane(n0inv[c]);
  const size_t o = (size_t)c * RW_LIMBS;
  if (L <= 64) rw_case<1>(op, a + o, b + o, n + o, ni, L, e, out + o, lane);
  else rw_case<2>(op, a + o, b + o, n + o, ni, L, e, out + o, lane);
}

// count cases: a, b, n, out of count * 128 limbs, n0inv / L / e of count words (host memory).
// Returns the HIP error (0: success), or -1 for arguments the kernel must not see.
int rw_run(uint32_t op, uint32_t count, const uint32_t* a, const uint32_t* b, const uint32_t* n,
           const uint32_t* n0inv, const uint32_t* L, const uint32_t* e, uint32_t* out) {
  if (count == 0) return 0;
  if (count > (1u << 20)) return -1;
  for (uint32_t i = 0; i < count; ++i)
    if (L[i] < 1 || L[i] > RW_LIMBS) return -1;
  const size_t big = (size_t)count * RW_LIMBS * sizeof(uint32_t), small = (size_t)count * sizeof(uint32_t);
  uint32_t* d = nullptr;  // a | b | n | out | n0inv | L | e
  hipError_t err = hipMalloc((void**)&d, 4 * big + 3 * small);
  if (err != hipSuccess) return (int)err;
  uint32_t* da = d;
  uint32_t* db = da + (size_t)count * RW_LIMBS;
  uint32_t* dn = db + (size_t)count * RW_LIMBS;
  uint32_t* dout = dn + (size_t)count * RW_LIMBS;
  uint32_t* dn0 = dout + (size_t)count * RW_LIMBS;
  uint32_t* dL = dn0 + count;
  uint32_t* de = dL + count;
  err = hipMemcpy(da, a, big, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(db, b, big, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(dn, n, big, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(dn0, n0inv, small, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(dL, L, small, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(de, e, small, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemset(dout, 0xA5, big);  // every limb of the result is written
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_rsa_wave_op, dim3((count + 3) / 4), dim3(256), 0, 0, op, count, da, db, dn, dn0, dL, de, dout);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out, dout, big, hipMemcpyDeviceToHost);
  hipFree(d);
  return (int)err;
}

}  // namespace

extern "C" {

int rw_mont_mul(uint32_t count, const uint32_t* a, const uint32_t* b, const uint32_t* n, const uint32_t* n0inv,
                const uint32_t* L, uint32_t* out) {
  return rw_run(RW_MONT_MUL, count, a, b, n, n0inv, L, L, out);
}
int rw_double_mod(uint32_t count, const uint32_t* x, const uint32_t* n, const uint32_t* L, uint32_t* out) {
  return rw_run(RW_DOUBLE_MOD, count, x, x, n, L, L, L, out);
}
// out[128 i] = a_i >= b_i
int rw_geq(uint32_t count, const uint32_t* a, const uint32_t* b, const uint32_t* L, uint32_t* out) {
  return rw_run(RW_GEQ, count, a, b, a, L, L, L, out);
}
int rw_modexp(uint32_t count, const uint32_t* s, const uint32_t* rr, const uint32_t* n, const uint32_t* n0inv,
              const uint32_t* L, const uint32_t* e, uint32_t* out) {
  return rw_run(RW_MODEXP, count, s, rr, n, n0inv, L, e, out);
}

}  // extern "C"
