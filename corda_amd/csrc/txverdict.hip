// Per-transaction verdicts on the device (include/cordagpu.h cg_tx_verdicts; lane logic in txverdict.h).
// The reduction reads what the verify kernels left in HBM: a status byte and a 12- or 24-byte record per
// signature, 24 bytes per transaction, and the small requirement tables; it writes 8 bytes per
// transaction and one per requirement. Memory-bound, no arithmetic to speak of.
//
//   k_tx_verdicts_small  one lane per transaction of up to kTxvSmallMax signatures (the notary shard's
//                        shape: ~5 signatures, 1-3 requirements). Adjacent lanes own adjacent spans, so
//                        a wave's record and status reads cover one contiguous run. Longer
//                        transactions go to a compacted list, one atomic per wave (ballot + popcount).
//   k_tx_verdicts_wave   one wave per listed transaction: lanes stride the span, the first bad
//                        signature is a wave min of (ordinal, status), leaf membership a wave-wide any.
//                        The walk itself runs uniformly on every lane of the wave.
// Both walk persistent, capped grids (keyws.h walk_grid). LDS holds the walk stacks only.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "keyws.h"
#include "txverdict.h"

namespace cg {

namespace {

constexpr uint32_t kTxvBlock = 256;
constexpr uint32_t kTxvStackWords = kTxvFrameWords * CG_REQ_MAX_DEPTH;  // per lane

// ws: [0] the list's length, [4 ..) the listed transaction indices (tx_verdicts_ws_bytes)
template <class Acc>
__global__ __launch_bounds__(kTxvBlock) void k_tx_verdicts_small(Acc acc, TxvTables tb, const cg_tx_check* checks,
                                                                 uint32_t n_tx, cg_tx_verdict* verdicts,
                                                                 uint8_t* req_status, uint32_t* ws) {
  __shared__ uint32_t stack[kTxvStackWords * kTxvBlock];
  const TxvStack st{stack + threadIdx.x, kTxvBlock};
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t step = (uint64_t)gridDim.x * kTxvBlock;
  // `base` is the wave's first transaction, the same on its 64 lanes: the ballot below sees whole waves
  for (uint64_t base = (uint64_t)blockIdx.x * kTxvBlock + (threadIdx.x & ~63u); base < n_tx; base += step) {
    const uint64_t t = base + lane;
    bool big = false;
    cg_tx_check ck;
    if (t < n_tx) {
      ck = checks[t];
      big = ck.n_sigs > kTxvSmallMax;
      if (!big) verdicts[t] = tx_verdict_lane(acc, tb, ck, (uint32_t)t, st, req_status);
    }
    const unsigned long long m = __ballot(big);
    if (m) {
      uint32_t at = 0;
      if (lane == (uint32_t)__ffsll((long long)m) - 1u) at = atomicAdd(ws, (uint32_t)__popcll(m));
      at = __shfl(at, __ffsll((long long)m) - 1);
      if (big) ws[4 + at + __popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)t;  // at most n_tx entries in all
    }
  }
}

template <class Acc>
struct WaveHas {
  const Acc& acc;
  const TxvTables& tb;
  const cg_tx_check& ck;
  uint32_t lane;
  __device__ bool operator()(uint32_t cls) const { return __ballot(span_has(acc, tb, ck, cls, lane, 64u)) != 0ull; }
};

template <class Acc>
__global__ __launch_bounds__(kTxvBlock) void k_tx_verdicts_wave(Acc acc, TxvTables tb, const cg_tx_check* checks,
                                                                uint32_t n_tx, cg_tx_verdict* verdicts,
                                                                uint8_t* req_status, const uint32_t* ws) {
  __shared__ uint32_t stack[kTxvStackWords * kTxvBlock];
  const TxvStack st{stack + threadIdx.x, kTxvBlock};
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (kTxvBlock / 64u);
  uint32_t n = ws[0];
  if (n > n_tx) n = n_tx;
  for (uint64_t w = blockIdx.x * (kTxvBlock / 64u) + (threadIdx.x >> 6); w < n; w += waves) {
    const uint32_t t = ws[4 + w];
    if (t >= n_tx) continue;  // never written by k_tx_verdicts_small; the same on every lane
    const cg_tx_check ck = checks[t];
    const bool in_table = span_in_table(tb, ck);
    TxvSpan sp;
    sp.first = kTxvNoBad;
    sp.flags = 0;
    if (in_table) {
      sp = span_scan(acc, tb, ck, t, lane, 64u);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        TxvSpan other;
        other.first = __shfl_xor((unsigned long long)sp.first, o);
        other.flags = __shfl_xor(sp.flags, o);
        sp = span_join(sp, other);
      }
    }
    WaveHas<Acc> has{acc, tb, ck, lane};
    const cg_tx_verdict v = tx_requirements(tb, ck, in_table, sp, has, st, req_status, lane == 0);
    if (lane == 0) verdicts[t] = v;
  }
}

template <class Acc>
hipError_t launch_with(Acc acc, const TxvTables& tb, const cg_tx_check* d_checks, uint32_t n_tx,
                       cg_tx_verdict* d_verdicts, uint8_t* d_req_status, uint32_t* ws, hipStream_t stream) {
  const unsigned gs = walk_grid(n_tx, kTxvBlock, WALK_CAP(4));
  hipLaunchKernelGGL(k_tx_verdicts_small<Acc>, dim3(gs), dim3(kTxvBlock), 0, stream, acc, tb, d_checks, n_tx,
                     d_verdicts, d_req_status, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // how many transactions are listed is known only on the device: a wave per transaction at most, capped
  const unsigned gw = walk_grid((uint64_t)n_tx * 64u, kTxvBlock, WALK_CAP(2));
  hipLaunchKernelGGL(k_tx_verdicts_wave<Acc>, dim3(gw), dim3(kTxvBlock), 0, stream, acc, tb, d_checks, n_tx,
                     d_verdicts, d_req_status, (const uint32_t*)ws);
  return hipGetLastError();
}

}  // namespace

size_t tx_verdicts_ws_bytes(uint64_t n_tx) { return sizeof(uint32_t) * (4 + (size_t)n_tx); }

hipError_t launch_tx_verdicts(const SigTable& d_sigs, uint64_t n_sigs, const uint8_t* d_status, const cg_key* d_keys,
                              uint32_t n_keys, const TxvSet& d, void* d_ws, hipStream_t stream) {
  const uint32_t n_tx = (uint32_t)d.n_tx;
  hipError_t e = hipSuccess;
  if (d.n_reqs) e = hipMemsetAsync(d.req_status, CG_REQ_HOST, d.n_reqs, stream);
  if (e != hipSuccess || n_tx == 0) return e;
  e = hipMemsetAsync(d_ws, 0, 4 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  TxvTables tb;
  tb.n_sigs = n_sigs;
  tb.status = d_status;
  tb.keys = d_keys;
  tb.n_keys = n_keys;
  tb.key_class = d.key_class;
  tb.reqs = d.reqs;
  tb.n_reqs = d.n_reqs;
  tb.nodes = d.nodes;
  tb.n_nodes = d.n_nodes;
  if (d_sigs.packed())
    return launch_with(Rec12{(const cg_txsig_packed*)d_sigs.p}, tb, d.checks, n_tx, d.verdicts, d.req_status,
                       (uint32_t*)d_ws, stream);
  return launch_with(Rec24{(const cg_txsig*)d_sigs.p}, tb, d.checks, n_tx, d.verdicts, d.req_status, (uint32_t*)d_ws,
                     stream);
}

}  // namespace cg
