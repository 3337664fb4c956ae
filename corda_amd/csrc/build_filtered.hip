// Tear-off building for gfx950: WireTransaction.buildFilteredTransaction / PartialMerkleTree.build
// (include/cordagpu.h, cg_build_filtered / cg_build_partial_trees), the other side of filtered.hip.
//
//   launch_tx_leaves  hash.hip's k_tx_map / k_tx_leaf_* / k_tx_leaves: statuses 1 / 2 / 3 and every
//                     leaf hash, one lane per component ordered by block count (shared with cg_tx_ids)
//   k_bf_count        one lane per transaction: the visible bytes checked (status 6), each visible
//                     component's rank among its transaction's, and the walk of pmt_build.h without
//                     hashing -> rows and slots the transaction needs
//   k_bf_scan         one block per counter: exclusive scan over the transactions, the totals and the
//                     over-capacity flag
//   k_bf_emit         one lane per transaction: the walk with hashing (P - 1 hashConcats, as
//                     k_tx_roots does), node rows and hashes at the scanned offsets, the root, the
//                     cg_filtered_tx row
//   k_bf_leaves       one lane per visible component: its cg_filtered_leaf row and its nonce
//                     SHA256(salt || BE32(i)), one compression
//   k_pt_count / k_pt_emit   the same two walks over a bare leaf list, one lane per tree; inclusion by
//                     value (pmt_mark) once per leaf into a scratch byte
//
// The walk's stack (kPmtLevels x 32 B) is indexed at run time, so it lives in the lane's scratch, as
// k_ftx_verify's does. Every row and slot is checked against its capacity before the store; hashes go
// out as two 16-byte stores of byte-swapped words.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "pmt_build.h"
#include "sha2.h"

namespace cg {

namespace {

__device__ __forceinline__ uint64_t bf_r4(uint64_t x) { return (x + 3) & ~(uint64_t)3; }

// SHA-256 of the 64-byte message l || r (SecureHash.hashConcat); o may be l or r
__device__ __forceinline__ void bf_concat(uint32_t o[8], const uint32_t l[8], const uint32_t r[8]) {
  uint32_t s[8], w[16];
  sha256_init(s);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    w[k] = l[k];
    w[8 + k] = r[k];
  }
  sha256_compress(s, w);
  w[0] = 0x80000000u;
#pragma unroll
  for (int k = 1; k < 15; ++k) w[k] = 0;
  w[15] = 512;
  sha256_compress(s, w);
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = s[k];
}

// What every emit pass writes through: the caller's tables, each store behind its capacity check.
struct BfSink {
  cg_pmt_node* nodes;
  uint64_t node_cap;
  uint8_t* out;
  uint64_t out_cap;
  uint64_t out_base;
  // 8 big-endian words -> the 32 digest bytes of slot `slot`
  __device__ __forceinline__ void put_be(uint64_t slot, const uint32_t v[8]) const {
    if (32 * slot + 32 > out_cap) return;
    uint4* p = (uint4*)(out + 32 * slot);
    p[0] = make_uint4(__builtin_bswap32(v[0]), __builtin_bswap32(v[1]), __builtin_bswap32(v[2]),
                      __builtin_bswap32(v[3]));
    p[1] = make_uint4(__builtin_bswap32(v[4]), __builtin_bswap32(v[5]), __builtin_bswap32(v[6]),
                      __builtin_bswap32(v[7]));
  }
  // 8 words as they are
  __device__ __forceinline__ void put_raw(uint64_t slot, const uint32_t v[8]) const {
    if (32 * slot + 32 > out_cap) return;
    uint4* p = (uint4*)(out + 32 * slot);
    p[0] = make_uint4(v[0], v[1], v[2], v[3]);
    p[1] = make_uint4(v[4], v[5], v[6], v[7]);
  }
  __device__ __forceinline__ void put_node(uint64_t row, uint32_t kind, uint64_t hash_slot) const {
    if (row >= node_cap) return;
    cg_pmt_node nd;
    nd.hash_off = kind == CG_PMT_NODE ? 0 : out_base + 32 * hash_slot;
    nd.kind = kind;
    nd.reserved = 0;
    nodes[row] = nd;
  }
};

// The count pass: the stream's length and how many entries carry a hash.
struct CountOps {
  static constexpr bool kHash = false;
  const uint8_t* vis;  // the tree's own bytes
  uint64_t n_nodes = 0, n_hashes = 0;
  __device__ __forceinline__ bool visible(uint64_t i) const { return vis[i] != 0; }
  __device__ __forceinline__ void leaf(uint64_t, uint32_t*) const {}
  __device__ __forceinline__ void concat(uint32_t*, const uint32_t*, const uint32_t*) const {}
  __device__ __forceinline__ void emit(uint32_t kind, const uint32_t*) {
    ++n_nodes;
    n_hashes += kind != CG_PMT_NODE;
  }
};

// The emit pass over leaf hashes kept as 8 words each at words[8 * i]; kSwap: they are raw digest
// bytes (a bare leaf list), otherwise big-endian words already (the tx-id workspace).
template <bool kSwap>
struct EmitOps {
  static constexpr bool kHash = true;
  const uint8_t* vis;
  const uint32_t* words;
  BfSink sink;
  uint64_t row, slot;  // the next node row and hash slot
  uint32_t n_nodes = 0;
  __device__ __forceinline__ bool visible(uint64_t i) const { return vis[i] != 0; }
  __device__ __forceinline__ void leaf(uint64_t i, uint32_t h[8]) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = kSwap ? __builtin_bswap32(words[8 * i + k]) : words[8 * i + k];
  }
  __device__ __forceinline__ void concat(uint32_t o[8], const uint32_t l[8], const uint32_t r[8]) const {
    bf_concat(o, l, r);
  }
  __device__ __forceinline__ void emit(uint32_t kind, const uint32_t* h) {
    sink.put_node(row, kind, slot);
    if (kind != CG_PMT_NODE) sink.put_be(slot++, h);
    ++row;
    ++n_nodes;
  }
};

__device__ __forceinline__ void bf_ftx_row(cg_filtered_tx* ftxs, uint64_t t, uint64_t node0, uint64_t leaf0,
                                           uint64_t root_off, uint32_t n_nodes, uint32_t n_leaves, uint32_t flags) {
  cg_filtered_tx f;
  f.first_node = node0;
  f.first_leaf = leaf0;
  f.root_off = root_off;
  f.n_nodes = n_nodes;
  f.n_leaves = n_leaves;
  f.flags = flags;
  f.reserved = 0;
  ftxs[t] = f;
}

// counters: cnt[0 .. n) rows of nodes, cnt[stride ..) rows of leaves, cnt[2 stride ..) slots
__device__ __forceinline__ void bf_put_counts(uint64_t* cnt, uint64_t stride, uint64_t t, uint64_t nodes,
                                              uint64_t leaves, uint64_t slots) {
  cnt[t] = nodes;
  cnt[stride + t] = leaves;
  cnt[2 * stride + t] = slots;
}

__global__ void __launch_bounds__(64) k_bf_count(const cg_tx* __restrict__ txs, uint64_t n_tx,
                                                 const cg_component* __restrict__ comps,
                                                 const uint8_t* __restrict__ visible, uint8_t* __restrict__ status,
                                                 uint32_t* __restrict__ rank, uint64_t* __restrict__ cnt,
                                                 uint64_t stride) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tx) return;
  const cg_tx tx = txs[t];
  if (status[t] == 0 && tx.n > kPmtMaxLeaves) status[t] = 1;
  if (status[t] != 0) {  // 1 / 2 / 3: the range may lie outside the tables, nothing of it is read
    bf_put_counts(cnt, stride, t, 0, 0, 1);
    return;
  }
  uint32_t r = 0;
  bool bad = false;
  for (uint32_t i = 0; i < tx.n; ++i) {
    const uint8_t v = visible[tx.first + i];
    bad = bad || v > 1 || (v == 1 && (comps[tx.first + i].flags & 1u));
    rank[tx.first + i] = r;
    r += v == 1;
  }
  if (bad) {
    status[t] = 6;
    bf_put_counts(cnt, stride, t, 0, 0, 1);
    return;
  }
  CountOps ops;
  ops.vis = visible + tx.first;
  uint32_t root[8];
  pmt_walk(tx.n, ops, root);
  bf_put_counts(cnt, stride, t, ops.n_nodes, r, 1 + r + ops.n_hashes);
}

// One block per counter array (blockIdx.x of arrs[stride * blockIdx.x ..)): counts -> exclusive
// offsets in place, a tile of 1024 consecutive counters at a time (coalesced: lane t takes counter
// base + t), each tile scanned by wave shuffles and the 16 wave sums, the tiles chained by a carry.
// partition.h's k_part_scan is the same one-block idea over its (class, block) matrix of 32-bit counts;
// these are three flat 64-bit arrays with totals and capacities behind them.
// With totals: block 0 / 1 / 2 also writes the total rows of nodes / rows of leaves / bytes of slots,
// and sets `over` where it exceeds its capacity (totals zeroed before).
__global__ void __launch_bounds__(1024) k_bf_scan(uint64_t* __restrict__ arrs, uint64_t stride, uint64_t n,
                                                  cg_build_totals* __restrict__ totals, uint64_t node_cap,
                                                  uint64_t leaf_cap, uint64_t out_cap) {
  __shared__ uint64_t wsum[16];
  uint64_t* a = arrs + stride * blockIdx.x;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n; base += 1024) {
    const uint64_t i = base + t;
    const uint64_t x = i < n ? a[i] : 0;
    uint64_t inc = x;  // inclusive within the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t y = (uint64_t)__shfl_up((unsigned long long)inc, d, 64);
      if (lane >= (uint32_t)d) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t before = 0, tile = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) {
      const uint64_t v = wsum[w];
      before += w < wave ? v : 0;
      tile += v;
    }
    if (i < n) a[i] = carry + before + inc - x;
    carry += tile;
    __syncthreads();  // wsum is free for the next tile
  }
  if (totals && t == 0) {
    const uint64_t total = carry;
    bool over;
    if (blockIdx.x == 0) {
      totals->n_nodes = total;
      over = total > node_cap;
    } else if (blockIdx.x == 1) {
      totals->n_leaves = total;
      over = total > leaf_cap;
    } else {
      totals->out_bytes = 32 * total;
      over = 32 * total > out_cap;
    }
    if (over) atomicOr(&totals->over, 1u);
  }
}

__global__ void __launch_bounds__(64) k_bf_emit(const cg_tx* __restrict__ txs, uint64_t n_tx,
                                                const uint8_t* __restrict__ visible,
                                                const uint8_t* __restrict__ status, const uint8_t* __restrict__ leaf_ws,
                                                const uint64_t* __restrict__ off, uint64_t stride, BfSink sink,
                                                cg_filtered_tx* __restrict__ ftxs) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tx) return;
  const uint64_t node0 = off[t], leaf0 = off[stride + t], slot0 = off[2 * stride + t];
  uint32_t root[8];
  if (status[t] != 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) root[k] = 0;
    sink.put_raw(slot0, root);
    bf_ftx_row(ftxs, t, node0, leaf0, sink.out_base + 32 * slot0, 0, 0, CG_FTX_FILTERED);
    return;
  }
  const cg_tx tx = txs[t];
  uint32_t vis_n = 0;  // status 0: every byte is 0 or 1
  for (uint32_t i = 0; i < tx.n; ++i) vis_n += visible[tx.first + i];
  EmitOps<false> ops;
  ops.vis = visible + tx.first;
  ops.words = (const uint32_t*)leaf_ws + 8 * tx.first;
  ops.sink = sink;
  ops.row = node0;
  ops.slot = slot0 + 1 + vis_n;
  pmt_walk(tx.n, ops, root);
  sink.put_be(slot0, root);
  bf_ftx_row(ftxs, t, node0, leaf0, sink.out_base + 32 * slot0, ops.n_nodes, vis_n, CG_FTX_FILTERED);
}

__global__ void __launch_bounds__(256) k_bf_leaves(const cg_tx* __restrict__ txs, const cg_component* __restrict__ comps,
                                                   uint64_t n_comps, const uint32_t* __restrict__ map,
                                                   const uint8_t* __restrict__ visible,
                                                   const uint8_t* __restrict__ status, const uint32_t* __restrict__ rank,
                                                   const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                   const uint64_t* __restrict__ off, uint64_t stride, BfSink sink,
                                                   cg_filtered_leaf* __restrict__ leaves, uint64_t leaf_cap) {
  const uint64_t ci = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= n_comps) return;
  const uint32_t t = map[ci];
  if (t == 0xffffffffu || status[t] != 0 || visible[ci] != 1) return;
  const cg_tx tx = txs[t];
  const cg_component c = comps[ci];
  const uint64_t row = off[stride + t] + rank[ci], slot = off[2 * stride + t] + 1 + rank[ci];
  // nonce = SHA256(salt || BE32(i)): 36 bytes, one block (computeNonce, MerkleTransaction.kt:33)
  const uint64_t lr = bf_r4(arena_len);
  uint32_t s8[8], w[16];
  sha256_init(s8);
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = __builtin_bswap32(cg_ld_bytes4(arena, lr, tx.salt_off + 4 * k));
  w[8] = (uint32_t)(ci - tx.first);
  w[9] = 0x80000000u;
#pragma unroll
  for (int k = 10; k < 15; ++k) w[k] = 0;
  w[15] = 36 * 8;
  sha256_compress(s8, w);
  sink.put_be(slot, s8);
  if (row < leaf_cap) {
    cg_filtered_leaf lf;
    lf.off = c.off;
    lf.nonce_off = sink.out_base + 32 * slot;
    lf.len = c.len;
    lf.flags = 0;
    leaves[row] = lf;
  }
}

// ---- bare PartialMerkleTree.build
__global__ void __launch_bounds__(256) k_pt_widen(const uint32_t* __restrict__ count, uint64_t n,
                                                  uint64_t* __restrict__ wsoff) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) wsoff[j] = count[j];
}

struct WordsAt {
  const uint32_t* p;
  __device__ __forceinline__ void operator()(uint64_t i, uint32_t h[8]) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = p[8 * i + k];
  }
};

__global__ void __launch_bounds__(64) k_pt_count(BuildPtIn in, const uint64_t* __restrict__ wsoff,
                                                 uint8_t* __restrict__ vis, uint8_t* __restrict__ status,
                                                 uint64_t* __restrict__ cnt, uint64_t stride) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= in.n) return;
  const uint64_t f = in.first[j], g = in.inc_first[j], wo = wsoff[j];
  const uint32_t n = in.count[j], m = in.inc_count[j];
  uint32_t st;
  if (n == 0 || n > kPmtMaxLeaves || f > in.n_leaf_hashes || n > in.n_leaf_hashes - f || g > in.n_inc_hashes ||
      m > in.n_inc_hashes - g || wo > in.leaf_total || n > in.leaf_total - wo) {
    st = 1;
  } else {
    const WordsAt leaf_at{(const uint32_t*)in.leaves + 8 * f}, inc_at{(const uint32_t*)in.include + 8 * g};
    st = pmt_mark(n, m, leaf_at, inc_at, vis + wo);
  }
  status[j] = (uint8_t)st;
  if (st != 0) {
    bf_put_counts(cnt, stride, j, 0, 0, 1);
    return;
  }
  CountOps ops;
  ops.vis = vis + wo;
  uint32_t root[8];
  pmt_walk(n, ops, root);
  bf_put_counts(cnt, stride, j, ops.n_nodes, m, 1 + m + ops.n_hashes);
}

__global__ void __launch_bounds__(64) k_pt_emit(BuildPtIn in, const uint64_t* __restrict__ wsoff,
                                                const uint8_t* __restrict__ vis, const uint8_t* __restrict__ status,
                                                const uint64_t* __restrict__ off, uint64_t stride, BfSink sink,
                                                cg_filtered_tx* __restrict__ ftxs, cg_filtered_leaf* __restrict__ leaves,
                                                uint64_t leaf_cap) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= in.n) return;
  const uint64_t node0 = off[j], leaf0 = off[stride + j], slot0 = off[2 * stride + j];
  uint32_t root[8];
  if (status[j] != 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) root[k] = 0;
    sink.put_raw(slot0, root);
    bf_ftx_row(ftxs, j, node0, leaf0, sink.out_base + 32 * slot0, 0, 0, 0);
    return;
  }
  const uint32_t n = in.count[j], m = in.inc_count[j];
  const WordsAt inc_at{(const uint32_t*)in.include + 8 * in.inc_first[j]};
  for (uint32_t q = 0; q < m; ++q) {  // hashesToCheck: copies of the include hashes
    uint32_t x[8];
    inc_at(q, x);
    sink.put_raw(slot0 + 1 + q, x);
    if (leaf0 + q < leaf_cap) {
      cg_filtered_leaf lf;
      lf.off = sink.out_base + 32 * (slot0 + 1 + q);
      lf.nonce_off = 0;
      lf.len = 32;
      lf.flags = CG_FLEAF_HASH;
      leaves[leaf0 + q] = lf;
    }
  }
  EmitOps<true> ops;
  ops.vis = vis + wsoff[j];
  ops.words = (const uint32_t*)in.leaves + 8 * in.first[j];
  ops.sink = sink;
  ops.row = node0;
  ops.slot = slot0 + 1 + m;
  pmt_walk(n, ops, root);
  sink.put_be(slot0, root);
  bf_ftx_row(ftxs, j, node0, leaf0, sink.out_base + 32 * slot0, ops.n_nodes, m, 0);
}

unsigned nblk(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

BfSink sink_of(const BuildOut& o) { return BfSink{o.nodes, o.node_cap, o.out, o.out_cap, o.out_base}; }

}  // namespace

// workspace: [rank 4 x n_comps][counters 3 x 8 x n_tx]
size_t build_ws_bytes(uint64_t n_tx, uint64_t n_comps) {
  return al256(4 * (n_comps ? n_comps : 1)) + 3 * al256(8 * (n_tx ? n_tx : 1));
}

hipError_t launch_build_filtered_count(const BuildTxIn& in, const BuildOut& o, uint8_t* d_leaf_ws, uint8_t* d_ws,
                                       hipStream_t s) {
  hipError_t e = hipMemsetAsync(o.totals, 0, sizeof(cg_build_totals), s);
  if (e != hipSuccess || !in.n_tx) return e;
  e = launch_tx_leaves(in.txs, in.n_tx, in.comps, in.n_comps, in.arena, in.arena_len, o.status, d_leaf_ws, s);
  if (e != hipSuccess) return e;
  uint32_t* rank = (uint32_t*)d_ws;
  uint64_t* cnt = (uint64_t*)(d_ws + al256(4 * (in.n_comps ? in.n_comps : 1)));
  const uint64_t stride = al256(8 * in.n_tx) / 8;
  hipLaunchKernelGGL(k_bf_count, dim3(nblk(in.n_tx, 64)), dim3(64), 0, s, in.txs, in.n_tx, in.comps, in.visible,
                     o.status, rank, cnt, stride);
  hipLaunchKernelGGL(k_bf_scan, dim3(3), dim3(1024), 0, s, cnt, stride, in.n_tx, o.totals, o.node_cap, o.leaf_cap,
                     o.out_cap);
  return hipGetLastError();
}

hipError_t launch_build_filtered_emit(const BuildTxIn& in, const BuildOut& o, uint8_t* d_leaf_ws, uint8_t* d_ws,
                                      hipStream_t s) {
  if (!in.n_tx) return hipSuccess;
  const uint32_t* rank = (const uint32_t*)d_ws;
  const uint64_t* off = (const uint64_t*)(d_ws + al256(4 * (in.n_comps ? in.n_comps : 1)));
  const uint64_t stride = al256(8 * in.n_tx) / 8;
  hipLaunchKernelGGL(k_bf_emit, dim3(nblk(in.n_tx, 64)), dim3(64), 0, s, in.txs, in.n_tx, in.visible,
                     (const uint8_t*)o.status, (const uint8_t*)d_leaf_ws, off, stride, sink_of(o), o.ftxs);
  if (in.n_comps)
    hipLaunchKernelGGL(k_bf_leaves, dim3(nblk(in.n_comps, 256)), dim3(256), 0, s, in.txs, in.comps, in.n_comps,
                       (const uint32_t*)tx_ws_map(d_leaf_ws, in.n_comps), in.visible, (const uint8_t*)o.status, rank,
                       in.arena, in.arena_len, off, stride, sink_of(o), o.leaves, o.leaf_cap);
  return hipGetLastError();
}

// workspace: [dense leaf offsets 8 x n][counters 3 x 8 x n][visible bytes leaf_total]
size_t build_pt_ws_bytes(uint64_t n, uint64_t leaf_total) {
  return 4 * al256(8 * (n ? n : 1)) + al256(leaf_total ? leaf_total : 1);
}

hipError_t launch_build_pt_count(const BuildPtIn& in, const BuildOut& o, uint8_t* d_ws, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(o.totals, 0, sizeof(cg_build_totals), s);
  if (e != hipSuccess || !in.n) return e;
  const uint64_t stride = al256(8 * in.n) / 8;
  uint64_t* wsoff = (uint64_t*)d_ws;
  uint64_t* cnt = wsoff + stride;
  uint8_t* vis = (uint8_t*)(cnt + 3 * stride);
  hipLaunchKernelGGL(k_pt_widen, dim3(nblk(in.n, 256)), dim3(256), 0, s, in.count, in.n, wsoff);
  hipLaunchKernelGGL(k_bf_scan, dim3(1), dim3(1024), 0, s, wsoff, stride, in.n, (cg_build_totals*)nullptr, 0, 0, 0);
  hipLaunchKernelGGL(k_pt_count, dim3(nblk(in.n, 64)), dim3(64), 0, s, in, (const uint64_t*)wsoff, vis, o.status, cnt,
                     stride);
  hipLaunchKernelGGL(k_bf_scan, dim3(3), dim3(1024), 0, s, cnt, stride, in.n, o.totals, o.node_cap, o.leaf_cap,
                     o.out_cap);
  return hipGetLastError();
}

hipError_t launch_build_pt_emit(const BuildPtIn& in, const BuildOut& o, uint8_t* d_ws, hipStream_t s) {
  if (!in.n) return hipSuccess;
  const uint64_t stride = al256(8 * in.n) / 8;
  const uint64_t* wsoff = (const uint64_t*)d_ws;
  const uint64_t* off = wsoff + stride;
  const uint8_t* vis = (const uint8_t*)(off + 3 * stride);
  hipLaunchKernelGGL(k_pt_emit, dim3(nblk(in.n, 64)), dim3(64), 0, s, in, wsoff, vis, (const uint8_t*)o.status, off,
                     stride, sink_of(o), o.ftxs, o.leaves, o.leaf_cap);
  return hipGetLastError();
}

}  // namespace cg
