// Tear-off building (include/cordagpu.h, cg_build_filtered / cg_build_partial_trees): the lane logic of
// build_filtered.hip, free of HIP so that the CPU compiles exactly what the GPU runs
// (tests/native/pmt_build_test.cpp, tests/test_pmt_build.py).
//
// pmt_walk is PartialMerkleTree.build's buildPartialTree (PartialMerkleTree.kt:98-123) over the padded
// leaf list of MerkleTree.getMerkleTree (MerkleTree.kt:27-66) as one left-to-right pass, without the
// full tree and without recursion. At leaf position i it takes the largest aligned block [i, i + 2^k)
// (2^k | i, i + 2^k <= P) that holds no included leaf, reduces it to its Merkle hash and emits one
// CG_PMT_LEAF; if position i itself is included it emits CG_PMT_INCLUDED. Pending subtrees wait in a
// stack indexed by level (a binary counter: after [0, i) the occupied levels are the set bits of i);
// a new entry merges with the entry of its own level (hashConcat, one CG_PMT_NODE) for as long as
// there is one. The blocks are maximal, so every such merge has an included leaf below it: NODE is
// always right and the stream comes out in post-order. A hidden block is reduced by the same counter
// on the levels below k, which the entries outside it never use (2^k | i), so one stack of kPmtLevels
// entries serves both. Every node of the full tree is hashed once: P - 1 hashConcats.
//
// pmt_mark is the by-value inclusion rule of PartialMerkleTree.build (:66-76) for a bare leaf list.
//
// Ops of pmt_walk:
//   static constexpr bool kHash            false: the count pass (no loads, no hashes, same stream)
//   bool visible(uint64_t i)               i < n
//   void leaf(uint64_t i, uint32_t h[8])   i < n: the leaf hash as 8 big-endian words
//   void concat(uint32_t o[8], const uint32_t l[8], const uint32_t r[8])   SHA256(l || r)
//   void emit(uint32_t kind, const uint32_t* h)   one stream entry (h: LEAF / INCLUDED only)
#pragma once
#include <stdint.h>

#include "../../include/cordagpu.h"

#if defined(__HIPCC__)
#define CG_PMT_HD __host__ __device__ __forceinline__
#else
#define CG_PMT_HD inline
#endif

namespace cg {

constexpr uint32_t kPmtLevels = 32;          // stack entries: one per level below the root
constexpr uint32_t kPmtMaxLeaves = 1u << 30; // leaves per tree: 2P - 1 nodes fit the 32-bit row counts
constexpr uint64_t kPmtNone = ~0ull;

// The first included position at or after i, or kPmtNone.
template <class Ops>
CG_PMT_HD uint64_t pmt_next_visible(Ops& ops, uint64_t i, uint64_t n) {
  while (i < n && !ops.visible(i)) ++i;
  return i < n ? i : kPmtNone;
}

// The walk over n >= 1 leaves (n <= kPmtMaxLeaves); root: the full tree's root hash (kHash only).
// One loop over the P positions with one leaf site and one hashConcat site: position p pushes its leaf
// and merges as often as p has trailing one bits, whatever is visible, so the lanes of a wave that walk
// trees of one size stay converged through every SHA-256. `hidden` is true inside a block that holds no
// included leaf: its merges (all below level k) emit nothing, and its last position, where the block's
// own hash is complete at level k, emits the block's one LEAF.
template <class Ops>
CG_PMT_HD void pmt_walk(uint64_t n, Ops& ops, uint32_t root[8]) {
  uint64_t P = 1;
  uint32_t top = 0;
  while (P < n) {
    P <<= 1;
    ++top;
  }
  uint32_t stk[kPmtLevels][8];
  uint32_t mask = 0;  // occupied levels
  uint32_t cur[8];
  for (int w = 0; w < 8; ++w) cur[w] = 0;
  uint64_t nv = pmt_next_visible(ops, 0, n);
  uint64_t next = 0;    // the position where the next block (or included leaf) starts
  uint32_t k = 0;       // the current hidden block is [next - 2^k, next)
  bool hidden = false;
  for (uint64_t p = 0; p < P; ++p) {
    if (p == next) {
      if (nv < p) nv = pmt_next_visible(ops, p, n);
      hidden = nv != p;
      k = 0;
      if (hidden) {  // the largest k: 2^k | p, p + 2^k <= min(P, nv)
        const uint64_t lim = nv < P ? nv : P;
        k = top;
        if (p) {
          k = 0;
          while (!((p >> k) & 1)) ++k;
        }
        while (p + (1ull << k) > lim) --k;
      }
      next = p + (1ull << k);
    }
    if (Ops::kHash) {
      if (p < n) {
        ops.leaf(p, cur);
      } else {
        for (int w = 0; w < 8; ++w) cur[w] = 0;  // zeroHash padding (MerkleTree.kt:35-43)
      }
    }
    if (!hidden) ops.emit(CG_PMT_INCLUDED, cur);
    uint32_t lv = 0;
    for (;;) {
      if (hidden && lv == k && p + 1 == next) {  // the block is complete
        ops.emit(CG_PMT_LEAF, cur);
        hidden = false;
      }
      if (lv >= kPmtLevels || !(mask & (1u << lv))) break;
      if (Ops::kHash) ops.concat(cur, stk[lv], cur);
      mask &= ~(1u << lv);
      ++lv;
      if (!hidden) ops.emit(CG_PMT_NODE, nullptr);
    }
    if (p + 1 < P) {
      if (Ops::kHash)
        for (int w = 0; w < 8; ++w) stk[lv][w] = cur[w];
      mask |= 1u << lv;
    }
  }
  for (int w = 0; w < 8; ++w) root[w] = cur[w];
}

// Inclusion by value for a bare leaf list: vis[i] = leaf i's hash is in the include list. Returns the
// status of cg_build_partial_trees: 1 no leaves; 4 zeroHash in the include list
// (IllegalArgumentException, PartialMerkleTree.kt:67); 5 the number of included leaves differs from
// the include list's length (MerkleTreeException, :74: a duplicate in the list, a hash the tree lacks,
// or an included hash that also sits at another leaf); 0 otherwise.
// leaf_at(i, h) / inc_at(q, h): the hash as 8 words (any byte order, the same for both).
template <class LeafAt, class IncAt>
CG_PMT_HD uint32_t pmt_mark(uint64_t n, uint32_t m, const LeafAt& leaf_at, const IncAt& inc_at, uint8_t* vis) {
  if (n == 0) return 1;
  for (uint32_t q = 0; q < m; ++q) {
    uint32_t x[8], d = 0;
    inc_at(q, x);
    for (int w = 0; w < 8; ++w) d |= x[w];
    if (d == 0) return 4;
  }
  uint64_t used = 0;
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t h[8];
    leaf_at(i, h);
    bool in = false;
    for (uint32_t q = 0; q < m && !in; ++q) {
      uint32_t x[8], d = 0;
      inc_at(q, x);
      for (int w = 0; w < 8; ++w) d |= x[w] ^ h[w];
      in = d == 0;
    }
    vis[i] = in ? 1 : 0;
    used += in;
  }
  return used == m ? 0 : 5;
}

}  // namespace cg
