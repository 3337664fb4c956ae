// The host-side policy of the host-buffer paths (cg_verify_tx_signatures, its packed form and
// cg_verify_batch in cordagpu.cpp), free of HIP so that it runs on the CPU
// (tests/native/txsig_plan_test.cpp, tests/test_txsig_plan.py):
//   - the chunk bounds of a tx-signature call,
//   - the key-use counts that pick each key's table mode (exact, or block-sampled and estimated),
//   - which arena bytes a chunk reads (Extent, scan_chunk) and which of them are not yet on the
//     device (Resident),
//   - the packed form's fix-up of keys and templates that lie outside the caller's arena.
// Nothing here changes a verdict: the counts and the bounds change only speed, the extents only
// which bytes are copied (the kernels bound-check every offset against the arena length).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

#include "../../include/cordagpu.h"

namespace cg {

// fn(t) for every t in [0, m), on the caller's threads (cordagpu.cpp: the context's HostPool, or inline)
using ParFor = std::function<void(uint64_t, const std::function<void(uint64_t)>&)>;

// ---------------------------------------------------------------- chunk bounds
// the host tx-signature forms split a large call into at least this many chunks besides the smaller
// first one (CG_TXSIG_FIRST_DIV): round 6 A/B on the configs[4] shard, 1/6 + 4 / 1/6 + 3 / 1/6 + 2
// chunks = 345.4 / 351.3 / 334.7 M sigs/s over 3 rounds (profiles/r06/h2hchunks)
constexpr uint64_t kTxsigMinChunks = 3;
constexpr uint64_t kTxsigFirstDiv = 6;  // the default first-chunk divisor

// Equal chunks of at most `chunk` items.
inline uint64_t equal_chunk(uint64_t chunk, uint64_t n) {
  if (n <= chunk) return n ? n : 1;
  const uint64_t k = (n + chunk - 1) / chunk;
  return (n + k - 1) / k;
}

// Chunks of `per` items, the last one shorter: {0, per, 2 per, ..., n} (n = 0: no chunk).
inline std::vector<uint64_t> equal_bounds(uint64_t n, uint64_t per) {
  std::vector<uint64_t> bounds;
  for (uint64_t f = 0; f < n; f += per) bounds.push_back(f);
  bounds.push_back(n);
  return bounds;
}

// Chunk k of a host tx-signature call = signatures [bounds[k], bounds[k + 1]).
// chunks: the device chunk, but at least kTxsigMinChunks of them for a large call unless the
// caller set cg_config.chunk_items (the first chunk's copy is the part nothing overlaps; measured on
// the configs[4] shard: 2 chunks 190.7M, 3 200.8M, 4 207.7M, 6 190.0M sigs/s,
// profiles/r03/chunks_v1)
// chunk bounds: with a first-chunk divisor D > 1 (CG_TXSIG_FIRST_DIV, default 6; 0 or 1: equal
// chunks of `per`) the first chunk is 1/D of the call and the rest is split into as many chunks as
// the equal split would make: the first copy is the part nothing hides, and at 1/6 it lands as
// the key-table builds finish (headline A/B, 4 pairs: 257.0 -> 262.9 M sigs/s; 1/5 neutral, 1/7
// and 1/8 -3%: their fronts then share the chip with the builds; profiles/r03/env_fd15*)
// (a call of more than one chunk and fewer than D signatures gets an empty first chunk)
inline std::vector<uint64_t> txsig_bounds(uint64_t n_sigs, uint64_t chunk, bool chunk_set, uint64_t first_div) {
  uint64_t per = equal_chunk(chunk, n_sigs);
  if (!chunk_set && n_sigs >= kTxsigMinChunks * (1ull << 20)) {
    const uint64_t alt = (n_sigs + kTxsigMinChunks - 1) / kTxsigMinChunks;
    if (alt < per) per = alt;
  }
  const uint64_t k0 = (n_sigs + per - 1) / per;
  if (first_div <= 1 || k0 <= 1) return equal_bounds(n_sigs, per);
  const uint64_t f0 = n_sigs / first_div, rest = n_sigs - f0;
  std::vector<uint64_t> bounds = {0, f0};
  for (uint64_t k = 1; k <= k0; ++k) bounds.push_back(f0 + rest * k / k0);
  return bounds;
}

// The largest chunk (sizes the item workspaces).
inline uint64_t largest_chunk(const std::vector<uint64_t>& bounds) {
  uint64_t per = 0;
  for (size_t k = 0; k + 1 < bounds.size(); ++k) per = std::max(per, bounds[k + 1] - bounds[k]);
  return per;
}

// ---------------------------------------------------------------- key-use counts
constexpr uint32_t kTxsigCountSample = 32;  // hot-key calls: 1 in 32 (blocks of 8 records): plan 3.0 -> 1.4-1.8 ms, 235 -> 237 / 247 M (profiles/r03/env_fd12)
constexpr uint32_t kTxsigSampleBlock = 8;

// CG_TXSIG_SAMPLE's value as a sample rate: a power of two, else 0 (no override)
inline uint32_t sample_override(uint32_t x) { return x && (x & (x - 1)) == 0 ? x : 0u; }
// CG_TXSIG_SAMPLE_BLOCK's value as a block length: 1 to 64, else the default
inline uint32_t sample_block(uint32_t x) { return x >= 1 && x <= 64 ? x : kTxsigSampleBlock; }

// 1 in S signatures counted (CG_TXSIG_SAMPLE, a power of two, overrides): S = 32 when keys average
// at least 256 uses (every key far above the 32-use full-table threshold), else 8: at S = 32 an
// unsampled key could not be told from one at the threshold, and a long-tailed key mix (Zipf
// over 1M keys) built full tables for every used key (125 -> 55 M sigs/s, profiles/r03/v12)
// Round 4: 1 (exact counts) instead of 1 in 8 when keys are many. With the quarter mode from 3
// uses, an unsampled key (unused, or used a few times) could not be given a mode: row 0 for all
// of them left ~20% of the 2^20-distinct-key leg's keys (12 uses) on the Horner ladder, quarter
// tables for all of them built tables for the Zipf leg's ~900k unused keys (125 -> 108 M sigs/s)
inline uint32_t sample_rate(uint32_t S_override, uint64_t n_sigs, uint32_t n_keys) {
  return S_override ? S_override : n_sigs >= 256ull * (n_keys ? n_keys : 1) ? kTxsigCountSample : 1u;
}

// The exact pass's per-thread arrays: per host thread a byte counter per key (a wrap to 0 logs
// the key in ovf: +256), kept across calls (cg_ctx owns one) so a call does not page-fault 16
// fresh arrays in
struct CountScratch {
  std::vector<std::vector<uint8_t>> cnt8;
  std::vector<std::vector<uint32_t>> ovf;
};

// counts[k] = the records of tab[0, n_sigs) whose key_idx is k (an index >= n_keys is ignored).
// exact: byte counters per thread (1 MB for 2^20 keys, cache-resident), wraps logged
template <class Rec>
void count_exact(const Rec* tab, uint64_t n_sigs, uint32_t n_keys, uint64_t nt, const ParFor& par, CountScratch& sc,
                 uint32_t* counts) {
  sc.cnt8.resize(nt);
  sc.ovf.resize(nt);
  auto scan8 = [&](uint64_t t) {
    std::vector<uint8_t>& c8 = sc.cnt8[t];
    if (c8.size() < n_keys) c8.resize(n_keys);
    if (n_keys) memset(c8.data(), 0, n_keys);  // (no keys: data() may be null)
    std::vector<uint32_t>& of = sc.ovf[t];
    of.clear();
    uint8_t* cc = c8.data();
    for (uint64_t i = n_sigs * t / nt; i < n_sigs * (t + 1) / nt; ++i) {
      const uint32_t k = tab[i].key_idx;
      if (k < n_keys && ++cc[k] == 0) of.push_back(k);
    }
  };
  par(nt, scan8);
  auto sum = [&](uint64_t t) {
    for (uint64_t k = n_keys * t / nt; k < n_keys * (t + 1) / nt; ++k) {
      uint32_t v = 0;
      for (uint64_t u = 0; u < nt; ++u) v += sc.cnt8[u][k];
      counts[k] = v;
    }
  };
  par(nt, sum);
  for (uint64_t t = 0; t < nt; ++t)
    for (uint32_t k : sc.ovf[t]) counts[k] += 256u;
}

// counts[k] += the sampled records whose key_idx is k: B consecutive records of every S B.
// CG_TXSIG_SAMPLE_BLOCK (A/B): consecutive records per sample. 8 reads an eighth of the table's
// cache lines instead of all of them (every 8th 24-B record): the pass went 5.3 -> 2.8 ms on the
// configs[4] shard, 218 -> 238 M sigs/s (profiles/r03/env_ec3); a key the block sampling
// under-counts only lands in a smaller table mode, whose ladders run on the side streams
template <class Rec>
void count_sampled(const Rec* tab, uint64_t n_sigs, uint32_t n_keys, uint64_t nt, const ParFor& par, uint32_t S,
                   uint32_t B, uint32_t* counts) {
  const uint64_t Bs = B;
  const uint64_t ng = (n_sigs + (uint64_t)S * Bs - 1) / ((uint64_t)S * Bs);
  std::vector<std::vector<uint32_t>> pc(nt > 1 ? nt : 0, std::vector<uint32_t>(n_keys ? n_keys : 1, 0u));
  auto scan = [&](uint64_t t) {
    uint32_t* cnt = nt > 1 ? pc[t].data() : counts;
    for (uint64_t g = ng * t / nt; g < ng * (t + 1) / nt; ++g) {
      // B consecutive records per group of S B, the block at a hashed position (no aliasing with
      // a layout that cycles through the keys); B > 1 reads fewer cache lines per sample
      const uint64_t i0 = (g * S + (((uint32_t)g * 0x9E3779B1u) >> 24) % S) * Bs;
      for (uint64_t i = i0; i < i0 + Bs && i < n_sigs; ++i) {
        const uint32_t k = tab[i].key_idx;
        if (k < n_keys) ++cnt[k];
      }
    }
  };
  if (nt == 1) {
    scan(0);
  } else {
    par(nt, scan);
    par(nt, [&](uint64_t t) {  // sum the per-thread counts, key ranges in parallel
      for (uint64_t k = n_keys * t / nt; k < n_keys * (t + 1) / nt; ++k)
        for (uint64_t u = 0; u < nt; ++u) counts[k] += pc[u][k];
    });
  }
}

// c sampled uses -> S (c + 3 sqrt(c) + 1): about three standard deviations above the unbiased
// S c, so a key whose true count clears a mode threshold is not sampled below it (two were not
// enough at 1 in 32: a few keys got full tables and a 0.18 ms full-table ladder per chunk,
// profiles/r03/v14; on the
// configs[4] shard the plain estimate put 2 of 4096 Ed25519 keys, true minimum 1 634 uses, under
// the 1 536 wide threshold: full tables and a 170 us pf ladder per chunk, profiles/r03/v5); an
// unsampled key counts min(S, 8): its row-0 table, so every key a signature may use has one
// The raised estimate only where it decides a wide table (wmin: the key's wide threshold): below
// the wide threshold the plain S c decides row 0 against full tables (a wrong full table costs
// ~230 ns, a wrong row 0 ~7 ns per use; at 1 in 8 the raised estimate put every sampled key of the
// 2^20-distinct-key leg, ~12 uses each, in full mode: 22-row builds for ~1M keys, profiles/r04/kd)
// floor_hot: the least a sampled key counts (hot_floor below).
inline uint32_t estimate_uses(uint64_t c, uint32_t S, uint64_t wmin, uint64_t floor_hot) {
  const uint64_t up = (uint64_t)S * (c + 3 * (uint64_t)std::ceil(std::sqrt((double)c)) + 1);
  uint64_t e = c ? (up >= wmin ? up : (uint64_t)S * c)
                 : (S < 8u ? S : 8u);  // unsampled: row-0 tables (below the 32-use threshold)
  if (c && e < floor_hot) e = floor_hot;
  return e > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)e;
}

// In a hot call (1 in 32: keys average 256+ uses) every sampled key is counted up to the wide
// threshold: a few keys left in full-table mode cost a serial full-table launch per chunk (0.18
// ms, ~1.4% of the headline, profiles/r03/ab_der), a wide table costs about 230 items' work.
inline uint64_t hot_floor(uint32_t S, uint32_t min_ed, uint32_t min_ec) {
  return S >= kTxsigCountSample ? (uint64_t)std::max(min_ed, min_ec) : 0u;
}

// Key-use counts for the table modes from a 1-in-S sample of the signature table (the budget's
// host threads; the modes change only speed, never a verdict), every key at least 1 so that each
// key an unsampled signature may use has its row-0 table. S = 1: exact counts, no estimate.
// counts: n_keys entries (at least one), zero on entry. min_ed / min_ec: the wide-table thresholds
// of the two key families (keys[k].scheme picks one).
template <class Rec>
void key_use_counts(const Rec* tab, uint64_t n_sigs, const cg_key* keys, uint32_t n_keys, uint64_t nt,
                    const ParFor& par, uint32_t S, uint32_t B, uint32_t min_ed, uint32_t min_ec, CountScratch& sc,
                    uint32_t* counts) {
  if (S == 1) return count_exact(tab, n_sigs, n_keys, nt, par, sc, counts);
  count_sampled(tab, n_sigs, n_keys, nt, par, S, B, counts);
  const uint64_t floor_hot = hot_floor(S, min_ed, min_ec);
  for (uint32_t k = 0; k < n_keys; ++k) {
    const uint64_t wmin = keys[k].scheme == CG_EDDSA_ED25519_SHA512 ? min_ed : min_ec;
    counts[k] = estimate_uses(counts[k], S, wmin, floor_hot);
  }
}

// ---------------------------------------------------------------- which arena bytes a chunk needs
struct Extent {
  uint64_t lo = UINT64_MAX, hi = 0;
  void add(uint64_t off, uint64_t len, uint64_t arena_len) {
    if (off > arena_len) return;  // outside the arena: the kernels never read it (CG_NOT_RUN)
    const uint64_t e = len > arena_len - off ? arena_len : off + len;
    if (off < lo) lo = off;
    if (e > hi) hi = e;
  }
  void merge(const Extent& o) {
    if (o.lo < lo) lo = o.lo;
    if (o.hi > hi) hi = o.hi;
  }
  bool empty() const { return lo >= hi; }
};

// The byte ranges already on the device (`have`: sorted disjoint intervals).
struct Resident {
  std::vector<std::pair<uint64_t, uint64_t>> have;
  // The parts of [e.lo, e.hi) not yet resident, in order; e is resident afterwards.
  std::vector<std::pair<uint64_t, uint64_t>> missing(const Extent& e) {
    std::vector<std::pair<uint64_t, uint64_t>> gaps;
    if (e.empty()) return gaps;
    uint64_t cur = e.lo;
    for (const auto& h : have) {
      if (h.second <= cur) continue;
      if (h.first >= e.hi) break;
      if (h.first > cur) gaps.push_back({cur, h.first});
      cur = h.second > cur ? h.second : cur;
      if (cur >= e.hi) break;
    }
    if (cur < e.hi) gaps.push_back({cur, e.hi});
    have.push_back({e.lo, e.hi});
    std::sort(have.begin(), have.end());
    std::vector<std::pair<uint64_t, uint64_t>> m;
    for (const auto& h : have) {
      if (!m.empty() && h.first <= m.back().second) m.back().second = std::max(m.back().second, h.second);
      else m.push_back(h);
    }
    have.swap(m);
    return gaps;
  }
};

// What signatures [f, e) of a table read: the signature bytes (24-byte records: their arena
// extent; 12-byte records: `span`, the chunk's stream bytes, the sum of round_up(sig_len, 4), whose
// extent follows once the chunk's stream offset is known) and the 32-byte ids of the transactions
// below n_ids, as an extent of the id table.
struct ChunkScan {
  Extent sig, ids;
  uint64_t span = 0;
};
inline void scan_record(const cg_txsig& r, uint64_t arena_len, ChunkScan& x) { x.sig.add(r.sig_off, r.sig_len, arena_len); }
inline void scan_record(const cg_txsig_packed& r, uint64_t, ChunkScan& x) {
  x.span += ((uint64_t)r.sig_len + 3u) & ~(uint64_t)3;
}
// exact: a threaded scan of the slice (one part below 2^16 records, else nt)
template <class Rec>
ChunkScan scan_chunk(const Rec* tab, uint64_t f, uint64_t e, uint64_t n_ids, uint64_t arena_len, uint64_t nt,
                     const ParFor& par) {
  const uint64_t m = (e - f) < (1u << 16) ? 1 : nt;
  std::vector<ChunkScan> part(m);
  auto scan = [&](uint64_t t) {
    ChunkScan x;  // thread-local until the end (the vector slots share cache lines)
    const uint64_t i0 = f + (e - f) * t / m, i1 = f + (e - f) * (t + 1) / m;
    for (uint64_t i = i0; i < i1; ++i) {
      scan_record(tab[i], arena_len, x);
      if (tab[i].tx_idx < n_ids) x.ids.add(32ull * tab[i].tx_idx, 32, 32ull * n_ids);
    }
    part[t] = x;
  };
  par(m, scan);
  ChunkScan all;
  for (const ChunkScan& p : part) {
    all.sig.merge(p.sig);
    all.ids.merge(p.ids);
    all.span += p.span;
  }
  return all;
}

// The header of a tx-signature call: the key bytes and the template bytes.
inline Extent txsig_head_extent(const cg_key* keys, uint32_t n_keys, const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                                uint64_t arena_len) {
  Extent head;
  for (uint32_t k = 0; k < n_keys; ++k) head.add(keys[k].off, keys[k].len, arena_len);
  for (uint32_t k = 0; k < n_tmpls; ++k) {
    head.add(tmpls[k].prefix_off, tmpls[k].prefix_len, arena_len);
    head.add(tmpls[k].suffix_off, tmpls[k].suffix_len, arena_len);
  }
  return head;
}

// ---------------------------------------------------------------- the packed form's fix-up
// The 12-byte form's signatures follow the caller's arena on the device, so a key or template that
// lies outside the caller's [0, caller_len) is moved out of the extended arena too (off =
// UINT64_MAX: it never reads a signature). keys_fix / tmpls_fix: the corrected copy of a table,
// empty when every entry of it is in range.
inline void txsig_packed_fixup(const cg_key* keys, uint32_t n_keys, const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                               uint64_t caller_len, std::vector<cg_key>& keys_fix,
                               std::vector<cg_signable_tmpl>& tmpls_fix) {
  auto out = [&](uint64_t off, uint64_t len) { return off > caller_len || len > caller_len - off; };
  for (uint32_t k = 0; k < n_keys; ++k)
    if (out(keys[k].off, keys[k].len)) {
      if (keys_fix.empty()) keys_fix.assign(keys, keys + n_keys);
      keys_fix[k].off = UINT64_MAX;
    }
  for (uint32_t k = 0; k < n_tmpls; ++k)
    if (out(tmpls[k].prefix_off, tmpls[k].prefix_len) || out(tmpls[k].suffix_off, tmpls[k].suffix_len)) {
      if (tmpls_fix.empty()) tmpls_fix.assign(tmpls, tmpls + n_tmpls);
      tmpls_fix[k].prefix_off = UINT64_MAX;
    }
}

}  // namespace cg
