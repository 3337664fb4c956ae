// Batch signature verification for gfx950: dispatch over the per-scheme kernels.
//
// Pipeline per batch (all on the caller's stream, no host round trip):
//   key prep      verify_ed.hip k_ed_keyprep_rows/_tab, verify_ec.hip k_ec_keyprep_rows/_tab
//   items         k_misc_status (unsupported scheme / bad key index); the plan (plan_sort.hip:
//                 items sorted by (scheme, key), one dense range per scheme); then the Ed25519 stages (k_ed_verify, k_ed_finish) and per
//                 curve the ECDSA stages (k_ec_prep, k_ec_inv, k_ec_ladder) over their ranges.
//                 Each stage writes the final status byte of its items.
// Replaces, per item, the JCA call at core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:553-559
// behind Crypto.doVerify (Crypto.kt:474-484).
#include "keyws.h"

namespace cg {

__global__ void k_misc_status(const cg_item* __restrict__ items, uint64_t n_items, const cg_key* __restrict__ keys,
                              uint32_t n_keys, uint8_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const uint32_t ki = items[i].key_idx;
  if (ki >= n_keys) {
    status[i] = CG_NOT_RUN;
    return;
  }
  const uint8_t s = keys[ki].scheme;
  if (s != CG_EDDSA_ED25519_SHA512 && s != CG_ECDSA_SECP256R1_SHA256 && s != CG_ECDSA_SECP256K1_SHA256)
    status[i] = CG_UNSUPPORTED;
  else if (s == CG_EDDSA_ED25519_SHA512)
    status[i] = CG_NOT_RUN;  // until a verdict lands (k_ed_hash writes only its early verdicts: verify_ed.hip)
}

// Per-key use counts, sampled: one item in KEY_USES_SAMPLE adds KEY_USES_SAMPLE (no-return
// atomics, a quarter of the traffic of counting all), every item marks its key as used (plain
// stores: the exact "has items" bit row 0 depends on). Out-of-range key indices are
// k_misc_status's (CG_NOT_RUN) and count nowhere.
__global__ void __launch_bounds__(256) k_key_init(uint32_t n_keys, uint32_t all, uint32_t* __restrict__ uses,
                                                  uint8_t* __restrict__ seen, uint32_t* __restrict__ full_count,
                                                  uint32_t* __restrict__ wide_idx, uint32_t* __restrict__ wide_count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < PLAN_CLASSES) full_count[i] = full_count[ROW0_COUNT_AT + i] = full_count[QUART_COUNT_AT + i] = 0;
  if (i == 0) full_count[SKIP_MISMATCH_AT] = 0;
  if (i < PLAN_CLASSES + 2) wide_count[i] = 0;
  if (i >= n_keys) return;
  uses[i] = all ? KEY_USES_ALL : 0u;
  seen[i] = all ? 1 : 0;
  wide_idx[i] = KEY_NOT_WIDE;
}

__global__ void __launch_bounds__(256) k_key_uses(const cg_item* __restrict__ items, uint64_t n_items,
                                                  uint32_t n_keys, uint32_t* __restrict__ uses,
                                                  uint8_t* __restrict__ seen) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const uint32_t k = items[i].key_idx;
  if (k >= n_keys) return;
  seen[k] = 1;
  // sample by a multiplicative hash of the index, not i % 4: a batch whose items cycle through
  // the keys with a stride (item j -> key j % n) would otherwise alias whole keys out
  if (((uint32_t)i * 0x9E3779B1u) >> 30 == 0) atomicAdd(&uses[k], KEY_USES_SAMPLE);
}

// The same, from a cg_txsig table (cg_verify_tx_signatures_device: the key tables are sized before
// any verify item exists, so the per-chunk item builds and splices can follow them).
template <class Sig>
__global__ void __launch_bounds__(256) k_key_uses_txsig(const Sig* __restrict__ sigs, uint64_t n,
                                                        uint32_t n_keys, uint32_t* __restrict__ uses,
                                                        uint8_t* __restrict__ seen) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = sigs[i].key_idx;
  if (k >= n_keys) return;
  seen[k] = 1;
  if (((uint32_t)i * 0x9E3779B1u) >> 30 == 0) atomicAdd(&uses[k], KEY_USES_SAMPLE);
}

// Exact counts made by the host (cg_verify_tx_signatures counts while it scans the signature
// table for the copy extents, so no signature table has to be resident before the key tables).
__global__ void __launch_bounds__(256) k_key_counts(const uint32_t* __restrict__ counts, uint32_t n_keys,
                                                    uint32_t* __restrict__ uses, uint8_t* __restrict__ seen) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_keys) return;
  uses[i] = counts[i];
  seen[i] = counts[i] != 0;
}

// Append the lanes with c == k to list k (one atomic per wave and class).
__device__ __forceinline__ void list_append(int c, uint32_t i, uint32_t n_keys, uint32_t* __restrict__ list,
                                            uint32_t* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int k = 0; k < PLAN_CLASSES; ++k) {
    const uint64_t m = __ballot(c == k);
    if (m == 0) continue;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(&count[k], (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    if (c == k) list[(size_t)k * n_keys + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
  }
}

// The wide-table cache (key_cache.h) at the start of a call, one block per pool: every slot whose
// tables are not known to be complete is empty again, nothing is live, the counters are zero, and
// the index holds the valid owners (at most KEY_WIDE_MAX a pool: one block, two barriers).
#define KC_BLOCK 1024
__global__ void __launch_bounds__(KC_BLOCK) k_kc_begin(KeyCache kc) {
  const int pool = blockIdx.x;
  KcOwner* owners = kc.owners[pool];
  uint32_t* index = kc.index[pool];
  if (threadIdx.x < KC_CTRS) kc.ctr[pool * KC_CTRS + threadIdx.x] = 0;
  for (uint32_t b = threadIdx.x; b < kc.size; b += KC_BLOCK) index[b] = 0;
  for (uint32_t s = threadIdx.x; s < kc.slots; s += KC_BLOCK) kc_begin_slot(owners, kc.live[pool], s, kc.dirty);
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kc.slots; s += KC_BLOCK)
    if (owners[s].state == KC_VALID) kc_index_insert(index, kc.size, kc.bits, owners, s);
}

__device__ __forceinline__ void kc_load_key(KcKey& k, const cg_key& key, const uint8_t* arena, uint64_t arena_len) {
  kc_key_load(k, key.scheme, key.fmt, key.len, arena, arena_len, key.off);
}

// Table mode per key: wide tables for keys with >= min_ed / min_ec items while the family's
// wide pool has slots (one atomic per wide key: they are few), else full tables from
// ED_DIRECT_MAX_USES items, quarter tables from KEY_QUARTER_MIN_USES, else row 0; the keys of each
// mode compacted per scheme class (row0 lists every used key without wide tables). One wave a block.
// With the wide-table cache (kc.on()), the same keys are wide, but a key whose tables the context
// still holds takes their slot (wide_idx) and joins no build list; the others are listed in `wide`
// without a slot, which k_kc_claim gives them.
__global__ void __launch_bounds__(64) k_key_classify(const cg_key* __restrict__ keys, uint32_t n_keys,
                                                     uint32_t* __restrict__ uses, const uint8_t* __restrict__ seen,
                                                     uint32_t* __restrict__ full, uint32_t* __restrict__ full_count,
                                                     uint32_t* __restrict__ wide_idx, uint32_t* __restrict__ wide,
                                                     uint32_t* __restrict__ wide_count, uint32_t* __restrict__ row0,
                                                     uint32_t* __restrict__ quart, uint32_t cap_ed, uint32_t cap_ec,
                                                     uint32_t min_ed, uint32_t min_ec, uint32_t skip_mask,
                                                     const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                     KeyCache kc) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  int c = -1, cw = -1, c0 = -1, cq = -1;  // full list, wide list, row-0 list, quarter list
  bool is_wide = false;
  uint32_t u = 0;
  if (i < n_keys) {  // the estimate, made exact where it matters: a used key counts >= 1
    u = uses[i];
    if (!seen[i]) u = 0;
    else if (u == 0) u = 1;
    uses[i] = u;
  }
  if (i < n_keys && u >= ED_DIRECT_MAX_USES) {
    const uint8_t s = keys[i].scheme;
    c = s == CG_EDDSA_ED25519_SHA512 ? PLAN_ED
      : s == CG_ECDSA_SECP256R1_SHA256 ? PLAN_R1
      : s == CG_ECDSA_SECP256K1_SHA256 ? PLAN_K1
                                       : -1;
    // KEY_USES_ALL (cg_prepare_keys_device: uses unknown) never gets wide tables
    const int pool = c == PLAN_ED ? 0 : 1;
    if (c >= 0 && u >= (pool == 0 ? min_ed : min_ec) && u != KEY_USES_ALL) {
      const uint32_t cap = pool == 0 ? cap_ed : cap_ec;
      if (cap) {
        const uint32_t slot = atomicAdd(&wide_count[PLAN_CLASSES + pool], 1u);
        if (slot < cap) {
          is_wide = true;
          if (!kc.on()) {
            wide_idx[i] = slot;
            cw = c;
          } else {
            KcKey k;
            kc_load_key(k, keys[i], arena, arena_len);
            const uint32_t hit = kc_probe(kc.index[pool], kc.size, kc.bits, kc.owners[pool], k);
            if (hit != KC_NONE) {
              wide_idx[i] = hit;
              kc.live[pool][hit] = 1;
              atomicAdd(&kc.ctr[pool * KC_CTRS + KC_CTR_HITS], 1u);
            } else {
              cw = c;  // k_kc_claim finds it a slot
            }
          }
          c = -1;
        } else if (kc.on()) {
          atomicAdd(&kc.ctr[pool * KC_CTRS + KC_CTR_FELL_BACK], 1u);
        }
      }
    }
  }
  if (i < n_keys && u >= 1 && !is_wide) {  // every used key without wide tables gets its row 0
    const uint8_t s = keys[i].scheme;
    c0 = s == CG_EDDSA_ED25519_SHA512 ? PLAN_ED
       : s == CG_ECDSA_SECP256R1_SHA256 ? PLAN_R1
       : s == CG_ECDSA_SECP256K1_SHA256 ? PLAN_K1
                                        : -1;
    if (u >= KEY_QUARTER_MIN_USES && u < ED_DIRECT_MAX_USES) cq = c0;  // and its quarter rows 1..3
  }
  if (skip_mask && (c >= 0 || c0 >= 0)) {  // a mode whose builds / ladders the host skipped
    const int cls = c >= 0 ? c : c0;
    const uint32_t f = cls == PLAN_R1 ? 0u : cls == PLAN_K1 ? 1u : 2u;
    if ((skip_mask >> f) & 1u) atomicOr(&full_count[SKIP_MISMATCH_AT], 1u << f);
  }
  list_append(c, i, n_keys, full, full_count);
  list_append(cw, i, n_keys, wide, wide_count);
  list_append(c0, i, n_keys, row0, full_count + ROW0_COUNT_AT);
  list_append(cq, i, n_keys, quart, full_count + QUART_COUNT_AT);
}

// The cache's claim pass, one block per pool, after k_key_classify: the slots no key of this call
// hit are listed (empty ones first), and the r-th key of the pool's build lists (Ed25519; secp256r1
// then secp256k1) takes the r-th of them, its owner pending until the builds commit. The call's
// wide keys number at most its cap, the slots at least that, so every listed key finds one; were
// the list ever short, the keys at its tail take full tables, as a key over the cap does.
__global__ void __launch_bounds__(KC_BLOCK) k_kc_claim(const cg_key* __restrict__ keys, uint32_t n_keys,
                                                       const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                       uint32_t* __restrict__ wide_idx, uint32_t* __restrict__ wide,
                                                       uint32_t* __restrict__ wide_count, uint32_t* __restrict__ full,
                                                       uint32_t* __restrict__ full_count, uint32_t* __restrict__ row0,
                                                       uint32_t skip_mask, KeyCache kc) {
  __shared__ uint32_t sc[2][KC_BLOCK];
  __shared__ uint32_t tot[2];
  const int pool = blockIdx.x;
  const uint32_t t = threadIdx.x;
  KcOwner* owners = kc.owners[pool];
  uint32_t cnt[2];
  kc_free_count(owners, kc.live[pool], kc.slots, t, KC_BLOCK, cnt);
  sc[0][t] = cnt[0];
  sc[1][t] = cnt[1];
  __syncthreads();
  for (uint32_t d = 1; d < KC_BLOCK; d <<= 1) {  // inclusive scans of both counts
    const uint32_t a = t >= d ? sc[0][t - d] : 0u, b = t >= d ? sc[1][t - d] : 0u;
    __syncthreads();
    sc[0][t] += a;
    sc[1][t] += b;
    __syncthreads();
  }
  if (t == KC_BLOCK - 1) {
    tot[0] = sc[0][t];
    tot[1] = sc[1][t];
  }
  __syncthreads();
  kc_free_fill(owners, kc.live[pool], kc.slots, t, KC_BLOCK, sc[0][t] - cnt[0], tot[0] + sc[1][t] - cnt[1],
               kc.freel[pool]);
  const uint32_t nfree = tot[0] + tot[1];
  const int c_lo = pool == 0 ? PLAN_ED : PLAN_R1, c_hi = pool == 0 ? PLAN_ED : PLAN_K1;
  static_assert(PLAN_R1 + 1 == PLAN_K1, "the ECDSA pool's classes are adjacent");
  uint32_t n_c[2] = {0, 0};
  for (int c = c_lo; c <= c_hi; ++c) n_c[c - c_lo] = wide_count[c];
  __syncthreads();  // the free list is written, the list lengths are read
  uint32_t base = 0;
  for (int c = c_lo; c <= c_hi; ++c) {
    const uint32_t n = n_c[c - c_lo];
    for (uint32_t l = t; l < n; l += KC_BLOCK) {
      const uint32_t i = wide[(size_t)c * n_keys + l];
      KcKey k;
      kc_load_key(k, keys[i], arena, arena_len);
      bool evicted;
      const uint32_t s = kc_claim(owners, kc.freel[pool], nfree, base + l, k, &evicted);
      if (s != KC_NONE) {
        wide_idx[i] = s;
        if (evicted) atomicAdd(&kc.ctr[pool * KC_CTRS + KC_CTR_EVICTED], 1u);
      } else {  // full tables and a row 0, like a key over the cap (k_key_classify)
        full[(size_t)c * n_keys + atomicAdd(&full_count[c], 1u)] = i;
        row0[(size_t)c * n_keys + atomicAdd(&full_count[ROW0_COUNT_AT + c], 1u)] = i;
        const uint32_t f = c == PLAN_R1 ? 0u : c == PLAN_K1 ? 1u : 2u;
        if ((skip_mask >> f) & 1u) atomicOr(&full_count[SKIP_MISMATCH_AT], 1u << f);
        atomicAdd(&kc.ctr[pool * KC_CTRS + KC_CTR_FELL_BACK], 1u);
      }
    }
    if (t == 0) wide_count[c] = base >= nfree ? 0u : (n < nfree - base ? n : nfree - base);  // the claimed head
    base += n;
  }
}

// After class c's wide row builds, on their stream: the slots this call claimed hold complete
// tables (valid) unless their key did not decode (empty again: such a key is never cached).
__global__ void __launch_bounds__(256) k_kc_commit(int c, uint32_t n_keys, const EdKeyHdr* __restrict__ hdr,
                                                   const uint32_t* __restrict__ wide,
                                                   const uint32_t* __restrict__ wide_count,
                                                   const uint32_t* __restrict__ wide_idx, KeyCache kc) {
  const int pool = c == PLAN_ED ? 0 : 1;
  const uint32_t n = wide_count[c];
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x) {
    const uint32_t i = wide[(size_t)c * n_keys + l];
    if (kc_commit(kc.owners[pool], wide_idx[i], hdr[i].status == 0))
      atomicAdd(&kc.ctr[pool * KC_CTRS + KC_CTR_BUILT], 1u);
  }
}
void kc_launch_commit(int c, uint32_t n_keys, const KeyWs& w, hipStream_t stream) {
  if (!w.kc.on()) return;
  hipLaunchKernelGGL(k_kc_commit, dim3(8), dim3(256), 0, stream, c, n_keys, (const EdKeyHdr*)w.hdr,
                     (const uint32_t*)w.wide, (const uint32_t*)w.wide_count, (const uint32_t*)w.wide_idx, w.kc);
}

// The items of family f's row-0 / quarter / full modes -> CG_NOT_RUN when k_key_classify flagged f
// (SKIP_MISMATCH_AT): their ladders or tables were skipped on the host's word. A uniform early exit
// otherwise (one load of the flag per wave).
__global__ void __launch_bounds__(256) k_mode_guard(const uint32_t* __restrict__ ranges,
                                                    const uint32_t* __restrict__ perm,
                                                    const uint32_t* __restrict__ full_count, uint32_t skip_mask,
                                                    uint8_t* __restrict__ status) {
  const uint32_t bad = full_count[SKIP_MISMATCH_AT] & skip_mask;
  if (!bad) return;
  for (int f = 0; f < 3; ++f) {
    if (!((bad >> f) & 1u)) continue;
    const int cls = f == 0 ? PLAN_R1 : f == 1 ? PLAN_K1 : PLAN_ED;
    const uint32_t beg = ranges[cls], end = ranges[PLAN_WIDE + cls];
    for (uint32_t p = beg + blockIdx.x * blockDim.x + threadIdx.x; p < end; p += gridDim.x * blockDim.x)
      status[perm[p]] = CG_NOT_RUN;
  }
}

hipError_t upload_constants() {
  hipError_t e = ed_upload_constants();
  if (e != hipSuccess) return e;
  e = ec_upload_constants();
  if (e != hipSuccess) return e;
  e = derive_upload_constants();
  if (e != hipSuccess) return e;
  return sign_ec_upload_constants();
}

size_t keyprep_bytes(uint32_t n_keys) { return key_ws_bytes(n_keys); }
size_t wide_bytes(uint32_t n_keys, uint64_t n_items, uint32_t max_slots) {
  return wide_pool_bytes(wide_cap(n_keys, n_items, max_slots));
}
size_t wide_slot_bytes() { return wide_pool_bytes(1); }
static_assert(kKeyWideMax == KEY_WIDE_MAX, "engine.h mirrors keyws.h");
WidePool make_wide_pool(void* base, uint32_t n_keys, uint64_t n_items, uint32_t max_slots, uint32_t alloc_slots) {
  return wide_pool(base, wide_cap(n_keys, n_items, max_slots), alloc_slots);
}
uint32_t wide_slots(uint32_t n_keys, uint64_t n_items, uint32_t max_slots) { return wide_cap(n_keys, n_items, max_slots); }
size_t key_cache_bytes(uint32_t slots) { return key_cache_total(slots); }
size_t item_ws_bytes(uint64_t n_items) { return item_ws_total(n_items); }
size_t btab_bytes() { return const_tab_bytes(); }
size_t btab_scratch_bytes() { return const_scratch_bytes(); }

hipError_t init_btab(void* d_btab, void* d_scratch, hipStream_t stream) {
  hipError_t e = ed_init_const(d_btab, d_scratch, stream);
  if (e != hipSuccess) return e;
  return ec_init_const(d_btab, d_scratch, stream);
}


// k_key_classify's outcome from the host counts: does any key of family f (0 r1, 1 k1, 2 Ed25519)
// end in row-0 or full-table mode? Mirrors the kernel (a counted key has u >= 1; wide when u >=
// max(ED_DIRECT_MAX_USES, the pool's minimum) and the pool's slots hold every such key).
static void families_needing_full(const KeyUses& src, uint32_t n_keys, const KeyWs& w, bool need[3]) {
  uint32_t hot[2] = {0, 0};  // keys asking for a wide slot, per pool (0 Ed25519, 1 ECDSA)
  bool low[3] = {false, false, false};
  for (uint32_t i = 0; i < n_keys; ++i) {
    const uint32_t u = src.host_counts[i];
    if (u == 0) continue;
    const uint8_t s = src.host_keys[i].scheme;
    const int f = s == CG_ECDSA_SECP256R1_SHA256 ? 0 : s == CG_ECDSA_SECP256K1_SHA256 ? 1 : s == CG_EDDSA_ED25519_SHA512 ? 2 : -1;
    if (f < 0) continue;
    const int pool = f == 2 ? 0 : 1;
    const uint32_t cap = pool == 0 ? w.cap_ed : w.cap_ec;
    if (u >= ED_DIRECT_MAX_USES && u >= (pool == 0 ? w.min_ed : w.min_ec) && u != KEY_USES_ALL && cap) ++hot[pool];
    else low[f] = true;
  }
  const bool over[2] = {hot[0] > w.cap_ed, hot[1] > w.cap_ec};
  for (int f = 0; f < 3; ++f) need[f] = low[f] || over[f == 2 ? 0 : 1];
}

// What the key stages of one call launch over.
struct KeyArgs {
  const VerifyReq& r;
  const cg_item* d_items;  // null: the items are not made yet (`src`), or there are none
  uint64_t n_items;
  const KeyUses* src;
  KeyWs w;
  uint32_t all;  // k_key_init: every key counts as used by everything (no counts)
};

// launch_schedule.h over HIP: the enums as this call's streams, the fork's events and the
// launchers. The table builds run from what launch_keyprep left in fork.pending, the item stages
// over one chunk's ItemArgs.
struct HipOps {
  using Error = hipError_t;
  static constexpr Error kOk = hipSuccess;
  hipStream_t main;
  const Fork& fork;
  const KeyArgs* key = nullptr;
  const ItemArgs* a = nullptr;
  KeyWs w{};   // of the chunk's keys (with `a`)
  ItemWs iw{};

  HipOps(hipStream_t s, const Fork& f, const KeyArgs* k, const ItemArgs* items) : main(s), fork(f), key(k), a(items) {
    if (!a) return;
    w = key_ws((void*)a->d_keyprep, a->n_keys, a->wide);
    iw = item_ws(a->d_item_ws, a->n_items);
  }
  hipStream_t st(cgs::Stream s) const { return s == cgs::MAIN ? main : fork.side[s - cgs::SIDE0]; }
  hipEvent_t ev(cgs::Event e) const {
    switch (e) {
      case cgs::EV_START: return fork.start;
      case cgs::EV_PLANNED: return fork.planned;
      case cgs::EV_READY0: case cgs::EV_READY1: case cgs::EV_READY2: return fork.ready[e - cgs::EV_READY0];
      case cgs::EV_FRONT: return fork.front;
      case cgs::EV_ROW0_0: case cgs::EV_ROW0_1: case cgs::EV_ROW0_2: return fork.row0[e - cgs::EV_ROW0_0];
      case cgs::EV_EC_FRONT_GO: return fork.ec_front_go;
      case cgs::EV_EC_FRONT_DONE0: case cgs::EV_EC_FRONT_DONE1: return fork.ec_front_done[e - cgs::EV_EC_FRONT_DONE0];
      default: return nullptr;
    }
  }
  Error record(cgs::Event e, cgs::Stream s) { return hipEventRecord(ev(e), st(s)); }
  Error wait(cgs::Stream s, cgs::Event e) { return hipStreamWaitEvent(st(s), ev(e), 0); }
  bool mid_hook() const { return fork.mid_front != nullptr; }
  void before_joins() {
    if (fork.mark) hipEventRecord(fork.mark, main);
  }

  Error run(cgs::Stage stage, cgs::Stream on, int, int) {
    hipStream_t s = st(on);
    switch (stage) {
      // ---- key stages
      case cgs::ST_KEY_INIT: {
        const uint32_t n = key->r.n_keys, kl = n > PLAN_CLASSES + 2 ? n : PLAN_CLASSES + 2;
        hipLaunchKernelGGL(k_key_init, dim3((kl + 255) / 256), dim3(256), 0, s, n, key->all, key->w.uses, key->w.seen,
                           key->w.full_count, key->w.wide_idx, key->w.wide_count);
        return kOk;
      }
      case cgs::ST_KEY_USES:
        hipLaunchKernelGGL(k_key_uses, dim3((unsigned)((key->n_items + 255) / 256)), dim3(256), 0, s, key->d_items,
                           key->n_items, key->r.n_keys, key->w.uses, key->w.seen);
        return kOk;
      case cgs::ST_KEY_COUNTS:
        hipLaunchKernelGGL(k_key_counts, dim3((key->r.n_keys + 255) / 256), dim3(256), 0, s, key->src->counts,
                           key->r.n_keys, key->w.uses, key->w.seen);
        return kOk;
      case cgs::ST_KEY_USES_TXSIG:
        with_records(key->src->sigs, [&](auto* recs) {
          using Rec = std::remove_const_t<std::remove_pointer_t<decltype(recs)>>;
          hipLaunchKernelGGL(k_key_uses_txsig<Rec>, dim3((unsigned)((key->src->n + 255) / 256)), dim3(256), 0, s, recs,
                             key->src->n, key->r.n_keys, key->w.uses, key->w.seen);
        });
        return kOk;
      case cgs::ST_KC_BEGIN:
        hipLaunchKernelGGL(k_kc_begin, dim3(2), dim3(KC_BLOCK), 0, s, key->w.kc);
        return kOk;
      case cgs::ST_KEY_CLASSIFY: {
        const KeyWs& kw = key->w;
        hipLaunchKernelGGL(k_key_classify, dim3((key->r.n_keys + 63) / 64), dim3(64), 0, s, key->r.d_keys, key->r.n_keys,
                           kw.uses, (const uint8_t*)kw.seen, kw.full, kw.full_count, kw.wide_idx, kw.wide, kw.wide_count,
                           kw.row0, kw.quart, kw.cap_ed, kw.cap_ec, kw.min_ed, kw.min_ec, fork.pending.skip_mask,
                           key->r.d_arena, key->r.arena_len, kw.kc);
        return kOk;
      }
      case cgs::ST_KC_CLAIM: {
        const KeyWs& kw = key->w;
        hipLaunchKernelGGL(k_kc_claim, dim3(2), dim3(KC_BLOCK), 0, s, key->r.d_keys, key->r.n_keys, key->r.d_arena,
                           key->r.arena_len, kw.wide_idx, kw.wide, kw.wide_count, kw.full, kw.full_count, kw.row0,
                           fork.pending.skip_mask, kw.kc);
        return kOk;
      }
      // decodes and row-base chains (few waves, latency-bound)
      case cgs::ST_CHAINS_R1: case cgs::ST_CHAINS_K1:
        ec_launch_keyprep_chains(stage == cgs::ST_CHAINS_R1 ? CG_CURVE_R1 : CG_CURVE_K1, key->r.d_keys, key->r.n_keys,
                                 key->r.d_arena, key->r.arena_len, key->w, s);
        return kOk;
      case cgs::ST_CHAINS_ED:
        ed_launch_keyprep_chains(key->r.d_keys, key->r.n_keys, key->r.d_arena, key->r.arena_len, key->w, s);
        return kOk;
      // the tables (the wide ones hold every SIMD for milliseconds)
      case cgs::ST_WIDE_TABS_R1: case cgs::ST_WIDE_TABS_K1: case cgs::ST_WIDE_TABS_ED:
      case cgs::ST_FULL_TABS_R1: case cgs::ST_FULL_TABS_K1: case cgs::ST_FULL_TABS_ED: {
        const PendingTabs& p = fork.pending;
        const KeyWs pw = key_ws(p.keyprep, p.n_keys, &p.wide);
        const bool full = stage >= cgs::ST_FULL_TABS_R1;
        const int k = stage - (full ? cgs::ST_FULL_TABS_R1 : cgs::ST_WIDE_TABS_R1);
        if (k == 2) ed_launch_keyprep_tabs(p.keys, p.n_keys, pw, s, full, !full);
        else ec_launch_keyprep_tabs(k == 0 ? CG_CURVE_R1 : CG_CURVE_K1, p.keys, p.n_keys, pw, s, full, !full);
        return kOk;
      }
      // the only key work on the main stream: Abyte for k_ed_hash (no decode)
      case cgs::ST_ED_ABYTE:
        ed_launch_key_abyte(key->r.d_keys, key->r.n_keys, key->r.d_arena, key->r.arena_len, key->w, s);
        return kOk;
      // ---- item stages
      case cgs::ST_MISC_STATUS:
        hipLaunchKernelGGL(k_misc_status, dim3((unsigned)((a->n_items + 255) / 256)), dim3(256), 0, s, a->d_items,
                           a->n_items, a->d_keys, a->n_keys, a->d_status);
        return kOk;
      case cgs::ST_PLAN: {  // items sorted by (scheme class, key) (plan_sort.hip)
        Error e = kOk;
        CG_TIME(fork, CG_STAGE_PLAN, s, e = launch_plan(a->d_items, a->n_items, a->d_keys, a->n_keys, w, iw, s));
        return e;
      }
      case cgs::ST_MID_HOOK: return (*fork.mid_front)();  // (the hook clears itself)
      case cgs::ST_EC_FRONT_R1: case cgs::ST_EC_FRONT_K1: {
        const bool r1 = stage == cgs::ST_EC_FRONT_R1;
        CG_TIME(fork, r1 ? CG_STAGE_R1_FRONT : CG_STAGE_K1_FRONT, s,
                ec_launch_front(r1 ? CG_CURVE_R1 : CG_CURVE_K1, a->d_items, a->n_items, a->d_arena, a->arena_len, a->mode,
                                a->d_status, w, a->d_msgs, a->msgs_len, iw, s));
        return kOk;
      }
      case cgs::ST_ED_FRONT:
        CG_TIME(fork, CG_STAGE_ED_HASH, s,
                ed_launch_front(a->d_items, a->n_items, a->d_arena, a->arena_len, a->mode, a->d_status, w, a->d_msgs,
                                a->msgs_len, iw, s));
        return kOk;
      case cgs::ST_ROW0_LADDER_ED:
        CG_TIME(fork, CG_STAGE_ED_LADDER_ROW0, s,
                ed_launch_ladder(false, a->d_items, a->n_items, a->d_status, w, iw, a->d_btab, s));
        return kOk;
      case cgs::ST_ROW0_LADDER_R1: case cgs::ST_ROW0_LADDER_K1: {
        const bool r1 = stage == cgs::ST_ROW0_LADDER_R1;
        CG_TIME(fork, r1 ? CG_STAGE_R1_LADDER_ROW0 : CG_STAGE_K1_LADDER_ROW0, s,
                ec_launch_ladder(r1 ? CG_CURVE_R1 : CG_CURVE_K1, false, a->d_items, a->n_items, a->d_status, w, iw,
                                 a->d_btab, s));
        return kOk;
      }
      case cgs::ST_FULL_LADDER_ED:
        CG_TIME(fork, CG_STAGE_ED_LADDER, s,
                ed_launch_ladder(true, a->d_items, a->n_items, a->d_status, w, iw, a->d_btab, s));
        return kOk;
      case cgs::ST_WIDE_LADDER_ED:
        CG_TIME(fork, CG_STAGE_ED_LADDER_WIDE, s,
                ed_launch_ladder_wide(a->d_items, a->n_items, a->d_status, w, iw, a->d_btab, s));
        return kOk;
      // (16 items per lane share an inversion: ~1.6 waves per SIMD, latency-bound)
      case cgs::ST_ED_FINISH:
        CG_TIME(fork, CG_STAGE_ED_FINISH, s,
                ed_launch_finish(a->d_items, a->n_items, a->d_arena, a->arena_len, a->d_status, iw, s));
        return kOk;
      case cgs::ST_FULL_LADDER_R1: case cgs::ST_FULL_LADDER_K1: {
        const bool r1 = stage == cgs::ST_FULL_LADDER_R1;
        CG_TIME(fork, r1 ? CG_STAGE_R1_LADDER : CG_STAGE_K1_LADDER, s,
                ec_launch_ladder(r1 ? CG_CURVE_R1 : CG_CURVE_K1, true, a->d_items, a->n_items, a->d_status, w, iw,
                                 a->d_btab, s));
        return kOk;
      }
      case cgs::ST_WIDE_LADDER_R1: case cgs::ST_WIDE_LADDER_K1: {
        const bool r1 = stage == cgs::ST_WIDE_LADDER_R1;
        CG_TIME(fork, r1 ? CG_STAGE_R1_LADDER_WIDE : CG_STAGE_K1_LADDER_WIDE, s,
                ec_launch_ladder_wide(r1 ? CG_CURVE_R1 : CG_CURVE_K1, a->d_items, a->n_items, a->d_status, w, iw,
                                      a->d_btab, s));
        return kOk;
      }
      case cgs::ST_MODE_GUARD:  // after every ladder and the finish of this chunk
        hipLaunchKernelGGL(k_mode_guard, dim3(64), dim3(256), 0, s, (const uint32_t*)iw.ranges, (const uint32_t*)iw.perm,
                           (const uint32_t*)w.full_count, fork.pending.skip_mask, a->d_status);
        return kOk;
      default: return hipErrorInvalidValue;  // the RSA passes and the prepare hook are cordagpu.cpp's
    }
  }
};
using Sched = cgs::Schedule<HipOps>;

static cgs::Chunk chunk_of(const HipOps& ops) {
  cgs::Chunk c;
  c.wide_ed = ops.w.cap_ed != 0;
  c.wide_ec = ops.w.cap_ec != 0;
  return c;
}

// The table builds launch_keyprep deferred (launch_schedule.h key_tables).
hipError_t launch_key_tables(const Fork& fork, hipStream_t stream) {
  HipOps ops(stream, fork, nullptr, nullptr);
  return Sched(ops, fork.pending).key_tables();
}

hipError_t launch_keyprep(const VerifyReq& r, void* d_keyprep, hipStream_t stream, const Fork& fork,
                          const WidePool* wide, const KeyUses* src) {
  const uint32_t n_keys = r.n_keys;
  const cg_item* d_items = src ? nullptr : r.d_items;  // with `src` the items are not made yet
  const uint64_t n_items = src ? src->n : r.n_items;
  const bool counted = d_items || src;  // tables sized by the call's key uses
  const KeyArgs key = {r, d_items, n_items, src, key_ws(d_keyprep, n_keys, counted ? wide : nullptr), counted ? 0u : 1u};
  cgs::KeyPlan k;
  k.any_keys = n_keys != 0;
  k.counted = counted;
  // use counts first (main stream; the side streams fork after them)
  if (d_items && n_items) k.uses = cgs::ST_KEY_USES;
  else if (src && src->counts) k.uses = cgs::ST_KEY_COUNTS;
  else if (src && src->sigs.p && src->n) k.uses = cgs::ST_KEY_USES_TXSIG;
  // every mode's builds and ladders unless this call's host counts prove a family has no row-0 /
  // quarter / full key; the classification checks that proof on the device (k_mode_guard)
  if (n_keys && !d_items && src && src->counts && src->host_counts && src->host_keys)
    families_needing_full(*src, n_keys, key.w, k.need_full);
  // CG_TEST_SKIP_FAMILIES=<mask> (tests only): skip those families' row-0 / quarter / full work as
  // if the host counts had proved it unneeded, so that the device check can be seen to catch it
  static const uint32_t test_skip = [] {
    const char* v = getenv("CG_TEST_SKIP_FAMILIES");
    return v ? (uint32_t)strtoul(v, nullptr, 0) & 7u : 0u;
  }();
  for (int f = 0; f < 3; ++f)
    if ((test_skip >> f) & 1u) k.need_full[f] = false;
  // the wide-table cache (key_cache.h): its index before the classification probes it, the claim
  // pass after; all on the main stream, ahead of the fork
  k.cache = key.w.kc.on();
  k.wide_ed = key.w.cap_ed != 0;
  k.wide_ec = key.w.cap_ec != 0;
  // what the table builds launch over, now or after the first chunk's plan sort when items follow
  // (its decoupled look-back stalls behind them)
  if (n_keys) {
    fork.pending.keys = r.d_keys;
    fork.pending.n_keys = n_keys;
    fork.pending.keyprep = d_keyprep;
    fork.pending.wide = counted && wide ? *wide : WidePool{};
  }
  HipOps ops(stream, fork, &key, nullptr);
  const hipError_t e = Sched(ops, fork.pending).keyprep(k);
  return e != hipSuccess || n_keys == 0 ? e : hipGetLastError();
}

hipError_t launch_items_plan(const ItemArgs& a, hipStream_t stream, const Fork& fork) {
  if (a.n_items == 0) return hipSuccess;
  HipOps ops(stream, fork, nullptr, &a);
  return Sched(ops, fork.pending).items_plan(chunk_of(ops));
}

hipError_t launch_items_front(const ItemArgs& a, hipStream_t stream, const Fork& fork, bool planned) {
  if (a.n_items == 0) return hipSuccess;
  HipOps ops(stream, fork, nullptr, &a);
  const hipError_t e = Sched(ops, fork.pending).items_front(chunk_of(ops), planned);
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_items_back(const ItemArgs& a, hipStream_t stream, const Fork& fork) {
  if (a.n_items == 0) return hipSuccess;
  HipOps ops(stream, fork, nullptr, &a);
  const hipError_t e = Sched(ops, fork.pending).items_back(chunk_of(ops));
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_items(const ItemArgs& a, hipStream_t stream, const Fork& fork) {
  const hipError_t e = launch_items_front(a, stream, fork, false);
  return e != hipSuccess ? e : launch_items_back(a, stream, fork);
}

// This build's entry points for the C ABI layer (engine.h EngineVariant; one per fixed-base radix).
static_assert(ED_WIDE_BW == EC_WIDE_GW, "one fixed-base radix per build (Makefile VARIANTS)");
const EngineVariant& variant() {
  static const EngineVariant v = {(uint32_t)ED_WIDE_BW, upload_constants, keyprep_bytes, wide_bytes, wide_slot_bytes,
                                  make_wide_pool, wide_slots, key_cache_bytes, btab_bytes, btab_scratch_bytes, init_btab, item_ws_bytes,
                                  launch_keyprep, launch_key_tables, launch_items, launch_items_plan,
                                  launch_items_front, launch_items_back,
                                  signer_bytes, sign_ws_bytes, launch_signer_expand, launch_sign,
                                  derive_ws_bytes, launch_derive_parents, launch_derive,
                                  ec_signer_bytes, sign_ec_ws_bytes, launch_ec_signer_expand, launch_sign_ec};
  return v;
}

}  // namespace cg
