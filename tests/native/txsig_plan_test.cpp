// CPU driver of corda_amd/csrc/txsig_plan.h (tests/test_txsig_plan.py): the host tx-signature
// path's chunk bounds, key-use counts, extents, resident intervals and packed fix-up, exported
// through a C ABI so the test can compare whole arrays with its numpy restatement. `nt` parts run
// on nt real threads (a HostPool of nt - 1 workers, as the library's contexts do).
#include "../../corda_amd/csrc/txsig_plan.h"

#include "../../corda_amd/csrc/host_pool.h"

namespace {

struct Par {
  cg::HostPool pool;
  cg::ParFor fn;
  explicit Par(uint64_t nt)
      : pool((unsigned)(nt > 1 ? nt - 1 : 0)),
        fn([this](uint64_t m, const std::function<void(uint64_t)>& f) { pool.run(m, f); }) {}
};

cg::CountScratch g_scratch;  // kept across calls, as a context keeps its own

uint64_t put(const std::vector<std::pair<uint64_t, uint64_t>>& v, uint64_t* out, uint64_t cap) {
  for (uint64_t i = 0; i < v.size() && i < cap; ++i) {
    out[2 * i] = v[i].first;
    out[2 * i + 1] = v[i].second;
  }
  return v.size();
}

}  // namespace

extern "C" {

uint64_t tp_bounds(uint64_t n_sigs, uint64_t chunk, int chunk_set, uint64_t first_div, uint64_t* out, uint64_t cap,
                   uint64_t* largest) {
  const std::vector<uint64_t> b = cg::txsig_bounds(n_sigs, chunk, chunk_set != 0, first_div);
  for (uint64_t i = 0; i < b.size() && i < cap; ++i) out[i] = b[i];
  *largest = cg::largest_chunk(b);
  return b.size();
}

uint64_t tp_equal_bounds(uint64_t n, uint64_t per, uint64_t* out, uint64_t cap) {
  const std::vector<uint64_t> b = cg::equal_bounds(n, per);
  for (uint64_t i = 0; i < b.size() && i < cap; ++i) out[i] = b[i];
  return b.size();
}

uint32_t tp_sample_override(uint32_t x) { return cg::sample_override(x); }
uint32_t tp_sample_block(uint32_t x) { return cg::sample_block(x); }
uint32_t tp_sample_rate(uint32_t s_override, uint64_t n_sigs, uint32_t n_keys) {
  return cg::sample_rate(s_override, n_sigs, n_keys);
}
uint32_t tp_estimate(uint64_t c, uint32_t S, uint64_t wmin, uint64_t floor_hot) {
  return cg::estimate_uses(c, S, wmin, floor_hot);
}
uint64_t tp_hot_floor(uint32_t S, uint32_t min_ed, uint32_t min_ec) { return cg::hot_floor(S, min_ed, min_ec); }

// tab: cg_txsig_packed records when packed, else cg_txsig; counts: max(n_keys, 1) entries, zeroed here
void tp_count_exact(int packed, const void* tab, uint64_t n_sigs, uint32_t n_keys, uint64_t nt, uint32_t* counts) {
  Par par(nt);
  memset(counts, 0, sizeof(uint32_t) * (n_keys ? n_keys : 1));
  if (packed) cg::count_exact((const cg_txsig_packed*)tab, n_sigs, n_keys, nt, par.fn, g_scratch, counts);
  else cg::count_exact((const cg_txsig*)tab, n_sigs, n_keys, nt, par.fn, g_scratch, counts);
}

void tp_count_sampled(int packed, const void* tab, uint64_t n_sigs, uint32_t n_keys, uint64_t nt, uint32_t S,
                      uint32_t B, uint32_t* counts) {
  Par par(nt);
  memset(counts, 0, sizeof(uint32_t) * (n_keys ? n_keys : 1));
  if (packed) cg::count_sampled((const cg_txsig_packed*)tab, n_sigs, n_keys, nt, par.fn, S, B, counts);
  else cg::count_sampled((const cg_txsig*)tab, n_sigs, n_keys, nt, par.fn, S, B, counts);
}

void tp_key_use_counts(int packed, const void* tab, uint64_t n_sigs, const cg_key* keys, uint32_t n_keys, uint64_t nt,
                       uint32_t S, uint32_t B, uint32_t min_ed, uint32_t min_ec, uint32_t* counts) {
  Par par(nt);
  memset(counts, 0, sizeof(uint32_t) * (n_keys ? n_keys : 1));
  if (packed)
    cg::key_use_counts((const cg_txsig_packed*)tab, n_sigs, keys, n_keys, nt, par.fn, S, B, min_ed, min_ec, g_scratch,
                       counts);
  else
    cg::key_use_counts((const cg_txsig*)tab, n_sigs, keys, n_keys, nt, par.fn, S, B, min_ed, min_ec, g_scratch, counts);
}

// x = {lo, hi}, updated in place
void tp_extent_add(uint64_t* x, uint64_t off, uint64_t len, uint64_t arena_len) {
  cg::Extent e;
  e.lo = x[0];
  e.hi = x[1];
  e.add(off, len, arena_len);
  x[0] = e.lo;
  x[1] = e.hi;
}
int tp_extent_empty(uint64_t lo, uint64_t hi) {
  cg::Extent e;
  e.lo = lo;
  e.hi = hi;
  return e.empty() ? 1 : 0;
}

void* tp_resident_new() { return new cg::Resident(); }
void tp_resident_free(void* r) { delete (cg::Resident*)r; }
// the gaps of [lo, hi) as (first, second) pairs in out; returns how many
uint64_t tp_resident_missing(void* r, uint64_t lo, uint64_t hi, uint64_t* out, uint64_t cap) {
  cg::Extent e;
  e.lo = lo;
  e.hi = hi;
  return put(((cg::Resident*)r)->missing(e), out, cap);
}
uint64_t tp_resident_have(void* r, uint64_t* out, uint64_t cap) { return put(((cg::Resident*)r)->have, out, cap); }

// out = {sig.lo, sig.hi, ids.lo, ids.hi, span}
void tp_scan_chunk(int packed, const void* tab, uint64_t f, uint64_t e, uint64_t n_ids, uint64_t arena_len, uint64_t nt,
                   uint64_t* out) {
  Par par(nt);
  const cg::ChunkScan x = packed ? cg::scan_chunk((const cg_txsig_packed*)tab, f, e, n_ids, arena_len, nt, par.fn)
                                 : cg::scan_chunk((const cg_txsig*)tab, f, e, n_ids, arena_len, nt, par.fn);
  out[0] = x.sig.lo;
  out[1] = x.sig.hi;
  out[2] = x.ids.lo;
  out[3] = x.ids.hi;
  out[4] = x.span;
}

void tp_head_extent(const cg_key* keys, uint32_t n_keys, const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                    uint64_t arena_len, uint64_t* out) {
  const cg::Extent h = cg::txsig_head_extent(keys, n_keys, tmpls, n_tmpls, arena_len);
  out[0] = h.lo;
  out[1] = h.hi;
}

// bit 0: a key was moved out (keys_out holds the corrected table), bit 1: a template (tmpls_out)
int tp_fixup(const cg_key* keys, uint32_t n_keys, const cg_signable_tmpl* tmpls, uint32_t n_tmpls, uint64_t caller_len,
             cg_key* keys_out, cg_signable_tmpl* tmpls_out) {
  std::vector<cg_key> kf;
  std::vector<cg_signable_tmpl> tf;
  cg::txsig_packed_fixup(keys, n_keys, tmpls, n_tmpls, caller_len, kf, tf);
  if (!kf.empty()) memcpy(keys_out, kf.data(), sizeof(cg_key) * n_keys);
  if (!tf.empty()) memcpy(tmpls_out, tf.data(), sizeof(cg_signable_tmpl) * n_tmpls);
  return (kf.empty() ? 0 : 1) | (tf.empty() ? 0 : 2);
}

}  // extern "C"
