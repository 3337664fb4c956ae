// C ABI of the MI355X batch signature-verification engine (include/cordagpu.h).
//
// Thin host layer: argument checks, per-context device workspace, H2D/D2H for the
// host-buffer entry points, and kernel launches through engine.h. No CPU fallback: every
// verdict is computed by the HIP kernels; if the device is unusable the call fails with
// CG_ERR_DEVICE and the status bytes stay CG_NOT_RUN.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cordagpu.h"
#include "call_scope.h"
#include "engine.h"
#include "host_budget.h"
#include "host_pool.h"
#include "pool.h"
#include "rsa.h"
#include "table_budget.h"
#include "txsig_plan.h"

// the other builds of the radix-dependent kernels (Makefile VARIANTS; engine.h EngineVariant)
namespace cg24 {
const cgt::EngineVariant& variant();
}
namespace cg22 {
const cgt::EngineVariant& variant();
}

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, const char* detail = "") {
  char buf[512];
  snprintf(buf, sizeof buf, fmt, detail);
  g_err = buf;
  return code;
}

int hip_fail(hipError_t e, const char* where) {
  char buf[512];
  snprintf(buf, sizeof buf, "%s: %s", where, hipGetErrorString(e));
  g_err = buf;
  return e == hipErrorOutOfMemory ? CG_ERR_NOMEM : CG_ERR_DEVICE;
}

#define HIP_TRY(expr, where)               \
  do {                                     \
    hipError_t _e = (expr);                \
    if (_e != hipSuccess) return hip_fail(_e, where); \
  } while (0)

// Environment switches (A/B runs). A caller keeps the value in a function-local static, so each
// is read once per process: flags are on with a leading '1' (default off) or off with a leading '0'
// (default on); numbers are decimal.
bool env_flag(const char* name, bool dflt) {
  const char* v = getenv(name);
  return v ? (dflt ? v[0] != '0' : v[0] == '1') : dflt;
}
uint64_t env_u64(const char* name, uint64_t dflt) {
  const char* v = getenv(name);
  return v ? (uint64_t)strtoull(v, nullptr, 10) : dflt;
}

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) { return bytes <= cap ? hipSuccess : replace(bytes + bytes / 4 + 256); }
  // exactly `bytes` (no growth margin): for the multi-GB wide-table pools
  hipError_t ensure_exact(size_t bytes) { return bytes <= cap ? hipSuccess : replace(bytes); }
  hipError_t replace(size_t want) {
    release();
    const hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Grows whichever of the buffers are short, after waiting for the device: an earlier call's kernels
// may still be using them (cg_reserve ahead of time avoids the wait).
struct Need {
  DevBuf* buf;
  size_t bytes;
};
hipError_t ensure_all(std::initializer_list<Need> needs) {
  bool grow = false;
  for (const Need& n : needs) grow = grow || n.buf->cap < n.bytes;
  if (!grow) return hipSuccess;
  hipError_t e = hipDeviceSynchronize();
  for (const Need& n : needs)
    if (e == hipSuccess) e = n.buf->ensure(n.bytes);
  return e;
}

// A host form's table to its device buffer: room for `room` bytes (at least the table, never nothing),
// then the copy, if there is anything to copy.
hipError_t stage(DevBuf& b, const void* src, size_t bytes, hipStream_t s, size_t room = 0) {
  hipError_t e = b.ensure(std::max<size_t>({bytes, room, 1}));
  if (e == hipSuccess && bytes) e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s);
  return e;
}
// A whole arena on the device: rounded up to the kernels' aligned dword loads, plus slack.
size_t arena_room(uint64_t arena_len) { return ((arena_len + 3) & ~(uint64_t)3) + 16; }

// The stream API of call_scope.h over HIP.
struct HipStreams {
  using Stream = hipStream_t;
  using Event = hipEvent_t;
  using Error = hipError_t;
  static constexpr Error kOk = hipSuccess;
  Error record(Event e, Stream s) { return hipEventRecord(e, s); }
  Error wait(Stream s, Event e) { return hipStreamWaitEvent(s, e, 0); }
  Error sync(Stream s) { return hipStreamSynchronize(s); }
};

}  // namespace

// cg::CallState: the context's stream and copy stream (the host forms' H2D of chunk k + 1 overlaps
// the verify of chunk k), and the ordering of its calls (call_scope.h: done, bridge, caller)
struct cg_ctx : cg::CallState<HipStreams> {
  int device = 0;
  uint64_t chunk = CG_DEFAULT_CHUNK_ITEMS;  // items per verify chunk (cg_config.chunk_items)
  bool chunk_set = false;                   // the caller chose it (else the host tx-signature path pipelines finer)
  bool fault = false;                       // cg_pool_inject_fault drill: every call fails (enter)
  cg::Fork fork = {{nullptr, nullptr, nullptr}, nullptr, {nullptr, nullptr, nullptr}, nullptr,
                   {nullptr, nullptr, nullptr}, nullptr};
  std::mutex mu;
  DevBuf keyprep, itemws, keys, items, arena, status, aux0, aux1, aux2;
  // the constant fixed-base tables (B, both curves' G; 91 GB at radix 2^26, 25 GB at 2^24, 6.9 GB at
  // 2^22), shared by every context of this process on the device (acquire_tables / release_tables),
  // and the build of the radix-dependent kernels that reads them (table_budget.h picks it at cg_open)
  void* btab = nullptr;
  const cgt::EngineVariant* eng = nullptr;
  uint64_t tab_bytes = 0;
  DevBuf wide;  // wide-table pools (keyws.h), sized by the largest call's item count
  // RSA_SHA256 (CG_FLAG_RSA; verify_rsa.hip): per-key records and the per-call item list + counter.
  // Never allocated, and no RSA kernel launched, without the flag.
  bool rsa = false;
  DevBuf rsakeys, rsalist;
  // wide slots this context may allocate: lowered when the device's free memory cannot hold the
  // pool a call asks for (another process or context on the device), so the call runs
  // with fewer hot keys on wide tables (full tables for the rest: slower, same verdicts) instead of
  // failing with CG_ERR_NOMEM
  uint32_t wide_max = cg::kKeyWideMax;
  // The wide-table cache (key_cache.h): the pool keeps its slots' tables between calls, and a call
  // builds only the tables of the hot keys it does not find there. wide_slots: the slots the pool
  // was allocated for (its layout); kcache: the owners, index and counters on the device.
  // kc_dirty: the next call empties the cache first (the pool moved, or a call failed after it had
  // claimed slots: kc_open is set while a call is between its claim and the enqueue of its last
  // kernel, and a call that finds it set knows the one before did not get there).
  DevBuf kcache;
  uint32_t wide_slots = 0;
  uint32_t wide_slots_max = cg::kKeyWideMax;  // CG_TEST_WIDE_SLOTS (tests): a smaller pool
  uint32_t kc_bits = 32;                      // CG_TEST_KEY_CACHE_BITS (tests): 2^bits home entries in the index
  bool kc_on = true;                          // off: CG_FLAG_NO_KEY_CACHE, CG_KEY_CACHE=0
  bool kc_dirty = true;
  bool kc_open = false;
  // transaction pipeline: verify items, spliced messages, templates; host-entry staging
  DevBuf txitems, msgs, tmpls, h_txs, h_comps, h_sigs, h_ids, h_txst;
  DevBuf sig12ws;  // the 12-byte signature table's per-block stream offsets (launch_tx_sig12_range)
  // per-transaction verdicts (txverdict.hip): the long-span list, and the host forms' tables and results
  DevBuf txvws, txvio;
  // tear-offs: leaf-hash workspace
  DevBuf ftxws;
  // tear-off building (build_filtered.hip): the walks' workspace; the host forms' inputs that have no
  // buffer of their own above, and their result tables
  DevBuf bfws, bfin, bfio;
  // The Ed25519 signer (sign_ed.hip). signers: the expanded keys, an allocation of its own made by
  // cg_signers_load and zeroed before it is freed (secret: a, prefix); a context that never signs
  // allocates neither. signws: a chunk's r column and digit slots, zeroed behind every sign call.
  DevBuf signers, signws;
  uint32_t n_signers = 0;
  // Key derivation (derive_keys.hip): the parents' HMAC midstates and a chunk's slots (d, the digits),
  // zeroed behind every derive call. derive_force: CG_TEST_DERIVE_FORCE_RETRIES (tests only), the ECDSA
  // accept rule refuses the first that many attempts of every item.
  DevBuf derivews;
  uint32_t derive_force = 0;
  // The ECDSA signer (sign_ec.hip). ec_signers: d of every loaded key, an allocation of its own made by
  // cg_ec_signers_load and zeroed before it is freed; signecws: a chunk's k, k G and e, zeroed behind
  // every sign call. Separate from the Ed25519 set above.
  DevBuf ec_signers, signecws;
  uint32_t n_ec_signers = 0;
  // The RSA-PSS signer (sign_rsa.hip). rsa_signers: every loaded key's CRT parts and Montgomery constants,
  // an allocation of its own made by cg_rsa_signers_load and zeroed before it is freed; signrsaws: a
  // chunk's H and salts, zeroed behind every sign call. The third set, separate from the two above.
  DevBuf rsa_signers, signrsaws;
  uint32_t n_rsa_signers = 0;
  // host-buffer verify: one event per pipeline chunk (seg); timing events for cg_stats (tev)
  // a second stream on a hardware queue of its own, idle in every schedule: the CG_HOST_TRACE marker
  // "tables built" waits there (launch_chunked)
  hipStream_t copy2 = nullptr;
  // the exact key-use count's per-thread byte counters (txsig_plan.h), kept across calls so a call
  // does not page-fault 16 fresh arrays in
  cg::CountScratch count_scratch;
  // host threads for the host paths' scans (host_pool.h), started on the first large call and sized
  // by the budget (host_budget.h: cg_config.host_threads, CG_HOST_THREADS, or the CPU quota divided
  // by the contexts open in the process), re-sized when the budget changes
  std::unique_ptr<cg::HostPool> hpool;
  uint32_t host_req = 0;   // cg_config.host_threads
  uint32_t quota = 1;      // the process's CPUs at cg_open
  bool counted = false;    // included in g_live_ctx
  std::vector<hipEvent_t> seg;
  hipEvent_t tev[4] = {};
  std::vector<hipEvent_t> segt;  // CG_HOST_TRACE: timing events behind each chunk's copy
  std::vector<hipEvent_t> segtab;  // the host tx-signature path: chunk k's signature-table slice landed
  hipEvent_t backt[2] = {nullptr, nullptr};  // CG_HOST_TRACE: chunk 0's back enqueued / tables ready
  std::vector<hipEvent_t> fbt;  // CG_HOST_TRACE: per chunk, the main stream reaching its front / its back's end
  std::vector<double> fbh;      // host ms at which chunk k's front kernels were enqueued
  bool htrace = false;
  cg::StageTimer timer;  // used when opened with CG_FLAG_STAGE_TIMING
};

namespace {

// contexts open in this process (the default host budget divides the CPU quota among them)
std::atomic<unsigned> g_live_ctx{0};

// The builds of the radix-dependent kernels, largest tables first (table_budget.h).
const cgt::EngineVariant* const kVariants[] = {&cg::variant(), &cg24::variant(), &cg22::variant()};
constexpr int kNumVariants = 3;

std::vector<cgb::TableSet> table_sets() {
  std::vector<cgb::TableSet> v;
  for (const cgt::EngineVariant* e : kVariants) v.push_back({e->fixed_base_bits, (uint64_t)e->btab_bytes()});
  return v;
}

// The constant fixed-base tables, one copy per device per process: read-only after the build, so
// every context on the device (a cg_pool's slots, a test's second context) shares it instead of
// holding its own (keyws.h const_tab_bytes: Ed25519 B and both curves' G at the variant's radix).
struct SharedTables {
  int device;
  int variant;
  void* p;
  unsigned refs;
};
std::mutex g_tab_mu;
std::vector<SharedTables> g_tabs;

// Picks the tables for a context on `device` under `budget` (0: automatic) and builds or shares them:
// *out = the tables, *variant = the kernel build that reads them. Automatic: when the device cannot
// allocate the set the free memory suggested (another process took it meanwhile), the next smaller.
hipError_t acquire_tables(int device, hipStream_t s, uint64_t budget, void** out, int* variant) {
  std::lock_guard<std::mutex> g(g_tab_mu);
  const std::vector<cgb::TableSet> sets = table_sets();
  int held = -1;
  for (const SharedTables& t : g_tabs)
    if (t.device == device && (held < 0 || t.variant < held)) held = t.variant;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
  const int pick = cgb::pick_tables(sets.data(), kNumVariants, budget, free_b, held);
  if (pick < 0) return hipErrorInvalidValue;
  for (SharedTables& t : g_tabs)
    if (t.device == device && t.variant == pick) {
      ++t.refs;
      *out = t.p;
      *variant = pick;
      return hipSuccess;
    }
  hipError_t e = hipErrorOutOfMemory;
  for (int v = pick; v < kNumVariants; ++v) {
    if (budget && sets[v].bytes > budget) continue;
    void* p = nullptr;
    e = hipMalloc(&p, sets[v].bytes);
    if (e == hipSuccess) {  // built once over a temporary scratch, freed afterwards
      DevBuf scratch;
      e = scratch.ensure(kVariants[v]->btab_scratch_bytes());
      if (e == hipSuccess) e = kVariants[v]->upload_constants();
      if (e == hipSuccess) e = kVariants[v]->init_btab(p, scratch.p, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      scratch.release();
      if (e == hipSuccess) {
        g_tabs.push_back({device, v, p, 1u});
        *out = p;
        *variant = v;
        return hipSuccess;
      }
      hipFree(p);
    }
    (void)hipGetLastError();
    if (e != hipErrorOutOfMemory || budget) break;  // only the automatic choice steps down
  }
  return e;
}

void release_tables(int device, void* p) {
  std::lock_guard<std::mutex> g(g_tab_mu);
  for (size_t i = 0; i < g_tabs.size(); ++i)
    if (g_tabs[i].device == device && g_tabs[i].p == p) {
      if (--g_tabs[i].refs == 0) {
        hipSetDevice(device);
        hipFree(p);
        g_tabs.erase(g_tabs.begin() + (ptrdiff_t)i);
      }
      return;
    }
}

// The host threads a call of n items may use: 1 below 2^16 items, else the budget; the pool is
// (re)made to match, so nt parts run on nt threads.
unsigned host_threads_of(cg_ctx* c, uint64_t n) {
  if (n < (1u << 16)) return 1;
  const unsigned nt = cg::host_threads_for(c->host_req, cg::host_threads_env(), c->quota, g_live_ctx.load());
  if (nt <= 1) c->hpool.reset();  // a budget of one runs inline (host_par), not on an older, larger pool
  else if (!c->hpool || c->hpool->threads() != nt) c->hpool.reset(new cg::HostPool(nt - 1));
  return nt;
}

// fn(t) for t in [0, m) on the context's pool (or inline)
void host_par(cg_ctx* c, uint64_t m, const std::function<void(uint64_t)>& fn) {
  if (m > 1 && c->hpool) {
    c->hpool->run(m, fn);
  } else {
    for (uint64_t t = 0; t < m; ++t) fn(t);
  }
}

// One C-ABI call's ordering on its context (call_scope.h), declared with the ctx lock held and after
// every host buffer the call copies from. A device form opens it on the caller's stream and runs on
// stream(). A caller's stream is bridged to the context's own stream: HIP multiplexes streams onto
// GPU_MAX_HW_QUEUES (4) hardware queues in creation order, and a stream created elsewhere (torch's,
// the JVM's) can share an in-order queue with one of the side streams, whose milliseconds-long
// chains and table builds then run ahead of the call's main-stream kernels (round 6: the
// device-resident headline on torch's stream sat ~3.5 ms per step behind side stream 0's wide chain
// and rows, profiles/r06/bridge). The context's stream, created first, has a queue of its own.
// CG_STREAM_BRIDGE=0: run on the caller's stream itself (A/B; read at cg_open).
HipStreams g_hip;
struct Call : cg::CallScope<HipStreams> {
  Call(cg_ctx* c, Form form) : CallScope(g_hip, *c, form) {}
  hipError_t open(void* hip_stream = nullptr) { return CallScope::open((hipStream_t)hip_stream); }
};

// Every entry point's first step under the ctx lock: the drill fault fails the call, else its device.
int enter(cg_ctx* c, const char* fn) {
  if (c->fault) return fail(CG_ERR_DEVICE, "%s: device fault (injected by cg_pool_inject_fault)", fn);
  HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
  return CG_OK;
}

// Equal chunks of at most c->chunk items.
uint64_t chunk_of(const cg_ctx* c, uint64_t n) { return cg::equal_chunk(c->chunk, n); }

// Key and item workspace for n_keys keys and chunks of ws_items items, plus the wide-table pools
// for a call of call_items items (0: none). Growing them waits for the device (cg_reserve ahead
// of time avoids that).
// A call of more than one chunk gets two item workspaces (launch_chunked runs chunk k + 1's front
// before chunk k's back).
size_t item_half_bytes(const cg_ctx* c, uint64_t ws_items) { return (c->eng->item_ws_bytes(ws_items) + 255) & ~(size_t)255; }
// The RSA workspace (contexts with CG_FLAG_RSA only): key records and the item list. Grows like keyprep.
hipError_t ensure_rsa(cg_ctx* c, uint32_t n_keys, uint64_t n_items) {
  if (!c->rsa) return hipSuccess;
  return ensure_all({{&c->rsakeys, cg::rsa_keys_bytes(n_keys)}, {&c->rsalist, cg::rsa_list_bytes(n_items)}});
}
// The RSA halves of a call, on the stream of its other launches: the key records before any item
// stage, the item pass after the last chunk's back (the item table, the arena window, the tx items
// and the message workspace are whole-call buffers, intact until the call ends).
hipError_t rsa_keyprep(cg_ctx* c, const cg::VerifyReq& r, hipStream_t s) {
  if (!c->rsa) return hipSuccess;
  return cg::launch_rsa_keyprep(r, c->rsakeys.p, s);
}
hipError_t rsa_items(cg_ctx* c, const cg::VerifyReq& r, hipStream_t s) {
  if (!c->rsa || r.n_items == 0) return hipSuccess;
  return cg::launch_rsa_items(r, c->rsakeys.p, c->rsalist.p, s);
}

hipError_t ensure_ws(cg_ctx* c, uint32_t n_keys, uint64_t ws_items, uint64_t call_items = 0) {
  {
    const hipError_t re = ensure_rsa(c, n_keys, call_items > ws_items ? call_items : ws_items);
    if (re != hipSuccess) return re;
  }
  // the wide pool is sized for the full slot cap (KEY_WIDE_MAX) whenever the device can hold it: a
  // cap lowered by an earlier call that met low free memory (another process on the device) is
  // raised again here once the memory is back, instead of staying low for the
  // context's life
  const uint32_t kmax = c->wide_slots_max;
  size_t wide = c->eng->wide_bytes(n_keys, call_items, kmax);
  const size_t items = item_half_bytes(c, ws_items) * (call_items > ws_items ? 2 : 1);
  if (c->keyprep.cap >= c->eng->keyprep_bytes(n_keys) && c->itemws.cap >= items && c->wide.cap >= wide) {
    c->wide_max = kmax;
    return hipSuccess;
  }
  uint32_t cap = kmax;
  if (wide > c->wide.cap) {  // cap the wide pool by the device's free memory (keeping 1 GiB spare)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const size_t need_other = (c->keyprep.cap >= c->eng->keyprep_bytes(n_keys) ? 0 : c->eng->keyprep_bytes(n_keys)) +
                                (c->itemws.cap >= items ? 0 : items);
      const size_t avail = free_b + c->wide.cap;  // the current pool is freed before the new one
      const size_t spare = (size_t)1 << 30;
      if (wide + need_other + spare > avail) {
        const size_t room = avail > need_other + spare ? avail - need_other - spare : 0;
        cap = (uint32_t)std::min<size_t>(room / c->eng->wide_slot_bytes(), kmax);
        wide = c->eng->wide_bytes(n_keys, call_items, cap);
      }
    }
  }
  c->wide_max = cap;
  if (c->keyprep.cap >= c->eng->keyprep_bytes(n_keys) && c->itemws.cap >= items && c->wide.cap >= wide)
    return hipSuccess;  // still short of memory: the pool the context has is the largest that fits
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = c->keyprep.ensure(c->eng->keyprep_bytes(n_keys));
  if (e == hipSuccess) e = c->itemws.ensure(items);
  if (e == hipSuccess && wide > c->wide.cap) {  // a new pool, laid out by its own capacity: the cache starts empty
    e = c->wide.ensure_exact(wide);
    c->wide_slots = e == hipSuccess ? c->eng->wide_slots(n_keys, call_items, cap) : 0;
    c->kc_dirty = true;
    if (e == hipSuccess && c->kc_on) e = c->kcache.ensure(c->eng->key_cache_bytes(c->wide_slots));
  }
  return e;
}

// The wide pools a call may use: what ensure_ws reserved for it (none if the buffer is short).
cg::WidePool wide_for(cg_ctx* c, uint32_t n_keys, uint64_t n_items) {
  if (c->wide.cap < c->eng->wide_bytes(n_keys, n_items, c->wide_max)) return cg::WidePool{};
  cg::WidePool p = c->eng->make_wide_pool(c->wide.p, n_keys, n_items, c->wide_max, c->wide_slots);
  if (c->kc_on && p.cap_ed && c->kcache.p && c->kcache.cap >= c->eng->key_cache_bytes(p.slots)) {
    if (c->kc_open) {  // the last call failed between claim and commit: whatever it left on the streams ends first
      (void)hipDeviceSynchronize();
      c->kc_dirty = true;
    }
    p.cache = c->kcache.p;
    p.cache_bits = c->kc_bits;
    p.cache_dirty = c->kc_dirty;
    c->kc_dirty = false;
    c->kc_open = true;
  }
  // CG_WIDE_MIN_USES_ED / _EC: override the thresholds (A/B runs)
  static const uint32_t min_ed = (uint32_t)env_u64("CG_WIDE_MIN_USES_ED", 0);
  static const uint32_t min_ec = (uint32_t)env_u64("CG_WIDE_MIN_USES_EC", 0);
  if (min_ed) p.min_ed = min_ed;
  if (min_ec) p.min_ec = min_ec;
  return p;
}

// launch_chunked's options (the tx-signature entry points set them). prepare: called with (k, first
// item, items) just before chunk k's front is enqueued; it makes chunk k's verify items (and, host
// form, its bytes) and orders `s` after them. The key tables are then sized from `uses` and start
// building at once, before any chunk is prepared (so they overlap the host copies).
// prepare_blocks: the hook copies from host memory and blocks the enqueuing thread.
struct ChunkOpts {
  const std::function<hipError_t(uint64_t, uint64_t, uint64_t)>* prepare = nullptr;
  const cg::KeyUses* uses = nullptr;
  bool prepare_blocks = false;
};

// launch_schedule.h's engine over a context: one call's request, chunk bounds and workspaces. Each
// method enqueues through the context's engine build on the call's stream `s`.
struct CallEng {
  using Error = hipError_t;
  static constexpr Error kOk = hipSuccess;
  using Clock = std::chrono::steady_clock;
  cg_ctx* c;
  const cg::VerifyReq& r;
  hipStream_t s;
  const cg::WidePool* wp;               // null: no pools (prepared keys)
  const std::vector<uint64_t>& bounds;  // chunk k = items [bounds[k], bounds[k + 1])
  const ChunkOpts& o;
  uint64_t half_bytes = 0;              // of one item workspace when the buffer holds two
  bool closes_cache = true;             // the call claimed wide-table cache slots (wide_for)
  Clock::time_point h0;                 // CG_HOST_TRACE: the host's time to enqueue a chunk
  double prep_ms = 0, front_ms = 0, back_ms = 0;
  const char* where = "launch_items";   // the failing step's name in the error text

  static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
  // chunk k's items and status bytes, over item workspace `half`
  cg::ItemArgs chunk(unsigned k, int half) const {
    cg::ItemArgs a = {r, c->keyprep.p, c->itemws.p, c->btab, wp};
    a.d_items = r.d_items + bounds[k];
    a.n_items = bounds[k + 1] - bounds[k];
    a.d_status = r.d_status + bounds[k];
    a.d_item_ws = (uint8_t*)c->itemws.p + (size_t)half * half_bytes;
    return a;
  }
  Error at(const char* w, Error e) {
    if (e != hipSuccess) where = w;
    return e;
  }
  Error keyprep() { return at("launch_keyprep", c->eng->launch_keyprep(r, c->keyprep.p, s, c->fork, wp, o.uses)); }
  Error rsa_keyprep() { return at("launch_rsa_keyprep", ::rsa_keyprep(c, r, s)); }
  Error key_tables() { return c->eng->launch_key_tables(c->fork, s); }
  Error prepare(unsigned k) {
    h0 = Clock::now();
    const hipError_t w = (*o.prepare)(k, bounds[k], bounds[k + 1] - bounds[k]);
    prep_ms = ms(h0, Clock::now());
    return w;
  }
  Error plan(unsigned k, int half) { return c->eng->launch_items_plan(chunk(k, half), s, c->fork); }
  Error front(unsigned k, int half, bool planned) {
    if (!o.prepare) h0 = Clock::now();
    const hipError_t e = c->eng->launch_items_front(chunk(k, half), s, c->fork, planned);
    front_ms = ms(h0, Clock::now());
    return e;
  }
  Error back(unsigned k, int half) {
    const auto h1 = Clock::now();
    if (k == 0 && c->htrace && c->backt[0]) {  // chunk 0's front done; every table family built
      hipEventRecord(c->backt[0], s);
      hipStream_t t = c->copy2;  // idle by now: the marker waits there, nothing else does
      for (int q = 0; q < 3; ++q) hipStreamWaitEvent(t, c->fork.ready[q], 0);
      hipEventRecord(c->backt[1], t);
    }
    c->fork.mark = c->htrace && 3 * (size_t)k + 2 < c->fbt.size() ? c->fbt[3 * k + 2] : nullptr;  // before the joins
    const hipError_t x = c->eng->launch_items_back(chunk(k, half), s, c->fork);
    c->fork.mark = nullptr;
    if (c->htrace && 3 * (size_t)k + 1 < c->fbt.size()) hipEventRecord(c->fbt[3 * k + 1], s);  // back k ends
    back_ms = ms(h1, Clock::now());
    return x;
  }
  void chunk_enqueued(unsigned k) const {
    if (c->htrace)  // CG_HOST_TRACE: the host's time to enqueue chunk k (its front includes the copies)
      fprintf(stderr, "[cg host] chunk %llu enqueue: front %.3f ms (prepare %.3f, with the copies), back %.3f ms\n",
              (unsigned long long)k, front_ms, prep_ms, back_ms);
  }
  // the RSA pass over the whole call, after the last chunk's back
  Error rsa_pass(Error x) {
    if (x == hipSuccess && closes_cache) c->kc_open = false;  // every kernel of the call is enqueued, the cache's commits among them
    return x != hipSuccess ? x : at("launch_rsa_items", rsa_items(c, r, s));
  }
  Error wait(cgs::Stream, cgs::Event e) {  // the main stream for a family's tables
    return at("hipStreamWaitEvent", hipStreamWaitEvent(s, c->fork.ready[e - cgs::EV_READY0], 0));
  }
};

// Key tables once for the whole call (sized by every item's key use), then the items in chunks:
// chunk k = items [bounds[k], bounds[k + 1]) (bounds[0] = 0, the last one = r.n_items). The order
// of the enqueues is launch_schedule.h's `chunked`.
// (the device tx-signature forms with both first chunks' items and plans before the table builds,
// as the batch forms have them, measured slower: 388.3 vs 392.1 M sigs/s over 3 pairs,
// profiles/r06/preplan: chunk 0's Ed25519 ladder then starts earlier but shares the chip with chunk
// 1's ECDSA fronts, 12.5 vs 11.9 ms of ladder per step; the chip is already full in phase 1)
// (host copies in a blocking prepare hook: with chunk k + 1's front ahead of chunk k's back, chunk
// k's ladders waited for chunk k + 1's copy: profiles/r03/v5 timeline)
hipError_t launch_chunked(cg_ctx* c, const cg::VerifyReq& r, const std::vector<uint64_t>& bounds, hipStream_t s,
                          const ChunkOpts& o) {
  if (r.n_items == 0) return hipSuccess;
  const cg::WidePool wp = wide_for(c, r.n_keys, r.n_items);
  // `per` (the largest chunk) sizes the item workspaces: chunk k's is half k % 2 when the buffer
  // holds two (ensure_ws), else the one
  const uint64_t per = cg::largest_chunk(bounds);
  CallEng g = {c, r, s, &wp, bounds, o};
  g.half_bytes = item_half_bytes(c, per);
  cgs::CallPlan p;
  p.chunks = (unsigned)(bounds.size() - 1);
  p.two = p.chunks > 1 && c->itemws.cap >= 2 * g.half_bytes;
  p.hook = o.prepare != nullptr;
  p.hook_blocks = o.prepare_blocks;
  return cgs::chunked(g, p);
}

// ---- host-buffer verify: which arena bytes each pipeline chunk needs (txsig_plan.h)
using cg::Extent;

struct HostPlan {
  std::vector<uint64_t> first;  // chunk k = items [first[k], first[k+1])
  std::vector<Extent> ext;      // arena bytes chunk k reads
  Extent keys, win;             // key bytes; everything the call reads
};

void plan_host(cg_ctx* c, const cg_key* keys, uint32_t n_keys, const cg_item* items, uint64_t n_items,
               uint64_t arena_len, uint64_t per, HostPlan& P) {
  for (uint32_t k = 0; k < n_keys; ++k) P.keys.add(keys[k].off, keys[k].len, arena_len);
  const uint64_t nch = (n_items + per - 1) / per;
  P.first.resize(nch + 1);
  for (uint64_t k = 0; k <= nch; ++k) P.first[k] = n_items * k / nch;
  P.ext.assign(nch, Extent());
  // the chunks' scans on the context's host pool (the budget's threads): 32 B read per item
  auto scan = [&](uint64_t k) {
    Extent x;  // thread-local until the end (neighbouring chunks' slots share cache lines)
    for (uint64_t i = P.first[k]; i < P.first[k + 1]; ++i) {
      x.add(items[i].sig_off, items[i].sig_len, arena_len);
      x.add(items[i].msg_off, items[i].msg_len, arena_len);
    }
    P.ext[k] = x;
  };
  host_threads_of(c, n_items);
  host_par(c, nch, scan);
  P.win = P.keys;
  for (const Extent& e : P.ext) P.win.merge(e);
  if (P.win.empty()) P.win.lo = P.win.hi = 0;
  P.win.lo &= ~(uint64_t)15;  // the device window starts 16-aligned (kernels load aligned words)
}

// Copies the parts of [e.lo, e.hi) not yet resident.
hipError_t copy_missing(cg::Resident& have, const Extent& e, const uint8_t* arena, uint8_t* dwin, uint64_t win_lo,
                        hipStream_t s) {
  for (const auto& g : have.missing(e)) {
    hipError_t r = hipMemcpyAsync(dwin + (g.first - win_lo), arena + g.first, g.second - g.first,
                                  hipMemcpyHostToDevice, s);
    if (r != hipSuccess) return r;
  }
  return hipSuccess;
}

// At least n events without timing in v.
hipError_t ensure_events(std::vector<hipEvent_t>& v, uint64_t n) {
  while (v.size() < n) {
    hipEvent_t e;
    const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) return r;
    v.push_back(e);
  }
  return hipSuccess;
}

// The device timings of a host call (tev[0..3]: start, first chunk ready, verify done, verdicts back).
void fill_stats(cg_ctx* c, cg_stats* stats, uint64_t n_items, uint32_t n_keys, double ms_key_prep,
                std::chrono::steady_clock::time_point t0) {
  if (!stats) return;
  float a = 0, b = 0, d = 0;
  hipEventElapsedTime(&a, c->tev[0], c->tev[1]);
  hipEventElapsedTime(&b, c->tev[1], c->tev[2]);
  hipEventElapsedTime(&d, c->tev[2], c->tev[3]);
  stats->n_items = n_items;
  stats->n_keys = n_keys;
  stats->ms_h2d = a;
  stats->ms_key_prep = ms_key_prep;
  stats->ms_verify = b;
  stats->ms_d2h = d;
  stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// cg_verify_batch with the ctx lock held; `h` holds the caller's host buffers. On failure the status
// bytes are CG_NOT_RUN.
int verify_host_locked(cg_ctx* c, const cg::VerifyReq& h, cg_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  if (const int rc = enter(c, "cg_verify_batch")) return rc;
  const uint32_t n_keys = h.n_keys;
  const uint64_t n_items = h.n_items;
  const uint64_t pipe = c->chunk < CG_PIPELINE_CHUNK_ITEMS ? c->chunk : CG_PIPELINE_CHUNK_ITEMS;
  HostPlan P;
  plan_host(c, h.d_keys, n_keys, h.d_items, n_items, h.arena_len, pipe, P);
  const uint64_t nch = P.ext.size();
  const uint64_t per_max = (n_items + nch - 1) / nch;
  HIP_TRY(c->keys.ensure(sizeof(cg_key) * (n_keys ? n_keys : 1)), "hipMalloc(keys)");
  HIP_TRY(c->items.ensure(sizeof(cg_item) * n_items), "hipMalloc(items)");
  HIP_TRY(c->arena.ensure((P.win.hi - P.win.lo) + 16), "hipMalloc(arena window)");
  HIP_TRY(c->status.ensure(n_items), "hipMalloc(status)");
  HIP_TRY(ensure_ws(c, n_keys, per_max, n_items), "hipMalloc(workspace)");
  HIP_TRY(ensure_events(c->seg, nch), "hipEventCreate");
  hipStream_t s = c->stream;
  uint8_t* dwin = (uint8_t*)c->arena.p;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(hipEventRecord(c->tev[0], s), "hipEventRecord");
  HIP_TRY(hipStreamWaitEvent(c->copy, c->tev[0], 0), "hipStreamWaitEvent");
  cg::Resident have;
  if (n_keys)
    HIP_TRY(hipMemcpyAsync(c->keys.p, h.d_keys, sizeof(cg_key) * n_keys, hipMemcpyHostToDevice, c->copy), "H2D keys");
  HIP_TRY(copy_missing(have, P.keys, h.d_arena, dwin, P.win.lo, c->copy), "H2D key bytes");
  HIP_TRY(hipMemcpyAsync(c->items.p, h.d_items, sizeof(cg_item) * n_items, hipMemcpyHostToDevice, c->copy), "H2D items");
  // key tables sized by every item's key, built while chunk 0's arena bytes copy
  HIP_TRY(hipEventRecord(c->seg[0], c->copy), "hipEventRecord");
  HIP_TRY(hipStreamWaitEvent(s, c->seg[0], 0), "hipStreamWaitEvent");
  // the device's copy of the request; the kernels index the arena by absolute offsets: hand them the
  // window's base shifted back
  cg::VerifyReq d = h;
  d.d_keys = (const cg_key*)c->keys.p;
  d.d_items = (const cg_item*)c->items.p;
  d.d_arena = dwin - P.win.lo;
  d.d_status = (uint8_t*)c->status.p;
  const cg::WidePool wp = wide_for(c, n_keys, n_items);
  HIP_TRY(c->eng->launch_keyprep(d, c->keyprep.p, s, c->fork, &wp, nullptr), "launch_keyprep");
  cg::ItemArgs a = {d, c->keyprep.p, c->itemws.p, c->btab, &wp};
  HIP_TRY(rsa_keyprep(c, d, s), "launch_rsa_keyprep");
  for (uint64_t k = 0; k < nch; ++k) {
    HIP_TRY(copy_missing(have, P.ext[k], h.d_arena, dwin, P.win.lo, c->copy), "H2D arena");
    HIP_TRY(hipEventRecord(c->seg[k], c->copy), "hipEventRecord");
    HIP_TRY(hipStreamWaitEvent(s, c->seg[k], 0), "hipStreamWaitEvent");
    if (k == 0) HIP_TRY(hipEventRecord(c->tev[1], s), "hipEventRecord");
    a.d_items = d.d_items + P.first[k];
    a.n_items = P.first[k + 1] - P.first[k];
    a.d_status = d.d_status + P.first[k];
    HIP_TRY(c->eng->launch_items(a, s, c->fork), "launch_items");
  }
  c->kc_open = false;  // every kernel of the call is enqueued, the wide-table cache's commits among them
  HIP_TRY(rsa_items(c, d, s), "launch_rsa_items");
  HIP_TRY(hipEventRecord(c->tev[2], s), "hipEventRecord");
  HIP_TRY(hipMemcpyAsync(h.d_status, d.d_status, n_items, hipMemcpyDeviceToHost, s), "D2H status");
  HIP_TRY(hipEventRecord(c->tev[3], s), "hipEventRecord");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  fill_stats(c, stats, n_items, n_keys, 0, t0);
  return CG_OK;
}

// The argument checks of the cg_verify_batch family, after the ctx / pool check (host: the forms over
// host buffers, which the library itself reads)
int batch_args(const char* fn, const cg::VerifyReq& r, bool host) {
  if (r.n_items && (!r.d_items || !r.d_status)) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  if (host && r.n_keys && !r.d_keys) return fail(CG_ERR_ARG, "%s: keys is NULL", fn);
  if (host && r.arena_len && !r.d_arena) return fail(CG_ERR_ARG, "%s: arena is NULL", fn);
  if (r.mode > CG_MODE_ISVALID) return fail(CG_ERR_ARG, "%s: bad mode", fn);
  return CG_OK;
}

}  // namespace

extern "C" {

int cg_abi_version(void) { return CG_ABI_VERSION; }

const char* cg_build_info(void) {
  return "corda_amd libcordagpu: HIP kernels for gfx950 (Ed25519 i2p-0.2.0 semantics, ECDSA BC-1.57 semantics, "
         "SHA-256/512, Merkle tx ids)";
}

int cg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* cg_last_error(void) { return g_err.c_str(); }

// ---- host memory registration (include/cordagpu.h: zero-copy ingestion)
namespace {
struct HostRange {
  uint64_t lo, hi;
};
std::mutex g_reg_mu;
std::vector<HostRange> g_reg;  // registered ranges, disjoint
}  // namespace

int cg_host_register(const void* p, uint64_t len) {
  if (!p || !len) return fail(CG_ERR_ARG, "cg_host_register: NULL pointer or empty range");
  const uint64_t lo = (uint64_t)(uintptr_t)p, hi = lo + len;
  if (hi < lo) return fail(CG_ERR_ARG, "cg_host_register: range wraps the address space");
  std::lock_guard<std::mutex> g(g_reg_mu);
  for (const HostRange& r : g_reg)
    if (lo < r.hi && r.lo < hi) return fail(CG_ERR_ARG, "cg_host_register: range overlaps a registered one");
  // portable: every device's DMA engines may read the pages (a cg_pool's slots, one process per node)
  HIP_TRY(hipHostRegister(const_cast<void*>(p), (size_t)len, hipHostRegisterPortable), "hipHostRegister");
  g_reg.push_back({lo, hi});
  return CG_OK;
}

int cg_host_unregister(const void* p) {
  const uint64_t lo = (uint64_t)(uintptr_t)p;
  std::lock_guard<std::mutex> g(g_reg_mu);
  for (size_t i = 0; i < g_reg.size(); ++i) {
    if (g_reg[i].lo != lo) continue;
    g_reg.erase(g_reg.begin() + (ptrdiff_t)i);
    HIP_TRY(hipHostUnregister(const_cast<void*>(p)), "hipHostUnregister");
    return CG_OK;
  }
  return fail(CG_ERR_ARG, "cg_host_unregister: pointer was not registered");
}

int cg_host_register_advised(uint32_t contexts_per_node) { return cg::host_register_advised(contexts_per_node) ? 1 : 0; }

int cg_host_registered(const void* p, uint64_t len) {
  const uint64_t lo = (uint64_t)(uintptr_t)p, hi = lo + len;
  std::lock_guard<std::mutex> g(g_reg_mu);
  for (const HostRange& r : g_reg)
    if (lo >= r.lo && hi <= r.hi && hi >= lo) return 1;
  return 0;
}

static_assert(sizeof(cg_config) == 56, "cg_config is 56 bytes in ABI v2");
static_assert(sizeof(cg_item) == 32 && sizeof(cg_key) == 16 && sizeof(cg_txsig) == 24 && sizeof(cg_txsig_packed) == 12,
              "ABI struct sizes");

int cg_open(cg_ctx** out, const cg_config* cfg) {
  if (!out) return fail(CG_ERR_ARG, "cg_open: out is NULL");
  *out = nullptr;
  if (cfg && (cfg->reserved0 || cfg->reserved1))
    return fail(CG_ERR_ARG, "cg_open: cg_config.reserved must be 0 (ABI v2: 56-byte cg_config)");
  const uint64_t tab_budget = cfg && cfg->table_bytes_max ? cfg->table_bytes_max
                                                          : cgb::table_bytes_env(getenv("CG_TABLE_BYTES_MAX"));
  if (tab_budget && tab_budget < table_sets().back().bytes) {
    char m[160];
    snprintf(m, sizeof m, "cg_open: table_bytes_max %llu is below the smallest fixed-base tables (%llu bytes, radix 2^%u)",
             (unsigned long long)tab_budget, (unsigned long long)table_sets().back().bytes, table_sets().back().bits);
    return fail(CG_ERR_ARG, "%s", m);
  }
  if (cfg && (cfg->flags & ~(CG_FLAG_STAGE_TIMING | CG_FLAG_RSA | CG_FLAG_NO_KEY_CACHE))) return fail(CG_ERR_ARG, "cg_open: unknown cg_config.flags bits");
  int dev = cfg ? cfg->device : 0;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n), "hipGetDeviceCount");
  if (dev < 0 || dev >= n) return fail(CG_ERR_ARG, "cg_open: device ordinal out of range");
  HIP_TRY(hipSetDevice(dev), "hipSetDevice");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(CG_ERR_DEVICE, "cg_open: kernels are built for gfx950, device is %s", prop.gcnArchName);
  cg_ctx* c = new cg_ctx();
  c->device = dev;
  c->host_req = cfg ? cfg->host_threads : 0u;
  c->quota = cg::cpu_quota();
  if (cfg && cfg->chunk_items) {
    c->chunk = cfg->chunk_items;
    c->chunk_set = true;
  }
  if (cfg && (cfg->flags & CG_FLAG_STAGE_TIMING)) c->fork.timer = &c->timer;
  c->rsa = cfg && (cfg->flags & CG_FLAG_RSA);
  // the wide-table cache: on unless the flag or CG_KEY_CACHE=0 (A/B runs) says otherwise; read here,
  // per context. CG_TEST_WIDE_SLOTS / CG_TEST_KEY_CACHE_BITS (tests only): a pool of at most that
  // many slots, so that keys are evicted; an index of 2^bits home entries, so that keys collide.
  c->kc_on = !(cfg && (cfg->flags & CG_FLAG_NO_KEY_CACHE)) && env_flag("CG_KEY_CACHE", true);
  c->wide_slots_max = (uint32_t)std::min<uint64_t>(env_u64("CG_TEST_WIDE_SLOTS", cg::kKeyWideMax), cg::kKeyWideMax);
  c->kc_bits = (uint32_t)std::min<uint64_t>(env_u64("CG_TEST_KEY_CACHE_BITS", 32), 32);
  c->derive_force = (uint32_t)std::min<uint64_t>(env_u64("CG_TEST_DERIVE_FORCE_RETRIES", 0), CG_DERIVE_MAX_RETRIES + 1);
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return hip_fail(e, "hipStreamCreate");
  }
  // Side streams: plain, created right after the context's stream. HIP multiplexes plain streams
  // onto GPU_MAX_HW_QUEUES (4) hardware queues in creation order, so the context's stream (the one a
  // caller gets with hip_stream = NULL) and the three side streams sit on four distinct queues;
  // a caller stream created elsewhere may share one with a side stream, whose latency-bound table
  // chain (milliseconds) then runs ahead of that caller's hashes (profiles/r02/wide_v2).
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipStreamCreateWithFlags(&c->fork.side[k], hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork.start, hipEventDisableTiming);
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&c->fork.ready[k], hipEventDisableTiming);
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&c->fork.row0[k], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork.front, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork.planned, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork.ec_front_go, hipEventDisableTiming);
  for (int k = 0; k < 2 && e == hipSuccess; ++k)
    e = hipEventCreateWithFlags(&c->fork.ec_front_done[k], hipEventDisableTiming);
  // The copy streams on hardware queues of their own (an all-CU mask makes HIP back a stream with a
  // dedicated queue): multiplexed onto the four default queues, the copy stream shared one with a
  // side stream, and the first chunk's bytes landed only after that stream's table builds (the
  // chunk's fronts started right after k_ed_keyprep_tab in every timeline; with
  // GPU_MAX_HW_QUEUES=8 they started 3 ms earlier: profiles/r03/env_hwq). Plain streams only
  // where the device does not report its CUs.
  {
    hipDeviceProp_t prop;
    const bool own = hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0;
    std::vector<uint32_t> mask(own ? (prop.multiProcessorCount + 31) / 32 : 0, 0u);
    for (int cu = 0; own && cu < prop.multiProcessorCount; ++cu) mask[cu / 32] |= 1u << (cu % 32);
    for (hipStream_t* cs : {&c->copy, &c->copy2})
      if (e == hipSuccess)
        e = own ? hipExtStreamCreateWithCUMask(cs, (uint32_t)mask.size(), mask.data())
                : hipStreamCreateWithFlags(cs, hipStreamNonBlocking);
  }
  for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreate(&c->tev[k]);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->bridge, hipEventDisableTiming);
  c->bridged = env_flag("CG_STREAM_BRIDGE", true);
  int var = 0;
  if (e == hipSuccess) e = acquire_tables(c->device, c->stream, tab_budget, &c->btab, &var);
  if (e == hipSuccess) {
    c->eng = kVariants[var];
    c->tab_bytes = c->eng->btab_bytes();
    e = c->eng->upload_constants();  // per device: a table set built for another device uploaded there
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "side streams / upload_constants / fixed-base tables");
    cg_close(c);
    return rc;
  }
  c->counted = true;
  ++g_live_ctx;
  *out = c;
  return CG_OK;
}

// The signer store zeroed, then freed (cg_signers_clear, a reload, cg_close), after the device has
// finished whatever still reads it.
static void signers_drop(cg_ctx* c) {
  c->n_signers = 0;
  if (!c->signers.p) return;
  (void)hipDeviceSynchronize();
  (void)hipMemset(c->signers.p, 0, c->signers.cap);
  (void)hipDeviceSynchronize();
  c->signers.release();
}

static void ec_signers_drop(cg_ctx* c) {
  c->n_ec_signers = 0;
  if (!c->ec_signers.p) return;
  (void)hipDeviceSynchronize();
  (void)hipMemset(c->ec_signers.p, 0, c->ec_signers.cap);
  (void)hipDeviceSynchronize();
  c->ec_signers.release();
}

static void rsa_signers_drop(cg_ctx* c) {
  c->n_rsa_signers = 0;
  if (!c->rsa_signers.p) return;
  (void)hipDeviceSynchronize();
  (void)hipMemset(c->rsa_signers.p, 0, c->rsa_signers.cap);
  (void)hipDeviceSynchronize();
  c->rsa_signers.release();
}

void cg_close(cg_ctx* c) {
  if (!c) return;
  if (c->counted) --g_live_ctx;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  signers_drop(c);
  ec_signers_drop(c);
  rsa_signers_drop(c);
  c->signws.release();
  c->signecws.release();
  c->signrsaws.release();
  c->derivews.release();
  c->keyprep.release();
  c->itemws.release();
  c->wide.release();
  c->kcache.release();
  if (c->btab) release_tables(c->device, c->btab);
  c->btab = nullptr;
  c->keys.release();
  c->items.release();
  c->arena.release();
  c->status.release();
  c->aux0.release();
  c->aux1.release();
  c->aux2.release();
  for (DevBuf* b : {&c->txitems, &c->msgs, &c->tmpls, &c->h_txs, &c->h_comps, &c->h_sigs, &c->h_ids, &c->h_txst,
                    &c->ftxws, &c->bfws, &c->bfin, &c->bfio, &c->sig12ws, &c->rsakeys, &c->rsalist, &c->txvws, &c->txvio})
    b->release();
  for (int k = 0; k < 3; ++k) {
    if (c->fork.side[k]) {
      hipStreamSynchronize(c->fork.side[k]);
      hipStreamDestroy(c->fork.side[k]);
    }
    if (c->fork.ready[k]) hipEventDestroy(c->fork.ready[k]);
    if (c->fork.row0[k]) hipEventDestroy(c->fork.row0[k]);
  }
  if (c->fork.start) hipEventDestroy(c->fork.start);
  if (c->fork.front) hipEventDestroy(c->fork.front);
  if (c->fork.planned) hipEventDestroy(c->fork.planned);
  if (c->fork.ec_front_go) hipEventDestroy(c->fork.ec_front_go);
  for (int k = 0; k < 2; ++k)
    if (c->fork.ec_front_done[k]) hipEventDestroy(c->fork.ec_front_done[k]);
  for (hipStream_t* cs : {&c->copy, &c->copy2})
    if (*cs) {
      hipStreamSynchronize(*cs);
      hipStreamDestroy(*cs);
    }
  for (hipEvent_t e : c->segt) hipEventDestroy(e);
  for (hipEvent_t e : c->segtab) hipEventDestroy(e);
  for (hipEvent_t e : c->fbt) hipEventDestroy(e);
  for (hipEvent_t e : c->backt)
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : c->seg) hipEventDestroy(e);
  for (int k = 0; k < 4; ++k)
    if (c->tev[k]) hipEventDestroy(c->tev[k]);
  if (c->done) hipEventDestroy(c->done);
  if (c->bridge) hipEventDestroy(c->bridge);
  for (auto* v : {&c->timer.recs, &c->timer.spare})
    for (auto& r : *v) {
      hipEventDestroy(r.a);
      hipEventDestroy(r.b);
    }
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

uint64_t cg_table_bytes(uint32_t fixed_base_bits) {
  for (const cgb::TableSet& t : table_sets())
    if (t.bits == fixed_base_bits) return t.bytes;
  return 0;
}

uint32_t cg_table_choice(uint64_t table_bytes_max, uint64_t device_free) {
  const std::vector<cgb::TableSet> sets = table_sets();
  const int k = cgb::pick_tables(sets.data(), (int)sets.size(), table_bytes_max, device_free, -1);
  return k < 0 ? 0u : sets[k].bits;
}

uint32_t cg_rsa_key_bits(const uint8_t* spki, uint32_t len) {
  if (!spki || len == 0 || len > 0xffffu) return 0;
  std::vector<uint32_t> buf((len + 3) / 4 + 1, 0u);  // aligned and padded: the decode reads dwords
  memcpy(buf.data(), spki, len);
  RsaKeyView v;
  const uint64_t lr = ((uint64_t)len + 3) & ~(uint64_t)3;
  return rsa_key_decode(v, (const uint8_t*)buf.data(), lr, 0, len) ? v.bits : 0u;
}

int cg_context_info(const cg_ctx* c, cg_info* out) {
  if (!c || !out) return fail(CG_ERR_ARG, "cg_context_info: NULL argument");
  memset(out, 0, sizeof *out);
  out->device = c->device;
  out->fixed_base_bits = c->eng ? c->eng->fixed_base_bits : 0u;
  out->table_bytes = c->tab_bytes;
  out->host_threads = cg::host_threads_for(c->host_req, cg::host_threads_env(), c->quota, g_live_ctx.load());
  out->chunk_items = c->chunk;
  return CG_OK;
}

int cg_stage_times(cg_ctx* c, double* ms_out, uint32_t* launches_out, uint32_t n) {
  if (!c || (n && (!ms_out || !launches_out))) return fail(CG_ERR_ARG, "cg_stage_times: NULL argument");
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_stage_times")) return rc;
  const uint32_t m = n < CG_STAGES ? n : CG_STAGES;
  for (uint32_t k = 0; k < m; ++k) {
    ms_out[k] = 0;
    launches_out[k] = 0;
  }
  int rc = CG_OK;
  for (auto& r : c->timer.recs) {
    float ms = 0;
    if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) rc = CG_ERR_DEVICE;
    if ((uint32_t)r.stage < m) {
      ms_out[r.stage] += ms;
      launches_out[r.stage] += 1;
    }
    c->timer.spare.push_back(r);
  }
  c->timer.recs.clear();
  return rc == CG_OK ? (int)m : fail(rc, "cg_stage_times: event wait failed");
}

int cg_reserve(cg_ctx* c, uint32_t max_keys, uint64_t max_items) {
  if (!c) return fail(CG_ERR_ARG, "cg_reserve: ctx is NULL");
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_reserve")) return rc;
  HIP_TRY(ensure_ws(c, max_keys, chunk_of(c, max_items), max_items), "hipMalloc(workspace)");
  return CG_OK;
}

int cg_key_cache_stats(cg_ctx* c, cg_key_cache_info* out) {
  if (!c || !out) return fail(CG_ERR_ARG, "cg_key_cache_stats: NULL argument");
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_key_cache_stats")) return rc;
  memset(out, 0, sizeof *out);
  out->enabled = c->kc_on ? 1u : 0u;
  out->slots = c->wide_slots;
  if (c->done_rec) HIP_TRY(hipEventSynchronize(c->done), "hipEventSynchronize");
  HIP_TRY(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  if (!c->kc_on || !c->kcache.p || c->kc_dirty) return CG_OK;  // no call has used the cache since it was emptied
  uint32_t ctr[16];  // keyws.h KeyCache: 8 counters per pool head the buffer
  HIP_TRY(hipMemcpy(ctr, c->kcache.p, sizeof ctr, hipMemcpyDeviceToHost), "hipMemcpy(key cache counters)");
  for (int q = 0; q < 2; ++q) {
    out->hits[q] = ctr[8 * q + 0];
    out->built[q] = ctr[8 * q + 1];
    out->evicted[q] = ctr[8 * q + 2];
    out->fell_back[q] = ctr[8 * q + 3];
  }
  return CG_OK;
}

int cg_verify_batch_device(cg_ctx* c, const cg_key* d_keys, uint32_t n_keys, const cg_item* d_items,
                           uint64_t n_items, const uint8_t* d_arena, uint64_t arena_len, uint32_t mode,
                           uint8_t* d_status, void* hip_stream) {
  if (!c) return fail(CG_ERR_ARG, "cg_verify_batch_device: ctx is NULL");
  const cg::VerifyReq r = {d_keys, n_keys, d_items, n_items, d_arena, arena_len, mode, d_status};
  if (const int a = batch_args("cg_verify_batch_device", r, false)) return a;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_verify_batch_device")) return rc;
  HIP_TRY(ensure_ws(c, n_keys, chunk_of(c, n_items), n_items), "hipMalloc(workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(launch_chunked(c, r, cg::equal_bounds(n_items, chunk_of(c, n_items)), call.stream(), ChunkOpts{}),
          "launch_verify");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

int cg_prepare_keys_device(cg_ctx* c, const cg_key* d_keys, uint32_t n_keys, const uint8_t* d_arena,
                           uint64_t arena_len, void* hip_stream) {
  if (!c) return fail(CG_ERR_ARG, "cg_prepare_keys_device: ctx is NULL");
  if (n_keys && !d_keys) return fail(CG_ERR_ARG, "cg_prepare_keys_device: keys is NULL");
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_prepare_keys_device")) return rc;
  HIP_TRY(ensure_all({{&c->keyprep, c->eng->keyprep_bytes(n_keys)}}), "hipMalloc(keyprep)");
  HIP_TRY(ensure_rsa(c, n_keys, 0), "hipMalloc(RSA workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  hipStream_t s = call.stream();
  const cg::VerifyReq r = {d_keys, n_keys, nullptr, 0, d_arena, arena_len, CG_MODE_DOVERIFY, nullptr};  // no items yet
  // the call ends with the main stream behind every family's table builds (launch_schedule.h
  // prepare_keys): `done` then covers the side streams' reads of the caller's key bytes
  const std::vector<uint64_t> none = {0};
  const ChunkOpts o;
  CallEng keys = {c, r, s, nullptr, none, o};
  HIP_TRY(cgs::prepare_keys(keys, n_keys != 0), keys.where);
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

int cg_verify_items_device(cg_ctx* c, const cg_key* d_keys, uint32_t n_keys, const cg_item* d_items,
                           uint64_t n_items, const uint8_t* d_arena, uint64_t arena_len, uint32_t mode,
                           uint8_t* d_status, void* hip_stream) {
  if (!c) return fail(CG_ERR_ARG, "cg_verify_items_device: ctx is NULL");
  const cg::VerifyReq r = {d_keys, n_keys, d_items, n_items, d_arena, arena_len, mode, d_status};
  if (const int a = batch_args("cg_verify_items_device", r, false)) return a;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->keyprep.cap < c->eng->keyprep_bytes(n_keys))
    return fail(CG_ERR_ARG, "cg_verify_items_device: keys were not prepared (call cg_prepare_keys_device)");
  if (c->rsa && c->rsakeys.cap < cg::rsa_keys_bytes(n_keys))
    return fail(CG_ERR_ARG, "cg_verify_items_device: RSA keys were not prepared (call cg_prepare_keys_device)");
  if (const int rc = enter(c, "cg_verify_items_device")) return rc;
  HIP_TRY(ensure_ws(c, n_keys, chunk_of(c, n_items)), "hipMalloc(item workspace)");
  HIP_TRY(ensure_rsa(c, n_keys, n_items), "hipMalloc(RSA workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  hipStream_t s = call.stream();
  const uint64_t per = chunk_of(c, n_items);
  std::vector<uint64_t> bounds = {0};  // chunks of `per`, the last one shorter
  for (uint64_t f = 0; f < n_items; f += per) bounds.push_back(per < n_items - f ? f + per : n_items);
  const ChunkOpts o;
  CallEng items = {c, r, s, nullptr, bounds, o};
  items.closes_cache = false;
  HIP_TRY(cgs::verify_items(items, (unsigned)(bounds.size() - 1)), items.where);
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

int cg_verify_batch(cg_ctx* c, const cg_key* keys, uint32_t n_keys, const cg_item* items, uint64_t n_items,
                    const uint8_t* arena, uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                    cg_stats* stats) {
  if (!c) return fail(CG_ERR_ARG, "cg_verify_batch: ctx is NULL");
  const cg::VerifyReq h = {keys, n_keys, items, n_items, arena, arena_len, mode, status_out};
  if (const int a = batch_args("cg_verify_batch", h, true)) return a;
  if (n_items) memset(status_out, CG_NOT_RUN, n_items);
  if (n_items == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  const int rc = verify_host_locked(c, h, stats);
  if (rc != CG_OK) memset(status_out, CG_NOT_RUN, n_items);
  return rc;
}

int cg_sha256_batch_device(cg_ctx* c, const cg_span* d_spans, uint64_t n, const uint8_t* d_arena,
                           uint64_t arena_len, uint8_t* d_digests, void* hip_stream) {
  if (!c) return fail(CG_ERR_ARG, "cg_sha256_batch_device: ctx is NULL");
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_sha256_batch_device")) return rc;
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(cg::launch_sha256(d_spans, n, d_arena, arena_len, d_digests, call.stream()), "launch_sha256");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

static int hash_batch(cg_ctx* c, const cg_span* spans, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                      uint8_t* out, int which) {
  if (!c) return fail(CG_ERR_ARG, "hash batch: ctx is NULL");
  if (n && (!spans || !out)) return fail(CG_ERR_ARG, "hash batch: NULL buffer");
  if (n == 0) return CG_OK;
  const size_t dlen = which == 256 ? 32 : 64;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, which == 256 ? "cg_sha256_batch" : "cg_sha512_batch")) return rc;
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->items, spans, sizeof(cg_span) * n, s), "H2D spans");
  HIP_TRY(stage(c->arena, arena, arena_len, s, arena_room(arena_len)), "H2D arena");
  HIP_TRY(c->aux0.ensure(dlen * n), "hipMalloc(digests)");
  HIP_TRY((which == 256 ? cg::launch_sha256 : cg::launch_sha512)((const cg_span*)c->items.p, n, (const uint8_t*)c->arena.p,
                                                                 arena_len, (uint8_t*)c->aux0.p, s), "launch_sha");
  HIP_TRY(hipMemcpyAsync(out, c->aux0.p, dlen * n, hipMemcpyDeviceToHost, s), "D2H digests");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

int cg_sha256_batch(cg_ctx* c, const cg_span* spans, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                    uint8_t* out) {
  return hash_batch(c, spans, n, arena, arena_len, out, 256);
}
int cg_sha512_batch(cg_ctx* c, const cg_span* spans, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                    uint8_t* out) {
  return hash_batch(c, spans, n, arena, arena_len, out, 512);
}

int cg_tx_ids_device(cg_ctx* c, const cg_tx* d_txs, uint64_t n_tx, const cg_component* d_comps, uint64_t n_comps,
                     const uint8_t* d_arena, uint64_t arena_len, uint8_t* d_ids, uint8_t* d_status,
                     void* hip_stream) {
  if (!c) return fail(CG_ERR_ARG, "cg_tx_ids_device: ctx is NULL");
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_tx_ids_device")) return rc;
  HIP_TRY(ensure_all({{&c->aux2, cg::tx_ws_bytes(n_comps)}}), "hipMalloc(leaf ws)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(cg::launch_tx_ids(d_txs, n_tx, d_comps, n_comps, d_arena, arena_len, d_ids, d_status,
                            (uint8_t*)c->aux2.p, call.stream()), "launch_tx_ids");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

int cg_tx_ids(cg_ctx* c, const cg_tx* txs, uint64_t n_tx, const cg_component* comps, uint64_t n_comps,
              const uint8_t* arena, uint64_t arena_len, uint8_t* ids_out, uint8_t* status_out) {
  if (!c) return fail(CG_ERR_ARG, "cg_tx_ids: ctx is NULL");
  if (n_tx && (!txs || !ids_out || !status_out)) return fail(CG_ERR_ARG, "cg_tx_ids: NULL buffer");
  if (n_tx == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_tx_ids")) return rc;
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->keys, txs, sizeof(cg_tx) * n_tx, s), "H2D txs");
  HIP_TRY(stage(c->items, comps, sizeof(cg_component) * n_comps, s), "H2D comps");
  HIP_TRY(stage(c->arena, arena, arena_len, s, arena_room(arena_len)), "H2D arena");
  HIP_TRY(c->aux0.ensure(32 * n_tx), "hipMalloc(ids)");
  HIP_TRY(c->status.ensure(n_tx), "hipMalloc(status)");
  HIP_TRY(c->aux2.ensure(cg::tx_ws_bytes(n_comps)), "hipMalloc(leaf ws)");
  HIP_TRY(cg::launch_tx_ids((const cg_tx*)c->keys.p, n_tx, (const cg_component*)c->items.p, n_comps,
                            (const uint8_t*)c->arena.p, arena_len, (uint8_t*)c->aux0.p, (uint8_t*)c->status.p,
                            (uint8_t*)c->aux2.p, s), "launch_tx_ids");
  HIP_TRY(hipMemcpyAsync(ids_out, c->aux0.p, 32 * n_tx, hipMemcpyDeviceToHost, s), "D2H ids");
  HIP_TRY(hipMemcpyAsync(status_out, c->status.p, n_tx, hipMemcpyDeviceToHost, s), "D2H status");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

int cg_merkle_roots(cg_ctx* c, const uint8_t* leaves, const uint64_t* first, const uint32_t* count, uint64_t n,
                    uint8_t* roots_out, uint8_t* status_out) {
  if (!c) return fail(CG_ERR_ARG, "cg_merkle_roots: ctx is NULL");
  if (n && (!first || !count || !roots_out || !status_out)) return fail(CG_ERR_ARG, "cg_merkle_roots: NULL buffer");
  if (n == 0) return CG_OK;
  uint64_t total = 0, ws = 0;
  std::vector<uint64_t> wsoff(n);
  for (uint64_t j = 0; j < n; ++j) {
    if (first[j] + count[j] > total) total = first[j] + count[j];
    wsoff[j] = ws;
    ws += count[j];
  }
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_merkle_roots")) return rc;
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->arena, leaves, 32 * total, s), "H2D leaves");
  HIP_TRY(stage(c->keys, first, 8 * n, s), "H2D first");
  HIP_TRY(stage(c->items, count, 4 * n, s), "H2D count");
  HIP_TRY(stage(c->aux2, wsoff.data(), 8 * n, s), "H2D wsoff");
  HIP_TRY(c->aux0.ensure(32 * n), "hipMalloc(roots)");
  HIP_TRY(c->status.ensure(n), "hipMalloc(status)");
  HIP_TRY(c->aux1.ensure(32 * (ws ? ws : 1)), "hipMalloc(ws)");
  HIP_TRY(cg::launch_merkle_roots((const uint8_t*)c->arena.p, (const uint64_t*)c->keys.p, (const uint32_t*)c->items.p,
                                  n, (uint8_t*)c->aux0.p, (uint8_t*)c->status.p, (uint8_t*)c->aux1.p,
                                  (const uint64_t*)c->aux2.p, s),
          "launch_merkle_roots");
  HIP_TRY(hipMemcpyAsync(roots_out, c->aux0.p, 32 * n, hipMemcpyDeviceToHost, s), "D2H roots");
  HIP_TRY(hipMemcpyAsync(status_out, c->status.p, n, hipMemcpyDeviceToHost, s), "D2H status");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

// The spliced-message slot of a template set: the longest prefix || id || suffix, 16-aligned.
static uint64_t tmpl_slot(const cg_signable_tmpl* tmpls, uint32_t n_tmpls) {
  uint64_t maxlen = 0;
  for (uint32_t k = 0; k < n_tmpls; ++k) {
    const uint64_t l = (uint64_t)tmpls[k].prefix_len + 32u + tmpls[k].suffix_len;
    if (l > maxlen) maxlen = l;
  }
  const uint64_t slot = (maxlen + 15) & ~(uint64_t)15;
  return slot ? slot : 16;
}

// One cg_verify_transactions call: the caller's tables (all in host memory, or all in HBM but the
// templates) and the three result buffers.
struct TxnReq {
  const cg_tx* txs;
  uint64_t n_tx;
  const cg_component* comps;
  uint64_t n_comps;
  const cg_key* keys;
  uint32_t n_keys;
  const cg_txsig* sigs;
  uint64_t n_sigs;
  const cg_signable_tmpl* tmpls;  // host memory in every form
  uint32_t n_tmpls;
  const uint8_t* arena;
  uint64_t arena_len;
  uint32_t mode;
  uint8_t *ids, *tx_status, *sig_status;
};
// The argument checks of the family, after the ctx / pool check (host: the forms over host buffers)
static int txn_args(const char* fn, const TxnReq& q, bool host) {
  if (q.n_tx && (!q.txs || !q.ids || !q.tx_status)) return fail(CG_ERR_ARG, "%s: NULL tx buffer", fn);
  if (q.n_sigs && (!q.sigs || !q.sig_status)) return fail(CG_ERR_ARG, "%s: NULL sig buffer", fn);
  if (host && q.n_comps && !q.comps) return fail(CG_ERR_ARG, "%s: comps is NULL", fn);
  if (host && q.n_keys && !q.keys) return fail(CG_ERR_ARG, "%s: keys is NULL", fn);
  if (q.n_tmpls && !q.tmpls) return fail(CG_ERR_ARG, "%s: templates is NULL", fn);
  if (host && q.arena_len && !q.arena) return fail(CG_ERR_ARG, "%s: arena is NULL", fn);
  if (q.mode > CG_MODE_ISVALID) return fail(CG_ERR_ARG, "%s: bad mode", fn);
  return CG_OK;
}

// The launches of cg_verify_transactions(_device) on `s` over the device tables `d`, inside the
// caller's open call (the ctx lock held): grows the workspace (waiting for the device), then ids, verify
// items and the chunked verify.
static int verify_transactions_locked(cg_ctx* c, const TxnReq& d, hipStream_t s) {
  const uint64_t slot = tmpl_slot(d.tmpls, d.n_tmpls), msgs_len = cg::tx_msgs_head(d.n_tmpls, slot);
  HIP_TRY(ensure_all({{&c->aux2, cg::tx_ws_bytes(d.n_comps)},
                      {&c->txitems, sizeof(cg_item) * (d.n_sigs ? d.n_sigs : 1)},
                      {&c->msgs, msgs_len ? msgs_len : 16},
                      {&c->tmpls, sizeof(cg_signable_tmpl) * (d.n_tmpls ? d.n_tmpls : 1)}}),
          "hipMalloc(transaction workspace)");
  HIP_TRY(ensure_ws(c, d.n_keys, chunk_of(c, d.n_sigs), d.n_sigs), "hipMalloc(workspace)");
  if (d.n_tmpls)
    HIP_TRY(hipMemcpyAsync(c->tmpls.p, d.tmpls, sizeof(cg_signable_tmpl) * d.n_tmpls, hipMemcpyHostToDevice, s),
            "H2D templates");
  HIP_TRY(cg::launch_tx_ids(d.txs, d.n_tx, d.comps, d.n_comps, d.arena, d.arena_len, d.ids, d.tx_status,
                            (uint8_t*)c->aux2.p, s), "launch_tx_ids");
  if (d.n_sigs) {
    HIP_TRY(cg::launch_tx_sig_items(d.sigs, d.n_sigs, (const cg_signable_tmpl*)c->tmpls.p, d.n_tmpls, d.tx_status,
                                    d.n_tx, d.ids, d.arena, d.arena_len, slot, (cg_item*)c->txitems.p,
                                    (uint8_t*)c->msgs.p, s),
            "launch_tx_sig_items");
    const cg::VerifyReq r = {d.keys, d.n_keys, (const cg_item*)c->txitems.p, d.n_sigs, d.arena, d.arena_len, d.mode,
                             d.sig_status, (const uint8_t*)c->msgs.p, msgs_len};
    HIP_TRY(launch_chunked(c, r, cg::equal_bounds(d.n_sigs, chunk_of(c, d.n_sigs)), s, ChunkOpts{}), "launch_verify");
  }
  return CG_OK;
}

int cg_verify_transactions_device(cg_ctx* c, const cg_tx* d_txs, uint64_t n_tx, const cg_component* d_comps,
                                  uint64_t n_comps, const cg_key* d_keys, uint32_t n_keys, const cg_txsig* d_sigs,
                                  uint64_t n_sigs, const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                                  const uint8_t* d_arena, uint64_t arena_len, uint32_t mode, uint8_t* d_ids,
                                  uint8_t* d_tx_status, uint8_t* d_sig_status, void* hip_stream) {
  if (!c) return fail(CG_ERR_ARG, "cg_verify_transactions_device: ctx is NULL");
  const TxnReq d = {d_txs, n_tx,  d_comps,   n_comps, d_keys, n_keys, d_sigs,      n_sigs,
                    tmpls, n_tmpls, d_arena, arena_len, mode, d_ids,  d_tx_status, d_sig_status};
  if (const int a = txn_args("cg_verify_transactions_device", d, false)) return a;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_verify_transactions_device")) return rc;
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  if (const int rc = verify_transactions_locked(c, d, call.stream())) return rc;
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

// cg_verify_transactions with the arguments checked and the ctx lock held (also a cg_pool slot's call)
static int verify_transactions_host_locked(cg_ctx* c, const TxnReq& h) {
  if (const int rc = enter(c, "cg_verify_transactions")) return rc;
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->h_txs, h.txs, sizeof(cg_tx) * h.n_tx, s), "H2D txs");
  HIP_TRY(stage(c->h_comps, h.comps, sizeof(cg_component) * h.n_comps, s), "H2D comps");
  HIP_TRY(stage(c->keys, h.keys, sizeof(cg_key) * h.n_keys, s), "H2D keys");
  HIP_TRY(stage(c->h_sigs, h.sigs, sizeof(cg_txsig) * h.n_sigs, s), "H2D sigs");
  HIP_TRY(stage(c->arena, h.arena, h.arena_len, s, arena_room(h.arena_len)), "H2D arena");
  HIP_TRY(c->h_ids.ensure(32 * (h.n_tx ? h.n_tx : 1)), "hipMalloc(ids)");
  HIP_TRY(c->h_txst.ensure(h.n_tx ? h.n_tx : 1), "hipMalloc(tx status)");
  HIP_TRY(c->status.ensure(h.n_sigs ? h.n_sigs : 1), "hipMalloc(sig status)");
  TxnReq d = h;  // the staged copies
  d.txs = (const cg_tx*)c->h_txs.p;
  d.comps = (const cg_component*)c->h_comps.p;
  d.keys = (const cg_key*)c->keys.p;
  d.sigs = (const cg_txsig*)c->h_sigs.p;
  d.arena = (const uint8_t*)c->arena.p;
  d.ids = (uint8_t*)c->h_ids.p;
  d.tx_status = (uint8_t*)c->h_txst.p;
  d.sig_status = (uint8_t*)c->status.p;
  if (const int rc = verify_transactions_locked(c, d, s)) return rc;
  if (h.n_tx) {
    HIP_TRY(hipMemcpyAsync(h.ids, d.ids, 32 * h.n_tx, hipMemcpyDeviceToHost, s), "D2H ids");
    HIP_TRY(hipMemcpyAsync(h.tx_status, d.tx_status, h.n_tx, hipMemcpyDeviceToHost, s), "D2H tx status");
  }
  if (h.n_sigs) HIP_TRY(hipMemcpyAsync(h.sig_status, d.sig_status, h.n_sigs, hipMemcpyDeviceToHost, s), "D2H sig status");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

int cg_verify_transactions(cg_ctx* c, const cg_tx* txs, uint64_t n_tx, const cg_component* comps, uint64_t n_comps,
                           const cg_key* keys, uint32_t n_keys, const cg_txsig* sigs, uint64_t n_sigs,
                           const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                           uint64_t arena_len, uint32_t mode, uint8_t* ids_out, uint8_t* tx_status_out,
                           uint8_t* sig_status_out) {
  if (!c) return fail(CG_ERR_ARG, "cg_verify_transactions: ctx is NULL");
  const TxnReq h = {txs,   n_tx,    comps, n_comps,   keys, n_keys,  sigs,          n_sigs,
                    tmpls, n_tmpls, arena, arena_len, mode, ids_out, tx_status_out, sig_status_out};
  if (const int a = txn_args("cg_verify_transactions", h, true)) return a;
  for (uint64_t i = 0; i < n_sigs; ++i) sig_status_out[i] = CG_NOT_RUN;
  if (n_tx == 0 && n_sigs == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return verify_transactions_host_locked(c, h);
}

// ---------------------------------------------------------------- signatures over known tx ids
// Verify items, spliced messages and the template table of n_sigs signatures (waits for the device
// when a buffer grows).
static hipError_t ensure_txsig_ws(cg_ctx* c, uint64_t n_sigs, uint32_t n_tmpls, uint64_t slot) {
  return ensure_all({{&c->txitems, sizeof(cg_item) * (n_sigs ? n_sigs : 1)},
                     {&c->msgs, cg::tx_msgs_head(n_tmpls, slot)},
                     {&c->tmpls, sizeof(cg_signable_tmpl) * (n_tmpls ? n_tmpls : 1)}});
}

// One tx-signature call (cg_verify_tx_signatures and its packed, device, pool and required-signatures
// forms): the caller's tables, all in host memory or all in HBM but the templates (host memory in every
// form). The 12-byte table's signatures are a dense stream of sig_bytes_len bytes: a buffer of its own
// in the host forms (sig_bytes), a stretch of the arena in the device forms (sig_bytes_off). A pool
// shard is a copy with the table, the status bytes and the stream narrowed.
struct TxsigReq {
  const cg_key* keys;
  uint32_t n_keys;
  const uint8_t* ids;
  uint64_t n_ids;
  cg::SigTable sigs;
  uint64_t n_sigs;
  const cg_signable_tmpl* tmpls;
  uint32_t n_tmpls;
  const uint8_t* arena;
  uint64_t arena_len;
  uint32_t mode;
  uint8_t* status;
  const uint8_t* sig_bytes = nullptr;
  uint64_t sig_bytes_off = 0, sig_bytes_len = 0;
};

// How launch_txsig schedules a call: the chunk bounds, where the key-use counts come from (sampled
// from the signature table on the device, or the host's exact counts), `ready` (the host form: run
// before chunk k's items are made, it lands the chunk's signature-table slice and bytes), and for the
// 12-byte table where the signatures start in the stream: chunk k's first one at (*chunk_base)[k] (host
// form: the host sums the lengths as it scans each chunk) or every 256-record block's offset
// precomputed in d_bases (device form).
struct TxsigSched {
  const std::vector<uint64_t>& bounds;
  cg::KeyUses uses;
  const std::function<hipError_t(uint64_t, uint64_t, uint64_t)>* ready = nullptr;
  const std::vector<uint64_t>* chunk_base = nullptr;
  const uint64_t* d_bases = nullptr;
};
// Templates to the device (midstates + images), then the chunked verify over the device tables `d`:
// each chunk's verify items and spliced SignableData made just before its front.
static hipError_t launch_txsig(cg_ctx* c, const TxsigReq& d, uint64_t slot, const TxsigSched& p, hipStream_t s) {
  if (d.n_sigs == 0) return hipSuccess;
  hipError_t e = hipSuccess;
  const cg_signable_tmpl* dt = (const cg_signable_tmpl*)c->tmpls.p;
  if (d.n_tmpls) e = hipMemcpyAsync(c->tmpls.p, d.tmpls, sizeof(cg_signable_tmpl) * d.n_tmpls, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = cg::launch_tx_sig_templates(dt, d.n_tmpls, d.arena, d.arena_len, slot, d.ids, d.n_ids, (uint8_t*)c->msgs.p, s);
  const std::function<hipError_t(uint64_t, uint64_t, uint64_t)> prepare = [&](uint64_t k, uint64_t first,
                                                                               uint64_t cnt) {
    hipError_t r = p.ready ? (*p.ready)(k, first, cnt) : hipSuccess;
    if (r == hipSuccess && d.sigs.packed())
      r = cg::launch_tx_sig12_range((const cg_txsig_packed*)d.sigs.p, first, cnt, d.sig_bytes_off, d.sig_bytes_len,
                                    p.chunk_base ? (*p.chunk_base)[k] : 0, p.d_bases, dt, d.n_tmpls, d.n_ids,
                                    d.arena_len, (cg_item*)c->txitems.p, c->sig12ws.p, s);
    else if (r == hipSuccess)
      r = cg::launch_tx_sig_range((const cg_txsig*)d.sigs.p, first, cnt, dt, d.n_tmpls, nullptr, d.n_ids, d.ids,
                                  d.arena_len, slot, (cg_item*)c->txitems.p, (uint8_t*)c->msgs.p, s);
    return r;
  };
  const cg::VerifyReq r = {d.keys, d.n_keys, (const cg_item*)c->txitems.p, d.n_sigs, d.arena, d.arena_len, d.mode,
                           d.status, (const uint8_t*)c->msgs.p, cg::tx_msgs_head(d.n_tmpls, slot)};
  if (e == hipSuccess) e = launch_chunked(c, r, p.bounds, s, ChunkOpts{&prepare, &p.uses, p.ready != nullptr});
  return e;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// CG_HOST_TRACE=1: per-chunk host timings of a host tx-signature call to stderr (extent scan, each
// copy call's return) and, after the call, where the device was when (timing events behind each
// chunk's copy, front and back). Off: every member returns at once and records nothing.
struct HostTrace {
  cg_ctx* c;
  const std::chrono::steady_clock::time_point t0;
  const bool on;
  std::vector<double> ht;  // per chunk: the scan's start, the scan, the table slice's copy call (ms)

  double ms() const { return on ? ms_since(t0) : 0; }
  // the events launch_chunked and the feed record for nch chunks
  hipError_t begin(uint64_t nch) {
    c->htrace = on;
    if (!on) return hipSuccess;
    hipError_t e = hipSuccess;
    for (int q = 0; q < 2 && e == hipSuccess; ++q)
      if (!c->backt[q]) e = hipEventCreate(&c->backt[q]);
    while (e == hipSuccess && c->fbt.size() < 3 * nch) {
      hipEvent_t ev;
      e = hipEventCreate(&ev);
      if (e == hipSuccess) c->fbt.push_back(ev);
    }
    c->fbh.assign(nch, 0.0);
    ht.assign(3 * nch, 0.0);
    return e;
  }
  // chunk k's scan ran from h0 to h1, then its table slice's copy call until now
  void table_staged(uint64_t k, double h0, double h1) {
    if (!on) return;
    ht[3 * k] = h0;
    ht[3 * k + 1] = h1 - h0;
    ht[3 * k + 2] = ms() - h1;
  }
  // chunk k's id copies were issued from h2 to h3, then its signature bytes (ek) until now; a timing
  // event behind them on the copy stream
  hipError_t bytes_staged(uint64_t k, hipStream_t cs, double h2, double h3, double table_mb, const Extent& ek) {
    if (!on) return hipSuccess;
    hipError_t e = hipSuccess;
    while (c->segt.size() <= k) {
      hipEvent_t ev;
      if (hipEventCreate(&ev) != hipSuccess) break;
      c->segt.push_back(ev);
    }
    if (c->segt.size() > k) e = hipEventRecord(c->segt[k], cs);
    fprintf(stderr, "[cg host] chunk %llu at %.3f: scan %.3f sigs %.3f (%.1f MB) ids %.3f arena %.3f (%.1f MB) ms\n",
            (unsigned long long)k, ht[3 * k], ht[3 * k + 1], ht[3 * k + 2], table_mb, h3 - h2, ms() - h3,
            ek.empty() ? 0.0 : (ek.hi - ek.lo) / 1e6);
    return e;
  }
  // the main stream reaches chunk k's front (its bytes have landed)
  hipError_t front_reached(uint64_t k, hipStream_t s) {
    if (!on || 3 * k >= c->fbt.size()) return hipSuccess;
    c->fbh[k] = ms();
    return hipEventRecord(c->fbt[3 * k], s);
  }
  // after the call's stream is drained: enqueued at h_enq
  void report(uint64_t nch, double h_enq) {
    if (!on) return;
    fprintf(stderr, "[cg host] enqueued at %.3f, done at %.3f ms; copies landed (device ms after the call's first event):",
            h_enq, ms());
    for (uint64_t k = 0; k < nch && k < c->segt.size(); ++k) {
      float t = 0;
      hipEventElapsedTime(&t, c->tev[0], c->segt[k]);
      fprintf(stderr, " %.3f", t);
    }
    float t = 0, f0 = 0, tb = 0;
    hipEventElapsedTime(&t, c->tev[0], c->tev[2]);
    hipEventElapsedTime(&f0, c->tev[0], c->backt[0]);
    hipEventElapsedTime(&tb, c->tev[0], c->backt[1]);
    fprintf(stderr, "; chunk 0 front done %.3f, tables built %.3f, verify done %.3f\n", f0, tb, t);
    for (uint64_t k = 0; k < nch && 3 * k + 2 < c->fbt.size(); ++k) {
      float fs = 0, be = 0, bj = 0;
      hipEventElapsedTime(&fs, c->tev[0], c->fbt[3 * k]);
      hipEventElapsedTime(&bj, c->tev[0], c->fbt[3 * k + 2]);
      hipEventElapsedTime(&be, c->tev[0], c->fbt[3 * k + 1]);
      fprintf(stderr, "[cg host] chunk %llu: front enqueued (host) %.3f, front reached (device) %.3f, back's "
              "kernels done %.3f, joins done %.3f\n", (unsigned long long)k, c->fbh[k], fs, bj, be);
    }
  }
};

// The per-chunk feed of a host tx-signature call, all on the copy stream. Chunk k's copies go in two
// parts around its front: `before` (launch_chunked's prepare hook) scans the chunk's extents and
// stages its signature-table slice, all its plan needs (segtab[k]); `mid` (the hook
// launch_items_front runs between the plan and the hashes) stages the ids it references that are
// not yet resident (a caller that lists each transaction's signatures together ships each id once,
// with its first chunk) and its signature bytes, what its hashes need (seg[k]). So the plan waits
// only for the table slice and overlaps the byte copy. Round 5 headline A/B against waiting for
// the whole chunk before its front, 10 interleaved pairs: 327.7 -> 330.5 M sigs/s, 7 of 10 pairs
// faster (profiles/r05/split).
// Measured and not kept: the next chunk's extent scan on the pool from a helper thread while this
// chunk's copies stage (round 4 neutral to -1%, the copies' landing times did not move,
// profiles/r04/ahead; round 5 326.7 vs 326.4 M, profiles/r05/scan_ahead), and a copy thread that
// issues every chunk's copies in order, running ahead of the thread that enqueues the kernels
// (round 6: the chunks land earlier, the step does not move, profiles/r06/copy_thread).
struct TxsigFeed {
  cg_ctx* c;
  HostTrace& tr;
  const std::vector<uint64_t>& bounds;
  const TxsigReq& h;  // the caller's buffers
  const TxsigReq& d;  // what the kernels see: the arena's length, where the 12-byte form's stream follows it
  const uint64_t nt;  // host threads of the extent scans, run through `par`
  const cg::ParFor& par;
  std::vector<Extent> ext_e, ext_i;  // chunk k's signature bytes / id bytes
  // the 12-byte table: chunk k's first signature at stream offset cbase[k] (cbase[k + 1] is set when
  // chunk k's table slice is staged)
  std::vector<uint64_t> cbase;
  cg::Resident have, have_ids, have_sig;  // arena bytes / id bytes / the 12-byte form's stream bytes on the device
  hipError_t copy_err = hipSuccess;       // the first failure inside a hook
  uint64_t mid_k = 0;                     // the chunk whose `mid` is pending
  const std::function<hipError_t()> mid_hook = [this] { return mid(); };
  const std::function<hipError_t(uint64_t, uint64_t, uint64_t)> before_hook = [this](uint64_t k, uint64_t, uint64_t) {
    return before(k);
  };

  TxsigFeed(cg_ctx* ctx, HostTrace& trace, const std::vector<uint64_t>& b, const TxsigReq& host, const TxsigReq& dev,
            uint64_t threads, const cg::ParFor& pf)
      : c(ctx), tr(trace), bounds(b), h(host), d(dev), nt(threads), par(pf), ext_e(b.size() - 1),
        ext_i(b.size() - 1), cbase(b.size(), 0) {}
  TxsigFeed(const TxsigFeed&) = delete;
  ~TxsigFeed() { c->fork.mid_front = nullptr; }  // no hook outlives the call, whatever the exit path

  // chunk k's extents (exact: a threaded scan of its slice of the table) and its table slice
  hipError_t copy_table(uint64_t k) {
    const uint64_t first = bounds[k], cnt = bounds[k + 1] - bounds[k];
    const double h0 = tr.ms();
    const cg::ChunkScan x = cg::with_records(h.sigs, [&](auto* recs) {
      return cg::scan_chunk(recs, first, first + cnt, h.n_ids, d.arena_len, nt, par);
    });
    ext_e[k] = x.sig;
    ext_i[k] = x.ids;
    if (h.sigs.packed()) {  // the chunk's stream bytes, clipped to the caller's buffer (past it: CG_NOT_RUN)
      cbase[k + 1] = cbase[k] + x.span;
      ext_e[k] = Extent();
      ext_e[k].add(cbase[k], x.span, h.sig_bytes_len);
    }
    const double h1 = tr.ms();
    const hipError_t e = hipMemcpyAsync((uint8_t*)c->h_sigs.p + (size_t)h.sigs.stride * first, h.sigs.from(first).p,
                                        (size_t)h.sigs.stride * cnt, hipMemcpyHostToDevice, c->copy);
    tr.table_staged(k, h0, h1);
    return e;
  }
  // chunk k's ids and signature bytes; seg[k] marks the end
  hipError_t copy_bytes(uint64_t k) {
    const Extent& ek = ext_e[k];
    uint8_t* dwin = (uint8_t*)c->arena.p;  // the device arena mirrors [0, arena_len)
    const double h2 = tr.ms();
    hipError_t e = copy_missing(have_ids, ext_i[k], h.ids, (uint8_t*)c->h_ids.p, 0, c->copy);
    const double h3 = tr.ms();
    if (e == hipSuccess && h.sigs.packed()) e = copy_missing(have_sig, ek, h.sig_bytes, dwin + d.sig_bytes_off, 0, c->copy);
    else if (e == hipSuccess) e = copy_missing(have, ek, h.arena, dwin, 0, c->copy);
    if (e == hipSuccess) e = hipEventRecord(c->seg[k], c->copy);
    if (e == hipSuccess) e = tr.bytes_staged(k, c->copy, h2, h3, h.sigs.stride * (bounds[k + 1] - bounds[k]) / 1e6, ek);
    return e;
  }
  // the second half of chunk mid_k's staging: bytes copied, the front's stream ordered after them
  hipError_t mid() {
    c->fork.mid_front = nullptr;
    const uint64_t k = mid_k;
    hipStream_t s = c->stream;
    hipError_t e = copy_bytes(k);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, c->seg[k], 0);
    if (e == hipSuccess) e = tr.front_reached(k, s);
    if (e == hipSuccess && k == 0) e = hipEventRecord(c->tev[1], s);
    if (e != hipSuccess) copy_err = e;
    return e;
  }
  // chunk k's front waits only for its signature-table slice; `mid` is left for the front to run
  hipError_t before(uint64_t k) {
    hipStream_t s = c->stream;
    hipError_t e = c->fork.mid_front ? mid() : hipSuccess;  // a hook a front did not consume
    if (e == hipSuccess) e = copy_table(k);
    if (e == hipSuccess) e = hipEventRecord(c->segtab[k], c->copy);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, c->segtab[k], 0);
    if (e == hipSuccess) {
      mid_k = k;
      c->fork.mid_front = &mid_hook;
    }
    if (e != hipSuccess) copy_err = e;
    return e;
  }
};

// ---- per-transaction verdicts (txverdict.hip): the host forms' tables (cg::TxvSet `h`), staged in one
// buffer (`d`)
// Carves c->txvio for the tables of `h` (waits for the device when it grows), and the list workspace.
static hipError_t txv_stage(cg_ctx* c, const cg::TxvSet& h, uint32_t n_keys, cg::TxvSet* d) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t o_checks = 0, o_nodes = o_checks + up(sizeof(cg_tx_check) * h.n_tx),
               o_verd = o_nodes + up(sizeof(cg_req_node) * h.n_nodes),
               o_reqs = o_verd + up(sizeof(cg_tx_verdict) * h.n_tx),
               o_class = o_reqs + up(sizeof(uint32_t) * h.n_reqs),
               o_rst = o_class + up(h.key_class ? sizeof(uint32_t) * n_keys : 0), need = o_rst + up(h.n_reqs) + 16;
  const hipError_t e = ensure_all({{&c->txvws, cg::tx_verdicts_ws_bytes(h.n_tx)}, {&c->txvio, need}});
  if (e != hipSuccess) return e;
  uint8_t* b = (uint8_t*)c->txvio.p;
  *d = h;  // the counts
  d->checks = (cg_tx_check*)(b + o_checks);
  d->nodes = (cg_req_node*)(b + o_nodes);
  d->verdicts = (cg_tx_verdict*)(b + o_verd);
  d->reqs = (uint32_t*)(b + o_reqs);
  d->key_class = h.key_class ? (uint32_t*)(b + o_class) : nullptr;
  d->req_status = b + o_rst;
  return hipSuccess;
}
// (d's tables are the context's own buffer, carved by txv_stage: writable)
static hipError_t txv_upload(const cg::TxvSet& h, uint32_t n_keys, const cg::TxvSet& d, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (h.n_tx) e = hipMemcpyAsync((void*)d.checks, h.checks, sizeof(cg_tx_check) * h.n_tx, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && h.n_nodes)
    e = hipMemcpyAsync((void*)d.nodes, h.nodes, sizeof(cg_req_node) * h.n_nodes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && h.n_reqs)
    e = hipMemcpyAsync((void*)d.reqs, h.reqs, sizeof(uint32_t) * h.n_reqs, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && h.key_class && n_keys)
    e = hipMemcpyAsync((void*)d.key_class, h.key_class, sizeof(uint32_t) * n_keys, hipMemcpyHostToDevice, s);
  return e;
}
static hipError_t txv_download(const cg::TxvSet& h, const cg::TxvSet& d, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (h.n_tx) e = hipMemcpyAsync(h.verdicts, d.verdicts, sizeof(cg_tx_verdict) * h.n_tx, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && h.n_reqs) e = hipMemcpyAsync(h.req_status, d.req_status, h.n_reqs, hipMemcpyDeviceToHost, s);
  return e;
}
// what a call that failed leaves in the caller's result buffers: nothing ran
static void txv_fill_not_run(const cg::TxvSet& h) {
  for (uint64_t t = 0; t < h.n_tx; ++t) h.verdicts[t] = cg_tx_verdict{0xFFFFFFFFu, CG_NOT_RUN, CG_TXV_SPAN_BAD, 0};
  if (h.n_reqs) memset(h.req_status, CG_REQ_HOST, h.n_reqs);
}

// cg_verify_tx_signatures with the ctx lock held, over the caller's host buffers `q`. Host side, in
// order: the key table and key bytes, the template bytes, the ids and the signature table (everything
// the key tables and the plans need), then the signature bytes chunk by chunk, each copy issued just
// before its chunk's front so that the key-table builds and the previous chunk's kernels run during it.
// The 12-byte form (cg_verify_tx_signatures_packed): the signatures dense in q.sig_bytes. On the
// device they follow the caller's arena at sig_region (16-aligned), so the kernels address every byte
// by an absolute arena offset as in the 24-byte form; a key or template that lies outside [0,
// arena_len) is moved out of the extended arena too (never reads a signature).
// txv (cg_verify_required_signatures_packed; else null): the per-transaction verdict kernels follow the
// last chunk on the same stream; their tables go up on the copy stream behind the last chunk's bytes.
// q.status may then be null (the statuses stay on the device).
static int verify_txsig_host_locked(cg_ctx* c, const TxsigReq& q, cg_stats* stats, const cg::TxvSet* txv) {
  const auto t0 = std::chrono::steady_clock::now();
  const bool packed = q.sigs.packed();
  const uint32_t n_keys = q.n_keys, n_tmpls = q.n_tmpls;
  const uint64_t n_sigs = q.n_sigs, n_ids = q.n_ids;
  TxsigReq h = q;  // the caller's buffers, its keys and templates fixed up
  TxsigReq d = q;  // what the kernels see
  d.sig_bytes_off = packed ? ((q.arena_len + 15) & ~(uint64_t)15) : 0;
  if (packed) d.arena_len = d.sig_bytes_off + q.sig_bytes_len;
  std::vector<cg_key> keys_fix;
  std::vector<cg_signable_tmpl> tmpls_fix;
  if (packed) {  // out-of-arena keys / templates stay out of range in the extended arena
    cg::txsig_packed_fixup(q.keys, n_keys, q.tmpls, n_tmpls, q.arena_len, keys_fix, tmpls_fix);
    if (!keys_fix.empty()) h.keys = keys_fix.data();
    if (!tmpls_fix.empty()) h.tmpls = tmpls_fix.data();
  }
  d.tmpls = h.tmpls;
  if (const int rc = enter(c, "cg_verify_tx_signatures")) return rc;
  // chunk bounds (txsig_plan.h); `per`, the largest chunk, sizes the item workspaces
  static const uint64_t first_div = env_u64("CG_TXSIG_FIRST_DIV", cg::kTxsigFirstDiv);
  const std::vector<uint64_t> bounds = cg::txsig_bounds(n_sigs, c->chunk, c->chunk_set, first_div);
  const uint64_t nch = bounds.size() - 1, per = cg::largest_chunk(bounds);
  // arena extents: key bytes + template bytes (the header), then each chunk's signature bytes, scanned
  // just before its copy, while the device works on the chunks before it
  const Extent head = cg::txsig_head_extent(h.keys, n_keys, h.tmpls, n_tmpls, q.arena_len);
  // the budget's host threads (host_budget.h), on the context's pool (spawning 16 threads per scan
  // cost 0.35-0.5 ms a round)
  const uint64_t nt = host_threads_of(c, n_sigs);
  const cg::ParFor par = [c](uint64_t m, const std::function<void(uint64_t)>& fn) { host_par(c, m, fn); };
  std::vector<uint32_t> counts(n_keys ? n_keys : 1, 0u);
  const uint64_t slot = tmpl_slot(h.tmpls, n_tmpls);
  HIP_TRY(c->keys.ensure(sizeof(cg_key) * (n_keys ? n_keys : 1)), "hipMalloc(keys)");
  HIP_TRY(c->h_sigs.ensure(q.sigs.stride * n_sigs), "hipMalloc(sigs)");
  if (packed) HIP_TRY(c->sig12ws.ensure(cg::tx_sig12_scratch_bytes(per)), "hipMalloc(signature offsets)");
  HIP_TRY(c->aux1.ensure(sizeof(uint32_t) * counts.size()), "hipMalloc(key use counts)");
  HIP_TRY(c->h_ids.ensure(32 * (n_ids ? n_ids : 1)), "hipMalloc(ids)");
  HIP_TRY(c->arena.ensure(d.arena_len + 16), "hipMalloc(arena window)");  // mirrors [0, arena_len): only referenced bytes are copied
  HIP_TRY(c->status.ensure(n_sigs), "hipMalloc(status)");
  HIP_TRY(ensure_txsig_ws(c, n_sigs, n_tmpls, slot), "hipMalloc(tx signature workspace)");
  HIP_TRY(ensure_ws(c, n_keys, per, n_sigs), "hipMalloc(workspace)");
  cg::TxvSet txd;
  if (txv) HIP_TRY(txv_stage(c, *txv, n_keys, &txd), "hipMalloc(verdict tables)");
  HIP_TRY(ensure_events(c->seg, nch + 1), "hipEventCreate");
  HIP_TRY(ensure_events(c->segtab, nch), "hipEventCreate");
  static const bool htrace = env_flag("CG_HOST_TRACE", false);
  HostTrace tr{c, t0, htrace, {}};
  HIP_TRY(tr.begin(nch), "hipEventCreate");
  hipStream_t s = c->stream;
  d.keys = (const cg_key*)c->keys.p;
  d.ids = (const uint8_t*)c->h_ids.p;
  d.sigs.p = c->h_sigs.p;
  d.arena = (const uint8_t*)c->arena.p;  // kernels index the arena by absolute offsets
  d.status = (uint8_t*)c->status.p;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(hipEventRecord(c->tev[0], s), "hipEventRecord");
  HIP_TRY(hipStreamWaitEvent(c->copy, c->tev[0], 0), "hipStreamWaitEvent");
  TxsigFeed feed(c, tr, bounds, h, d, nt, par);
  if (n_keys)
    HIP_TRY(hipMemcpyAsync(c->keys.p, h.keys, sizeof(cg_key) * n_keys, hipMemcpyHostToDevice, c->copy), "H2D keys");
  HIP_TRY(copy_missing(feed.have, head, h.arena, (uint8_t*)c->arena.p, 0, c->copy), "H2D key / template bytes");
  // The key-use counts (txsig_plan.h) gate only the key tables; chunk 0's bytes gate everything else.
  // (Sampling the counts while chunk 0 copies, on a second copy stream with a pinned counts buffer,
  // measured slower on the configs[4] shard: 197 / 205 vs 213 / 220 M sigs/s, profiles/r03/ab_sc: the
  // sample pass slows 2x beside the pageable copy's staging and the late counts delay the key tables.)
  {
    static const uint32_t S_env = cg::sample_override((uint32_t)env_u64("CG_TXSIG_SAMPLE", 0));
    static const uint32_t B = cg::sample_block((uint32_t)env_u64("CG_TXSIG_SAMPLE_BLOCK", cg::kTxsigSampleBlock));
    const uint32_t S = cg::sample_rate(S_env, n_sigs, n_keys);
    const cg::WidePool thr = c->eng->make_wide_pool(nullptr, n_keys, n_sigs, cg::kKeyWideMax, 0);  // the wide thresholds
    cg::with_records(h.sigs, [&](auto* recs) {
      cg::key_use_counts(recs, n_sigs, h.keys, n_keys, nt, par, S, B, thr.min_ed, thr.min_ec, c->count_scratch,
                         counts.data());
    });
  }
  const double ms_plan = ms_since(t0);  // host-side planning: the key-use sample pass
  HIP_TRY(hipMemcpyAsync(c->aux1.p, counts.data(), sizeof(uint32_t) * counts.size(), hipMemcpyHostToDevice, c->copy),
          "H2D key use counts");
  HIP_TRY(hipEventRecord(c->seg[nch], c->copy), "hipEventRecord");
  HIP_TRY(hipStreamWaitEvent(s, c->seg[nch], 0), "hipStreamWaitEvent");
  TxsigSched sched{bounds, {}, &feed.before_hook, packed ? &feed.cbase : nullptr, nullptr};
  sched.uses.counts = (const uint32_t*)c->aux1.p;
  sched.uses.n = n_sigs;
  sched.uses.host_keys = h.keys;
  sched.uses.host_counts = counts.data();
  const hipError_t le = launch_txsig(c, d, slot, sched, s);
  if (le == hipSuccess && c->fork.mid_front) feed.mid();  // the last front did not consume its hook
  if (feed.copy_err != hipSuccess) return hip_fail(feed.copy_err, "H2D signature bytes");
  HIP_TRY(le, "launch_txsig");
  if (txv) {  // after the last chunk's back, the joined side streams and the mode guard: all on s by now
    HIP_TRY(txv_upload(*txv, n_keys, txd, c->copy), "H2D verdict tables");
    HIP_TRY(hipEventRecord(c->seg[nch], c->copy), "hipEventRecord");
    HIP_TRY(hipStreamWaitEvent(s, c->seg[nch], 0), "hipStreamWaitEvent");
    HIP_TRY(cg::launch_tx_verdicts(d.sigs, n_sigs, d.status, d.keys, n_keys, txd, c->txvws.p, s), "launch_tx_verdicts");
  }
  HIP_TRY(hipEventRecord(c->tev[2], s), "hipEventRecord");
  if (q.status) HIP_TRY(hipMemcpyAsync(q.status, d.status, n_sigs, hipMemcpyDeviceToHost, s), "D2H status");
  if (txv) HIP_TRY(txv_download(*txv, txd, s), "D2H verdicts");
  HIP_TRY(hipEventRecord(c->tev[3], s), "hipEventRecord");
  HIP_TRY(call.close(), "hipEventRecord");
  const double h_enq = tr.ms();
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  tr.report(nch, h_enq);
  fill_stats(c, stats, n_sigs, n_keys, ms_plan, t0);
  return CG_OK;
}

// The argument checks of the tx-signature family: what every form checks (need_status: the status
// buffer must be there when there are signatures), then what only the forms over host buffers (which
// the library reads itself) or only the device forms (the 12-byte table's stream) check.
static int txsig_args(const char* fn, cg_ctx* c, const TxsigReq& q, bool need_status = true) {
  if (!c) return fail(CG_ERR_ARG, "%s: ctx is NULL", fn);
  if (q.n_sigs && (!q.sigs.p || (need_status && !q.status)))
    return fail(CG_ERR_ARG, "%s: NULL signature / status buffer", fn);
  if (q.n_keys && !q.keys) return fail(CG_ERR_ARG, "%s: keys is NULL", fn);
  if (q.n_ids && !q.ids) return fail(CG_ERR_ARG, "%s: ids is NULL", fn);
  if (q.n_tmpls && !q.tmpls) return fail(CG_ERR_ARG, "%s: templates is NULL", fn);
  if (q.n_tmpls > 0x10000u) return fail(CG_ERR_ARG, "%s: more than 65536 templates (cg_txsig.tmpl is 16-bit)", fn);
  if (q.mode > CG_MODE_ISVALID) return fail(CG_ERR_ARG, "%s: bad mode", fn);
  return CG_OK;
}
static int txsig_buffer_args(const char* fn, const TxsigReq& q, bool host) {
  if (host && q.arena_len && !q.arena) return fail(CG_ERR_ARG, "%s: arena is NULL", fn);
  if (host && q.sig_bytes_len && !q.sig_bytes) return fail(CG_ERR_ARG, "%s: sig_bytes is NULL", fn);
  if (!host && (q.sig_bytes_off > q.arena_len || q.sig_bytes_len > q.arena_len - q.sig_bytes_off))
    return fail(CG_ERR_ARG, "%s: the signature stream lies outside the arena", fn);
  return CG_OK;
}

int cg_verify_tx_signatures_device(cg_ctx* c, const cg_key* d_keys, uint32_t n_keys, const uint8_t* d_ids,
                                   uint64_t n_ids, const cg_txsig* d_sigs, uint64_t n_sigs,
                                   const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena,
                                   uint64_t arena_len, uint32_t mode, uint8_t* d_status, void* hip_stream) {
  const TxsigReq d = {d_keys, n_keys,  d_ids,   n_ids,     {d_sigs, (uint32_t)sizeof(cg_txsig)}, n_sigs,
                      tmpls,  n_tmpls, d_arena, arena_len, mode,                                 d_status};
  if (const int a = txsig_args("cg_verify_tx_signatures_device", c, d)) return a;
  if (n_sigs == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_verify_tx_signatures_device")) return rc;
  const uint64_t slot = tmpl_slot(tmpls, n_tmpls);
  const std::vector<uint64_t> bounds = cg::equal_bounds(n_sigs, chunk_of(c, n_sigs));
  HIP_TRY(ensure_txsig_ws(c, n_sigs, n_tmpls, slot), "hipMalloc(tx signature workspace)");
  HIP_TRY(ensure_ws(c, n_keys, chunk_of(c, n_sigs), n_sigs), "hipMalloc(workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  TxsigSched sched{bounds, {}};
  sched.uses.sigs = d.sigs;
  sched.uses.n = n_sigs;
  HIP_TRY(launch_txsig(c, d, slot, sched, call.stream()), "launch_txsig");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

// The two halves of a packed device call over the device tables `d`, with the ctx lock held and the
// device set: the chunk bounds and the workspace before the call opens, then every launch up to the
// last chunk's back on `s`.
static hipError_t txsig_packed_device_ws(cg_ctx* c, const TxsigReq& d, uint64_t slot, std::vector<uint64_t>& bounds) {
  if (d.n_sigs == 0) return hipSuccess;
  // equal chunks rounded to the 256-record blocks whose stream offsets are computed once for the table
  const uint64_t per = (chunk_of(c, d.n_sigs) + 255) & ~(uint64_t)255;
  bounds = cg::equal_bounds(d.n_sigs, per);
  hipError_t e = ensure_txsig_ws(c, d.n_sigs, d.n_tmpls, slot);
  if (e == hipSuccess) e = ensure_ws(c, d.n_keys, per, d.n_sigs);
  if (e == hipSuccess) e = c->sig12ws.ensure(cg::tx_sig12_scratch_bytes(d.n_sigs));
  return e;
}
static hipError_t launch_txsig_packed_device(cg_ctx* c, const TxsigReq& d, uint64_t slot,
                                             const std::vector<uint64_t>& bounds, hipStream_t s) {
  if (d.n_sigs == 0) return hipSuccess;
  const hipError_t e =
      cg::launch_tx_sig12_bases((const cg_txsig_packed*)d.sigs.p, 0, d.n_sigs, 0, (uint64_t*)c->sig12ws.p, s);
  if (e != hipSuccess) return e;
  TxsigSched sched{bounds, {}, nullptr, nullptr, (const uint64_t*)c->sig12ws.p};
  sched.uses.sigs = d.sigs;
  sched.uses.n = d.n_sigs;
  return launch_txsig(c, d, slot, sched, s);
}

int cg_verify_tx_signatures_packed_device(cg_ctx* c, const cg_key* d_keys, uint32_t n_keys, const uint8_t* d_ids,
                                          uint64_t n_ids, const cg_txsig_packed* d_sigs, uint64_t n_sigs,
                                          uint64_t sig_bytes_off, uint64_t sig_bytes_len,
                                          const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena,
                                          uint64_t arena_len, uint32_t mode, uint8_t* d_status, void* hip_stream) {
  const char* fn = "cg_verify_tx_signatures_packed_device";
  const TxsigReq d = {d_keys,  n_keys,  d_ids,     n_ids, {d_sigs, (uint32_t)sizeof(cg_txsig_packed)}, n_sigs,  tmpls,
                      n_tmpls, d_arena, arena_len, mode,  d_status, nullptr, sig_bytes_off, sig_bytes_len};
  int a = txsig_args(fn, c, d);
  if (a == CG_OK) a = txsig_buffer_args(fn, d, false);
  if (a != CG_OK) return a;
  if (n_sigs == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  const uint64_t slot = tmpl_slot(tmpls, n_tmpls);
  std::vector<uint64_t> bounds;
  HIP_TRY(txsig_packed_device_ws(c, d, slot, bounds), "hipMalloc(tx signature workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(launch_txsig_packed_device(c, d, slot, bounds, call.stream()), "launch_txsig");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

// cg_verify_tx_signatures and its packed form over the caller's host buffers `h`, arguments checked
static int verify_txsig_host(cg_ctx* c, const TxsigReq& h, cg_stats* stats) {
  if (h.n_sigs) memset(h.status, CG_NOT_RUN, h.n_sigs);
  if (h.n_sigs == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  const int rc = verify_txsig_host_locked(c, h, stats, nullptr);
  if (rc != CG_OK) memset(h.status, CG_NOT_RUN, h.n_sigs);
  return rc;
}

int cg_verify_tx_signatures_packed(cg_ctx* c, const cg_key* keys, uint32_t n_keys, const uint8_t* ids, uint64_t n_ids,
                                   const cg_txsig_packed* sigs, uint64_t n_sigs, const uint8_t* sig_bytes,
                                   uint64_t sig_bytes_len, const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                                   const uint8_t* arena, uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                                   cg_stats* stats) {
  const char* fn = "cg_verify_tx_signatures_packed";
  const TxsigReq h = {keys,    n_keys, ids,       n_ids, {sigs, (uint32_t)sizeof(cg_txsig_packed)}, n_sigs,    tmpls,
                      n_tmpls, arena,  arena_len, mode,  status_out, sig_bytes, 0, sig_bytes_len};
  int a = txsig_args(fn, c, h);
  if (a == CG_OK) a = txsig_buffer_args(fn, h, true);
  return a != CG_OK ? a : verify_txsig_host(c, h, stats);
}

int cg_verify_tx_signatures(cg_ctx* c, const cg_key* keys, uint32_t n_keys, const uint8_t* ids, uint64_t n_ids,
                            const cg_txsig* sigs, uint64_t n_sigs, const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                            const uint8_t* arena, uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                            cg_stats* stats) {
  const char* fn = "cg_verify_tx_signatures";
  const TxsigReq h = {keys,  n_keys,  ids,   n_ids,     {sigs, (uint32_t)sizeof(cg_txsig)}, n_sigs,
                      tmpls, n_tmpls, arena, arena_len, mode,                               status_out};
  int a = txsig_args(fn, c, h);
  if (a == CG_OK) a = txsig_buffer_args(fn, h, true);
  return a != CG_OK ? a : verify_txsig_host(c, h, stats);
}

// ---------------------------------------------------------------- per-transaction verdicts
static int txv_args(const char* fn, const cg::SigTable& sigs, uint64_t n_sigs, const void* status, uint32_t n_keys,
                    const void* keys, const cg::TxvSet& t) {
  if (sigs.stride != sizeof(cg_txsig_packed) && sigs.stride != sizeof(cg_txsig))
    return fail(CG_ERR_ARG, "%s: sig_stride is neither 12 (cg_txsig_packed) nor 24 (cg_txsig)", fn);
  if (n_sigs && (!sigs.p || !status)) return fail(CG_ERR_ARG, "%s: NULL signature table / status", fn);
  if (n_keys && !keys) return fail(CG_ERR_ARG, "%s: keys is NULL", fn);
  if (t.n_tx && (!t.checks || !t.verdicts)) return fail(CG_ERR_ARG, "%s: NULL checks / verdicts", fn);
  if (t.n_tx > 0xFFFFFFFFull) return fail(CG_ERR_ARG, "%s: more than 2^32 - 1 transactions", fn);
  if (t.n_reqs && (!t.reqs || !t.req_status)) return fail(CG_ERR_ARG, "%s: NULL reqs / req_status", fn);
  if (t.n_nodes && !t.nodes) return fail(CG_ERR_ARG, "%s: nodes is NULL", fn);
  return CG_OK;
}
static int txv_reserved(const char* fn, const cg::TxvSet& t) {
  for (uint64_t k = 0; k < t.n_tx; ++k)
    if (t.checks[k].reserved != 0) return fail(CG_ERR_ARG, "%s: cg_tx_check.reserved must be 0", fn);
  return CG_OK;
}

int cg_tx_verdicts_device(cg_ctx* c, const void* d_sig_table, uint32_t sig_stride, uint64_t n_sigs,
                          const uint8_t* d_status, const cg_key* d_keys, uint32_t n_keys, const uint32_t* d_key_class,
                          const cg_tx_check* d_checks, uint64_t n_tx, const uint32_t* d_reqs, uint32_t n_reqs,
                          const cg_req_node* d_nodes, uint32_t n_nodes, cg_tx_verdict* d_verdicts,
                          uint8_t* d_req_status, void* hip_stream) {
  if (!c) return fail(CG_ERR_ARG, "cg_tx_verdicts_device: ctx is NULL");
  const cg::SigTable sigs = {d_sig_table, sig_stride};
  const cg::TxvSet d = {d_key_class, d_checks, n_tx, d_reqs, n_reqs, d_nodes, n_nodes, d_verdicts, d_req_status};
  if (const int a = txv_args("cg_tx_verdicts_device", sigs, n_sigs, d_status, n_keys, d_keys, d)) return a;
  if (n_tx == 0 && n_reqs == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_tx_verdicts_device")) return rc;
  HIP_TRY(ensure_all({{&c->txvws, cg::tx_verdicts_ws_bytes(n_tx)}}), "hipMalloc(verdict workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(cg::launch_tx_verdicts(sigs, n_sigs, d_status, d_keys, n_keys, d, c->txvws.p, call.stream()),
          "launch_tx_verdicts");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

static int tx_verdicts_host_locked(cg_ctx* c, const cg::SigTable& sigs, uint64_t n_sigs, const uint8_t* status,
                                   const cg_key* keys, uint32_t n_keys, const cg::TxvSet& h) {
  if (const int rc = enter(c, "cg_tx_verdicts")) return rc;
  cg::TxvSet d;
  HIP_TRY(txv_stage(c, h, n_keys, &d), "hipMalloc(verdict tables)");
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->h_sigs, sigs.p, (size_t)sigs.stride * n_sigs, s), "H2D sigs");
  HIP_TRY(stage(c->status, status, n_sigs, s), "H2D status");
  HIP_TRY(stage(c->keys, keys, sizeof(cg_key) * n_keys, s), "H2D keys");
  HIP_TRY(txv_upload(h, n_keys, d, s), "H2D verdict tables");
  HIP_TRY(cg::launch_tx_verdicts({c->h_sigs.p, sigs.stride}, n_sigs, (const uint8_t*)c->status.p,
                                 (const cg_key*)c->keys.p, n_keys, d, c->txvws.p, s),
          "launch_tx_verdicts");
  HIP_TRY(txv_download(h, d, s), "D2H verdicts");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

int cg_tx_verdicts(cg_ctx* c, const void* sig_table, uint32_t sig_stride, uint64_t n_sigs, const uint8_t* status,
                   const cg_key* keys, uint32_t n_keys, const uint32_t* key_class, const cg_tx_check* checks,
                   uint64_t n_tx, const uint32_t* reqs, uint32_t n_reqs, const cg_req_node* nodes, uint32_t n_nodes,
                   cg_tx_verdict* verdicts_out, uint8_t* req_status_out) {
  if (!c) return fail(CG_ERR_ARG, "cg_tx_verdicts: ctx is NULL");
  const cg::SigTable sigs = {sig_table, sig_stride};
  const cg::TxvSet h = {key_class, checks, n_tx, reqs, n_reqs, nodes, n_nodes, verdicts_out, req_status_out};
  int a = txv_args("cg_tx_verdicts", sigs, n_sigs, status, n_keys, keys, h);
  if (a == CG_OK) a = txv_reserved("cg_tx_verdicts", h);
  if (a != CG_OK) return a;
  if (n_tx == 0 && n_reqs == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  const int rc = tx_verdicts_host_locked(c, sigs, n_sigs, status, keys, n_keys, h);
  if (rc != CG_OK) txv_fill_not_run(h);
  return rc;
}

int cg_verify_required_signatures_packed_device(cg_ctx* c, const cg_key* d_keys, uint32_t n_keys,
                                                const uint8_t* d_ids, uint64_t n_ids, const cg_txsig_packed* d_sigs,
                                                uint64_t n_sigs, uint64_t sig_bytes_off, uint64_t sig_bytes_len,
                                                const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                                                const uint8_t* d_arena, uint64_t arena_len, uint32_t mode,
                                                const uint32_t* d_key_class, const cg_tx_check* d_checks,
                                                uint64_t n_tx, const uint32_t* d_reqs, uint32_t n_reqs,
                                                const cg_req_node* d_nodes, uint32_t n_nodes, uint8_t* d_status,
                                                cg_tx_verdict* d_verdicts, uint8_t* d_req_status, void* hip_stream) {
  const char* fn = "cg_verify_required_signatures_packed_device";
  const TxsigReq d = {d_keys,  n_keys,  d_ids,     n_ids, {d_sigs, (uint32_t)sizeof(cg_txsig_packed)}, n_sigs,  tmpls,
                      n_tmpls, d_arena, arena_len, mode,  d_status, nullptr, sig_bytes_off, sig_bytes_len};
  const cg::TxvSet t = {d_key_class, d_checks, n_tx, d_reqs, n_reqs, d_nodes, n_nodes, d_verdicts, d_req_status};
  int a = txsig_args(fn, c, d);
  if (a == CG_OK) a = txv_args(fn, d.sigs, n_sigs, d_status, n_keys, d_keys, t);
  if (a == CG_OK) a = txsig_buffer_args(fn, d, false);
  if (a != CG_OK) return a;
  if (n_sigs == 0 && n_tx == 0 && n_reqs == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  HIP_TRY(ensure_all({{&c->txvws, cg::tx_verdicts_ws_bytes(n_tx)}}), "hipMalloc(verdict workspace)");
  const uint64_t slot = tmpl_slot(tmpls, n_tmpls);
  std::vector<uint64_t> bounds;
  HIP_TRY(txsig_packed_device_ws(c, d, slot, bounds), "hipMalloc(tx signature workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  hipStream_t s = call.stream();
  HIP_TRY(launch_txsig_packed_device(c, d, slot, bounds, s), "launch_txsig");
  // launch_txsig has joined the side streams and run the mode guard on s: the statuses are final there
  HIP_TRY(cg::launch_tx_verdicts(d.sigs, n_sigs, d_status, d_keys, n_keys, t, c->txvws.p, s), "launch_tx_verdicts");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

int cg_verify_required_signatures_packed(cg_ctx* c, const cg_key* keys, uint32_t n_keys, const uint8_t* ids,
                                         uint64_t n_ids, const cg_txsig_packed* sigs, uint64_t n_sigs,
                                         const uint8_t* sig_bytes, uint64_t sig_bytes_len,
                                         const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                         uint64_t arena_len, uint32_t mode, const uint32_t* key_class,
                                         const cg_tx_check* checks, uint64_t n_tx, const uint32_t* reqs,
                                         uint32_t n_reqs, const cg_req_node* nodes, uint32_t n_nodes,
                                         uint8_t* status_out, cg_tx_verdict* verdicts_out, uint8_t* req_status_out,
                                         cg_stats* stats) {
  const char* fn = "cg_verify_required_signatures_packed";
  const TxsigReq q = {keys,    n_keys, ids,       n_ids, {sigs, (uint32_t)sizeof(cg_txsig_packed)}, n_sigs,    tmpls,
                      n_tmpls, arena,  arena_len, mode,  status_out, sig_bytes, 0, sig_bytes_len};
  const cg::TxvSet h = {key_class, checks, n_tx, reqs, n_reqs, nodes, n_nodes, verdicts_out, req_status_out};
  // status_out may be NULL (the verdict checks then take the table for it)
  int a = txsig_args(fn, c, q, false);
  if (a == CG_OK) a = txv_args(fn, q.sigs, n_sigs, sigs, n_keys, keys, h);
  if (a == CG_OK) a = txv_reserved(fn, h);
  if (a == CG_OK) a = txsig_buffer_args(fn, q, true);
  if (a != CG_OK) return a;
  if (n_sigs && status_out) memset(status_out, CG_NOT_RUN, n_sigs);
  if (n_sigs == 0 && n_tx == 0 && n_reqs == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  // without signatures the verify path has nothing to enqueue: the reduction alone
  const int rc = n_sigs ? verify_txsig_host_locked(c, q, stats, &h)
                        : tx_verdicts_host_locked(c, q.sigs, 0, nullptr, keys, n_keys, h);
  if (rc != CG_OK) {
    if (n_sigs && status_out) memset(status_out, CG_NOT_RUN, n_sigs);
    txv_fill_not_run(h);
  }
  return rc;
}

int cg_verify_filtered_device(cg_ctx* c, const cg_filtered_tx* d_ftxs, uint64_t n_ftx, const cg_pmt_node* d_nodes,
                              uint64_t n_nodes, const cg_filtered_leaf* d_leaves, uint64_t n_leaves,
                              const uint8_t* d_arena, uint64_t arena_len, uint8_t* d_status, void* hip_stream) {
  if (!c) return fail(CG_ERR_ARG, "cg_verify_filtered_device: ctx is NULL");
  if (n_ftx && (!d_ftxs || !d_status)) return fail(CG_ERR_ARG, "cg_verify_filtered_device: NULL buffer");
  if (n_ftx == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_verify_filtered_device")) return rc;
  HIP_TRY(ensure_all({{&c->ftxws, cg::ftx_ws_bytes(n_leaves)}}), "hipMalloc(filtered ws)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(cg::launch_filtered(d_ftxs, n_ftx, d_nodes, n_nodes, d_leaves, n_leaves, d_arena, arena_len, d_status,
                              (uint8_t*)c->ftxws.p, call.stream()), "launch_filtered");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

int cg_verify_filtered(cg_ctx* c, const cg_filtered_tx* ftxs, uint64_t n_ftx, const cg_pmt_node* nodes,
                       uint64_t n_nodes, const cg_filtered_leaf* leaves, uint64_t n_leaves, const uint8_t* arena,
                       uint64_t arena_len, uint8_t* status_out) {
  if (!c) return fail(CG_ERR_ARG, "cg_verify_filtered: ctx is NULL");
  if (n_ftx && (!ftxs || !status_out)) return fail(CG_ERR_ARG, "cg_verify_filtered: NULL buffer");
  if ((n_nodes && !nodes) || (n_leaves && !leaves) || (arena_len && !arena))
    return fail(CG_ERR_ARG, "cg_verify_filtered: NULL table");
  if (n_ftx == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, "cg_verify_filtered")) return rc;
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->h_txs, ftxs, sizeof(cg_filtered_tx) * n_ftx, s), "H2D ftxs");
  HIP_TRY(stage(c->h_comps, nodes, sizeof(cg_pmt_node) * n_nodes, s), "H2D nodes");
  HIP_TRY(stage(c->h_sigs, leaves, sizeof(cg_filtered_leaf) * n_leaves, s), "H2D leaves");
  HIP_TRY(stage(c->arena, arena, arena_len, s, arena_room(arena_len)), "H2D arena");
  HIP_TRY(c->status.ensure(n_ftx), "hipMalloc(status)");
  HIP_TRY(c->ftxws.ensure(cg::ftx_ws_bytes(n_leaves)), "hipMalloc(filtered ws)");
  HIP_TRY(cg::launch_filtered((const cg_filtered_tx*)c->h_txs.p, n_ftx, (const cg_pmt_node*)c->h_comps.p, n_nodes,
                              (const cg_filtered_leaf*)c->h_sigs.p, n_leaves, (const uint8_t*)c->arena.p, arena_len,
                              (uint8_t*)c->status.p, (uint8_t*)c->ftxws.p, s), "launch_filtered");
  HIP_TRY(hipMemcpyAsync(status_out, c->status.p, n_ftx, hipMemcpyDeviceToHost, s), "D2H status");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

// ---------------------------------------------------------------- tear-off building (build_filtered.hip)
static_assert(sizeof(cg_build_totals) == 32, "cg_build_totals layout");

using cg::al256;

static int build_out_args(const char* fn, uint64_t n, const cg::BuildOut& o, bool device) {
  if (n && (!o.ftxs || !o.status || !o.totals)) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  if ((o.node_cap && !o.nodes) || (o.leaf_cap && !o.leaves) || (o.out_cap && !o.out))
    return fail(CG_ERR_ARG, "%s: NULL table", fn);
  if (device && ((uintptr_t)o.out & 15) != 0) return fail(CG_ERR_ARG, "%s: out is not 16-byte aligned", fn);
  return CG_OK;
}

// A host form between its two enqueues: the count pass's totals read back, and the result tables of
// exactly that size in bfio. d: the device-side BuildOut (ftxs, status and totals set by the caller).
static int build_host_tables(cg_ctx* c, const char* fn, const cg::BuildOut& h, cg::BuildOut* d, hipStream_t s) {
  cg_build_totals t;
  HIP_TRY(hipMemcpyAsync(&t, d->totals, sizeof t, hipMemcpyDeviceToHost, s), "D2H totals");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  *h.totals = t;
  if (t.over) {
    char msg[256];
    snprintf(msg, sizeof msg, "a capacity is too small: the call needs %llu node rows, %llu leaf rows, %llu output bytes",
             (unsigned long long)t.n_nodes, (unsigned long long)t.n_leaves, (unsigned long long)t.out_bytes);
    return fail(CG_ERR_ARG, (std::string(fn) + ": %s").c_str(), msg);
  }
  const uint64_t nodes_b = al256(sizeof(cg_pmt_node) * t.n_nodes), leaves_b = al256(sizeof(cg_filtered_leaf) * t.n_leaves);
  HIP_TRY(c->bfio.ensure(nodes_b + leaves_b + t.out_bytes + 256), "hipMalloc(build tables)");
  uint8_t* p = (uint8_t*)c->bfio.p;
  d->nodes = (cg_pmt_node*)p;
  d->leaves = (cg_filtered_leaf*)(p + nodes_b);
  d->out = p + nodes_b + leaves_b;
  d->node_cap = t.n_nodes;
  d->leaf_cap = t.n_leaves;
  d->out_cap = t.out_bytes;
  return CG_OK;
}

static int build_host_results(const cg::BuildOut& h, const cg::BuildOut& d, uint64_t n, hipStream_t s) {
  const cg_build_totals& t = *h.totals;
  HIP_TRY(hipMemcpyAsync(h.ftxs, d.ftxs, sizeof(cg_filtered_tx) * n, hipMemcpyDeviceToHost, s), "D2H ftxs");
  HIP_TRY(hipMemcpyAsync(h.status, d.status, n, hipMemcpyDeviceToHost, s), "D2H status");
  if (t.n_nodes)
    HIP_TRY(hipMemcpyAsync(h.nodes, d.nodes, sizeof(cg_pmt_node) * t.n_nodes, hipMemcpyDeviceToHost, s), "D2H nodes");
  if (t.n_leaves)
    HIP_TRY(hipMemcpyAsync(h.leaves, d.leaves, sizeof(cg_filtered_leaf) * t.n_leaves, hipMemcpyDeviceToHost, s),
            "D2H leaves");
  if (t.out_bytes) HIP_TRY(hipMemcpyAsync(h.out, d.out, t.out_bytes, hipMemcpyDeviceToHost, s), "D2H out");
  return CG_OK;
}

// The part of bfin a host form's fixed-size results take: [ftxs 40 n][status n][totals]
static uint64_t build_fixed_bytes(uint64_t n) { return al256(sizeof(cg_filtered_tx) * n) + al256(n) + 256; }
static void build_fixed_split(uint8_t* p, uint64_t n, cg::BuildOut* d) {
  d->ftxs = (cg_filtered_tx*)p;
  d->status = p + al256(sizeof(cg_filtered_tx) * n);
  d->totals = (cg_build_totals*)(d->status + al256(n));
}

int cg_build_filtered_device(cg_ctx* c, const cg_tx* d_txs, uint64_t n_tx, const cg_component* d_comps,
                             uint64_t n_comps, const uint8_t* d_arena, uint64_t arena_len, const uint8_t* d_visible,
                             uint64_t out_base, cg_filtered_tx* d_ftxs, cg_pmt_node* d_nodes, uint64_t node_cap,
                             cg_filtered_leaf* d_leaves, uint64_t leaf_cap, uint8_t* d_out, uint64_t out_cap,
                             uint8_t* d_status, cg_build_totals* d_totals, void* hip_stream) {
  const char* fn = "cg_build_filtered_device";
  if (!c) return fail(CG_ERR_ARG, "%s: ctx is NULL", fn);
  const cg::BuildOut o{out_base, d_ftxs, d_nodes, node_cap, d_leaves, leaf_cap, d_out, out_cap, d_status, d_totals};
  if (!d_totals) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  if (const int rc = build_out_args(fn, n_tx, o, true)) return rc;
  if (n_tx && (!d_txs || (n_comps && (!d_comps || !d_visible)))) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  const cg::BuildTxIn in{d_txs, n_tx, d_comps, n_comps, d_arena, arena_len, d_visible};
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  HIP_TRY(ensure_all({{&c->aux2, cg::tx_ws_bytes(n_comps)}, {&c->bfws, cg::build_ws_bytes(n_tx, n_comps)}}),
          "hipMalloc(build ws)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(cg::launch_build_filtered_count(in, o, (uint8_t*)c->aux2.p, (uint8_t*)c->bfws.p, call.stream()),
          "launch_build_filtered_count");
  HIP_TRY(cg::launch_build_filtered_emit(in, o, (uint8_t*)c->aux2.p, (uint8_t*)c->bfws.p, call.stream()),
          "launch_build_filtered_emit");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

int cg_build_filtered(cg_ctx* c, const cg_tx* txs, uint64_t n_tx, const cg_component* comps, uint64_t n_comps,
                      const uint8_t* arena, uint64_t arena_len, const uint8_t* visible, uint64_t out_base,
                      cg_filtered_tx* ftxs_out, cg_pmt_node* nodes_out, uint64_t node_cap,
                      cg_filtered_leaf* leaves_out, uint64_t leaf_cap, uint8_t* out, uint64_t out_cap,
                      uint8_t* status_out, cg_build_totals* totals_out) {
  const char* fn = "cg_build_filtered";
  if (!c) return fail(CG_ERR_ARG, "%s: ctx is NULL", fn);
  cg::BuildOut h{out_base, ftxs_out, nodes_out, node_cap, leaves_out, leaf_cap, out, out_cap, status_out, totals_out};
  if (!totals_out) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  if (const int rc = build_out_args(fn, n_tx, h, false)) return rc;
  if (n_tx && (!txs || (n_comps && (!comps || !visible)) || (arena_len && !arena)))
    return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  memset(totals_out, 0, sizeof *totals_out);
  if (n_tx == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->keys, txs, sizeof(cg_tx) * n_tx, s), "H2D txs");
  HIP_TRY(stage(c->items, comps, sizeof(cg_component) * n_comps, s), "H2D comps");
  HIP_TRY(stage(c->arena, arena, arena_len, s, arena_room(arena_len)), "H2D arena");
  const uint64_t vis_b = al256(n_comps ? n_comps : 1);
  HIP_TRY(c->bfin.ensure(vis_b + build_fixed_bytes(n_tx)), "hipMalloc(build inputs)");
  if (n_comps) HIP_TRY(hipMemcpyAsync(c->bfin.p, visible, n_comps, hipMemcpyHostToDevice, s), "H2D visible");
  HIP_TRY(c->aux2.ensure(cg::tx_ws_bytes(n_comps)), "hipMalloc(leaf ws)");
  HIP_TRY(c->bfws.ensure(cg::build_ws_bytes(n_tx, n_comps)), "hipMalloc(build ws)");
  const cg::BuildTxIn in{(const cg_tx*)c->keys.p, n_tx, (const cg_component*)c->items.p, n_comps,
                         (const uint8_t*)c->arena.p, arena_len, (const uint8_t*)c->bfin.p};
  cg::BuildOut d = h;
  d.nodes = nullptr;
  d.leaves = nullptr;
  d.out = nullptr;
  build_fixed_split((uint8_t*)c->bfin.p + vis_b, n_tx, &d);
  HIP_TRY(cg::launch_build_filtered_count(in, d, (uint8_t*)c->aux2.p, (uint8_t*)c->bfws.p, s),
          "launch_build_filtered_count");
  if (const int rc = build_host_tables(c, fn, h, &d, s)) return rc;
  HIP_TRY(cg::launch_build_filtered_emit(in, d, (uint8_t*)c->aux2.p, (uint8_t*)c->bfws.p, s),
          "launch_build_filtered_emit");
  if (const int rc = build_host_results(h, d, n_tx, s)) return rc;
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

int cg_build_partial_trees_device(cg_ctx* c, const uint8_t* d_leaves, uint64_t n_leaf_hashes, const uint64_t* d_first,
                                  const uint32_t* d_count, uint64_t n, uint64_t leaf_total, const uint8_t* d_include,
                                  uint64_t n_inc_hashes, const uint64_t* d_inc_first, const uint32_t* d_inc_count,
                                  uint64_t out_base, cg_filtered_tx* d_ftxs, cg_pmt_node* d_nodes, uint64_t node_cap,
                                  cg_filtered_leaf* d_leaves_out, uint64_t leaf_cap, uint8_t* d_out, uint64_t out_cap,
                                  uint8_t* d_status, cg_build_totals* d_totals, void* hip_stream) {
  const char* fn = "cg_build_partial_trees_device";
  if (!c) return fail(CG_ERR_ARG, "%s: ctx is NULL", fn);
  const cg::BuildOut o{out_base, d_ftxs, d_nodes, node_cap, d_leaves_out, leaf_cap, d_out, out_cap, d_status, d_totals};
  if (!d_totals) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  if (const int rc = build_out_args(fn, n, o, true)) return rc;
  if (n && (!d_first || !d_count || !d_inc_first || !d_inc_count || (n_leaf_hashes && !d_leaves) ||
            (n_inc_hashes && !d_include)))
    return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  if ((((uintptr_t)d_leaves | (uintptr_t)d_include) & 3) != 0)
    return fail(CG_ERR_ARG, "%s: a hash table is not 4-byte aligned", fn);
  const cg::BuildPtIn in{d_leaves, n_leaf_hashes, d_first, d_count, n, leaf_total, d_include, n_inc_hashes,
                         d_inc_first, d_inc_count};
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  HIP_TRY(ensure_all({{&c->bfws, cg::build_pt_ws_bytes(n, leaf_total)}}), "hipMalloc(build ws)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(cg::launch_build_pt_count(in, o, (uint8_t*)c->bfws.p, call.stream()), "launch_build_pt_count");
  HIP_TRY(cg::launch_build_pt_emit(in, o, (uint8_t*)c->bfws.p, call.stream()), "launch_build_pt_emit");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

int cg_build_partial_trees(cg_ctx* c, const uint8_t* leaves, const uint64_t* first, const uint32_t* count, uint64_t n,
                           const uint8_t* include, const uint64_t* inc_first, const uint32_t* inc_count,
                           uint64_t out_base, cg_filtered_tx* ftxs_out, cg_pmt_node* nodes_out, uint64_t node_cap,
                           cg_filtered_leaf* leaves_out, uint64_t leaf_cap, uint8_t* out, uint64_t out_cap,
                           uint8_t* status_out, cg_build_totals* totals_out) {
  const char* fn = "cg_build_partial_trees";
  if (!c) return fail(CG_ERR_ARG, "%s: ctx is NULL", fn);
  cg::BuildOut h{out_base, ftxs_out, nodes_out, node_cap, leaves_out, leaf_cap, out, out_cap, status_out, totals_out};
  if (!totals_out) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  if (const int rc = build_out_args(fn, n, h, false)) return rc;
  if (n && (!first || !count || !inc_first || !inc_count)) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  memset(totals_out, 0, sizeof *totals_out);
  if (n == 0) return CG_OK;
  uint64_t n_leaf_hashes = 0, n_inc_hashes = 0, leaf_total = 0;
  for (uint64_t j = 0; j < n; ++j) {
    if (first[j] + count[j] > n_leaf_hashes) n_leaf_hashes = first[j] + count[j];
    if (inc_first[j] + inc_count[j] > n_inc_hashes) n_inc_hashes = inc_first[j] + inc_count[j];
    leaf_total += count[j];
  }
  if ((n_leaf_hashes && !leaves) || (n_inc_hashes && !include)) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->arena, leaves, 32 * n_leaf_hashes, s), "H2D leaves");
  HIP_TRY(stage(c->aux0, include, 32 * n_inc_hashes, s), "H2D include");
  HIP_TRY(stage(c->keys, first, 8 * n, s), "H2D first");
  HIP_TRY(stage(c->items, count, 4 * n, s), "H2D count");
  HIP_TRY(stage(c->aux1, inc_first, 8 * n, s), "H2D inc_first");
  HIP_TRY(stage(c->aux2, inc_count, 4 * n, s), "H2D inc_count");
  HIP_TRY(c->bfin.ensure(build_fixed_bytes(n)), "hipMalloc(build results)");
  HIP_TRY(c->bfws.ensure(cg::build_pt_ws_bytes(n, leaf_total)), "hipMalloc(build ws)");
  const cg::BuildPtIn in{(const uint8_t*)c->arena.p, n_leaf_hashes, (const uint64_t*)c->keys.p,
                         (const uint32_t*)c->items.p, n, leaf_total, (const uint8_t*)c->aux0.p, n_inc_hashes,
                         (const uint64_t*)c->aux1.p, (const uint32_t*)c->aux2.p};
  cg::BuildOut d = h;
  d.nodes = nullptr;
  d.leaves = nullptr;
  d.out = nullptr;
  build_fixed_split((uint8_t*)c->bfin.p, n, &d);
  HIP_TRY(cg::launch_build_pt_count(in, d, (uint8_t*)c->bfws.p, s), "launch_build_pt_count");
  if (const int rc = build_host_tables(c, fn, h, &d, s)) return rc;
  HIP_TRY(cg::launch_build_pt_emit(in, d, (uint8_t*)c->bfws.p, s), "launch_build_pt_emit");
  if (const int rc = build_host_results(h, d, n, s)) return rc;
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

// ---------------------------------------------------------------- Ed25519 signing (sign_ed.hip)
static_assert(sizeof(cg_sign_req) == 8 && sizeof(cg_sign_item) == 16, "sign request layouts");

// With the ctx lock held. The store: [expanded keys][seeds 32 n][Abytes 32 n]; the seeds are zeroed on
// the stream right behind the expansion.
static int signers_load_locked(cg_ctx* c, const uint8_t* seeds, uint32_t n, uint8_t* pubkeys_out) {
  if (const int rc = enter(c, "cg_signers_load")) return rc;
  signers_drop(c);
  const size_t keys_b = (c->eng->signer_bytes() * n + 255) & ~(size_t)255, seeds_b = 32 * (size_t)n;
  HIP_TRY(c->signers.ensure_exact(keys_b + 2 * seeds_b), "hipMalloc(signers)");
  uint8_t* base = (uint8_t*)c->signers.p;
  uint8_t *d_seeds = base + keys_b, *d_pub = d_seeds + seeds_b;
  hipStream_t s = c->stream;
  hipError_t e;
  {
    Call call(c, Call::kHost);
    e = call.open();
    if (e == hipSuccess) e = hipMemcpyAsync(d_seeds, seeds, seeds_b, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = c->eng->launch_signer_expand(d_seeds, n, base, d_pub, c->btab, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_seeds, 0, seeds_b, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pubkeys_out, d_pub, seeds_b, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = call.close();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) {
    signers_drop(c);  // nothing half-loaded, no seed left behind
    return hip_fail(e, "cg_signers_load");
  }
  c->n_signers = n;
  return CG_OK;
}

int cg_signers_load(cg_ctx* c, const uint8_t* seeds, uint32_t n, uint8_t* pubkeys_out) {
  if (!c) return fail(CG_ERR_ARG, "cg_signers_load: ctx is NULL");
  if (n == 0 || n > CG_SIGNERS_MAX) return fail(CG_ERR_ARG, "cg_signers_load: 1 .. CG_SIGNERS_MAX signers");
  if (!seeds || !pubkeys_out) return fail(CG_ERR_ARG, "cg_signers_load: NULL buffer");
  std::lock_guard<std::mutex> g(c->mu);
  return signers_load_locked(c, seeds, n, pubkeys_out);
}

int cg_signers_clear(cg_ctx* c) {
  if (!c) return fail(CG_ERR_ARG, "cg_signers_clear: ctx is NULL");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
  signers_drop(c);
  return CG_OK;
}

// One sign call: the caller's tables, all in host memory or all in HBM but the templates. `fused`: reqs
// are cg_sign_req over SignableData splices of ids, else cg_sign_item over arena bytes.
struct SignReq {
  const void* reqs;
  uint64_t n;
  bool fused;
  const uint8_t* ids;
  uint64_t n_ids;
  const cg_signable_tmpl* tmpls;
  uint32_t n_tmpls;
  const uint8_t* arena;
  uint64_t arena_len;
  uint8_t* sigs;
  uint8_t* status;
  size_t req_bytes() const { return fused ? sizeof(cg_sign_req) : sizeof(cg_sign_item); }
};

static int sign_args(const char* fn, cg_ctx* c, const SignReq& q, bool host) {
  if (!c) return fail(CG_ERR_ARG, "%s: ctx is NULL", fn);
  if (q.n && (!q.reqs || !q.sigs || !q.status)) return fail(CG_ERR_ARG, "%s: NULL request / signature / status buffer", fn);
  if (q.n_ids && !q.ids) return fail(CG_ERR_ARG, "%s: ids is NULL", fn);
  if (q.n_tmpls && !q.tmpls) return fail(CG_ERR_ARG, "%s: templates is NULL", fn);
  if (q.n_tmpls > 0x10000u) return fail(CG_ERR_ARG, "%s: more than 65536 templates (cg_sign_req.tmpl is 16-bit)", fn);
  if (host && q.arena_len && !q.arena) return fail(CG_ERR_ARG, "%s: arena is NULL", fn);
  return CG_OK;
}

static hipError_t ensure_sign_ws(cg_ctx* c, const SignReq& q, uint64_t slot) {
  return ensure_all({{&c->signws, c->eng->sign_ws_bytes(chunk_of(c, q.n))},
                     {&c->msgs, q.fused ? cg::tx_msgs_head(q.n_tmpls, slot) : 1},
                     {&c->tmpls, sizeof(cg_signable_tmpl) * (q.n_tmpls ? q.n_tmpls : 1)}});
}

// Every launch of a sign call over the device tables `d` on `s`: the templates' images, then each chunk
// of at most the context's chunk items over the one sign workspace, which is zeroed behind the last
// kernel whatever happened before (it holds every r of the last chunk).
static hipError_t launch_sign_call(cg_ctx* c, const SignReq& d, uint64_t slot, hipStream_t s) {
  hipError_t e = hipSuccess;
  const cg_signable_tmpl* dt = (const cg_signable_tmpl*)c->tmpls.p;
  if (d.fused) {
    if (d.n_tmpls) e = hipMemcpyAsync(c->tmpls.p, d.tmpls, sizeof(cg_signable_tmpl) * d.n_tmpls, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = cg::launch_tx_sig_templates(dt, d.n_tmpls, d.arena, d.arena_len, slot, d.ids, d.n_ids, (uint8_t*)c->msgs.p, s);
  }
  const std::vector<uint64_t> bounds = cg::equal_bounds(d.n, chunk_of(c, d.n));
  for (size_t k = 0; e == hipSuccess && k + 1 < bounds.size(); ++k) {
    const uint64_t first = bounds[k], cnt = bounds[k + 1] - first;
    const cg::SignArgs a = {(const uint8_t*)d.reqs + first * d.req_bytes(), cnt, d.fused, c->signers.p, c->n_signers,
                            d.arena, d.arena_len, (const uint8_t*)c->msgs.p, dt, d.n_tmpls, d.n_ids,
                            d.sigs + 64 * first, d.status + first, c->signws.p, c->btab};
    e = c->eng->launch_sign(a, s);
  }
  const hipError_t z = hipMemsetAsync(c->signws.p, 0, c->eng->sign_ws_bytes(chunk_of(c, d.n)), s);
  return e != hipSuccess ? e : z;
}

static int sign_device(const char* fn, cg_ctx* c, const SignReq& d, void* hip_stream) {
  if (const int a = sign_args(fn, c, d, false)) return a;
  if (d.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  if (c->n_signers == 0) return fail(CG_ERR_ARG, "%s: no signers loaded (cg_signers_load)", fn);
  const uint64_t slot = tmpl_slot(d.tmpls, d.n_tmpls);
  HIP_TRY(ensure_sign_ws(c, d, slot), "hipMalloc(sign workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(launch_sign_call(c, d, slot, call.stream()), "launch_sign");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

// A host-buffer sign call with the ctx lock held (cg_sign_tx_ids, cg_sign_batch, the pool form).
static int sign_host_locked(const char* fn, cg_ctx* c, const SignReq& h) {
  if (const int rc = enter(c, fn)) return rc;
  if (c->n_signers == 0) return fail(CG_ERR_ARG, "%s: no signers loaded (cg_signers_load)", fn);
  const uint64_t slot = tmpl_slot(h.tmpls, h.n_tmpls);
  HIP_TRY(ensure_sign_ws(c, h, slot), "hipMalloc(sign workspace)");
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->items, h.reqs, h.req_bytes() * h.n, s), "H2D sign requests");
  HIP_TRY(stage(c->arena, h.arena, h.arena_len, s, arena_room(h.arena_len)), "H2D arena");
  HIP_TRY(stage(c->h_ids, h.ids, 32 * h.n_ids, s), "H2D ids");
  HIP_TRY(c->aux0.ensure(64 * h.n), "hipMalloc(signatures)");
  HIP_TRY(c->status.ensure(h.n), "hipMalloc(status)");
  SignReq d = h;
  d.reqs = c->items.p;
  d.arena = (const uint8_t*)c->arena.p;
  d.ids = (const uint8_t*)c->h_ids.p;
  d.sigs = (uint8_t*)c->aux0.p;
  d.status = (uint8_t*)c->status.p;
  HIP_TRY(launch_sign_call(c, d, slot, s), "launch_sign");
  HIP_TRY(hipMemcpyAsync(h.sigs, d.sigs, 64 * h.n, hipMemcpyDeviceToHost, s), "D2H signatures");
  HIP_TRY(hipMemcpyAsync(h.status, d.status, h.n, hipMemcpyDeviceToHost, s), "D2H status");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

static int sign_host(const char* fn, cg_ctx* c, const SignReq& h) {
  if (const int a = sign_args(fn, c, h, true)) return a;
  if (h.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return sign_host_locked(fn, c, h);
}

int cg_sign_tx_ids(cg_ctx* c, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                   const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                   uint8_t* sigs_out, uint8_t* status_out) {
  return sign_host("cg_sign_tx_ids", c, {reqs, n, true, ids, n_ids, tmpls, n_tmpls, arena, arena_len, sigs_out, status_out});
}

int cg_sign_tx_ids_device(cg_ctx* c, const uint8_t* d_ids, uint64_t n_ids, const cg_sign_req* d_reqs, uint64_t n,
                          const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena, uint64_t arena_len,
                          uint8_t* d_sigs, uint8_t* d_status, void* hip_stream) {
  return sign_device("cg_sign_tx_ids_device", c,
                     {d_reqs, n, true, d_ids, n_ids, tmpls, n_tmpls, d_arena, arena_len, d_sigs, d_status}, hip_stream);
}

int cg_sign_batch(cg_ctx* c, const cg_sign_item* items, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                  uint8_t* sigs_out, uint8_t* status_out) {
  return sign_host("cg_sign_batch", c, {items, n, false, nullptr, 0, nullptr, 0, arena, arena_len, sigs_out, status_out});
}

// ---------------------------------------------------------------- ECDSA signing (sign_ec.hip)
// With the ctx lock held. The store: [signers][d 32 n][schemes n][X || Y 64 n][status n], each part
// 256-aligned; the d bytes are zeroed on the stream right behind the expansion.
static int ec_signers_load_locked(cg_ctx* c, const uint8_t* schemes, const uint8_t* secrets, uint32_t n,
                                  uint8_t* pubs_out, uint8_t* status_out) {
  if (const int rc = enter(c, "cg_ec_signers_load")) return rc;
  ec_signers_drop(c);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t keys_b = al(c->eng->ec_signer_bytes() * n), d_b = 32 * (size_t)n, pub_b = 64 * (size_t)n;
  HIP_TRY(c->ec_signers.ensure_exact(keys_b + al(d_b) + al(n) + al(pub_b) + al(n)), "hipMalloc(ECDSA signers)");
  uint8_t* base = (uint8_t*)c->ec_signers.p;
  uint8_t *d_d = base + keys_b, *d_sch = d_d + al(d_b), *d_pub = d_sch + al(n), *d_st = d_pub + al(pub_b);
  hipStream_t s = c->stream;
  hipError_t e;
  {
    Call call(c, Call::kHost);
    e = call.open();
    if (e == hipSuccess) e = hipMemcpyAsync(d_d, secrets, d_b, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_sch, schemes, n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = c->eng->launch_ec_signer_expand(d_sch, d_d, n, base, d_pub, d_st, c->btab, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_d, 0, d_b, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pubs_out, d_pub, pub_b, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(status_out, d_st, n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = call.close();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) {
    ec_signers_drop(c);  // nothing half-loaded, no d left behind
    return hip_fail(e, "cg_ec_signers_load");
  }
  c->n_ec_signers = n;
  return CG_OK;
}

static int ec_signers_load_args(const char* fn, const uint8_t* schemes, const uint8_t* secrets, uint32_t n,
                                const uint8_t* pubs_out, const uint8_t* status_out) {
  if (n == 0 || n > CG_SIGNERS_MAX) return fail(CG_ERR_ARG, "%s: 1 .. CG_SIGNERS_MAX signers", fn);
  if (!schemes || !secrets || !pubs_out || !status_out) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  return CG_OK;
}

int cg_ec_signers_load(cg_ctx* c, const uint8_t* schemes, const uint8_t* secrets, uint32_t n, uint8_t* pubs_out,
                       uint8_t* status_out) {
  if (!c) return fail(CG_ERR_ARG, "cg_ec_signers_load: ctx is NULL");
  if (const int a = ec_signers_load_args("cg_ec_signers_load", schemes, secrets, n, pubs_out, status_out)) return a;
  std::lock_guard<std::mutex> g(c->mu);
  return ec_signers_load_locked(c, schemes, secrets, n, pubs_out, status_out);
}

int cg_ec_signers_clear(cg_ctx* c) {
  if (!c) return fail(CG_ERR_ARG, "cg_ec_signers_clear: ctx is NULL");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
  ec_signers_drop(c);
  return CG_OK;
}

// One ECDSA sign call: a SignReq (sigs: the 72-byte slots) with the nonces and the length bytes.
struct SignEcReq {
  SignReq q;
  const uint8_t* nonces;
  uint8_t* sig_len;
};

static int sign_ec_args(const char* fn, cg_ctx* c, const SignEcReq& r, bool host) {
  if (const int a = sign_args(fn, c, r.q, host)) return a;
  if (r.q.n && (!r.nonces || !r.sig_len)) return fail(CG_ERR_ARG, "%s: NULL nonce / length buffer", fn);
  return CG_OK;
}

static hipError_t ensure_sign_ec_ws(cg_ctx* c, const SignReq& q, uint64_t slot) {
  return ensure_all({{&c->signecws, c->eng->sign_ec_ws_bytes(chunk_of(c, q.n))},
                     {&c->msgs, q.fused ? cg::tx_msgs_head(q.n_tmpls, slot) : 1},
                     {&c->tmpls, sizeof(cg_signable_tmpl) * (q.n_tmpls ? q.n_tmpls : 1)}});
}

// Every launch of the call over the device tables `r` on `s` (launch_sign_call's shape): the templates'
// images, then each chunk over the one workspace, which is zeroed behind the last kernel whatever happened
// before (it holds the last chunk's k, k G and e).
static hipError_t launch_sign_ec_call(cg_ctx* c, const SignEcReq& r, uint64_t slot, hipStream_t s) {
  const SignReq& d = r.q;
  hipError_t e = hipSuccess;
  const cg_signable_tmpl* dt = (const cg_signable_tmpl*)c->tmpls.p;
  if (d.fused) {
    if (d.n_tmpls) e = hipMemcpyAsync(c->tmpls.p, d.tmpls, sizeof(cg_signable_tmpl) * d.n_tmpls, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = cg::launch_tx_sig_templates(dt, d.n_tmpls, d.arena, d.arena_len, slot, d.ids, d.n_ids, (uint8_t*)c->msgs.p, s);
  }
  const std::vector<uint64_t> bounds = cg::equal_bounds(d.n, chunk_of(c, d.n));
  for (size_t k = 0; e == hipSuccess && k + 1 < bounds.size(); ++k) {
    const uint64_t first = bounds[k], cnt = bounds[k + 1] - first;
    const cg::SignEcArgs a = {(const uint8_t*)d.reqs + first * d.req_bytes(), cnt, d.fused, c->ec_signers.p,
                              c->n_ec_signers, d.arena, d.arena_len, (const uint8_t*)c->msgs.p, dt, d.n_tmpls, d.n_ids,
                              r.nonces + 32 * first, d.sigs + CG_EC_SIG_MAX * first, r.sig_len + first,
                              d.status + first, c->signecws.p, c->btab};
    e = c->eng->launch_sign_ec(a, s);
  }
  const hipError_t z = hipMemsetAsync(c->signecws.p, 0, c->eng->sign_ec_ws_bytes(chunk_of(c, d.n)), s);
  return e != hipSuccess ? e : z;
}

static int sign_ec_device(const char* fn, cg_ctx* c, const SignEcReq& d, void* hip_stream) {
  if (const int a = sign_ec_args(fn, c, d, false)) return a;
  if (d.q.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  if (c->n_ec_signers == 0) return fail(CG_ERR_ARG, "%s: no ECDSA signers loaded (cg_ec_signers_load)", fn);
  const uint64_t slot = tmpl_slot(d.q.tmpls, d.q.n_tmpls);
  HIP_TRY(ensure_sign_ec_ws(c, d.q, slot), "hipMalloc(sign workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(launch_sign_ec_call(c, d, slot, call.stream()), "launch_sign_ec");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

// A host-buffer call with the ctx lock held. Staged in aux0: [signatures 72 n][nonces 32 n][lengths n];
// the staged nonces are zeroed on the stream behind the kernels, whatever happened before.
static int sign_ec_host_locked(const char* fn, cg_ctx* c, const SignEcReq& h) {
  if (const int rc = enter(c, fn)) return rc;
  if (c->n_ec_signers == 0) return fail(CG_ERR_ARG, "%s: no ECDSA signers loaded (cg_ec_signers_load)", fn);
  const SignReq& q = h.q;
  const uint64_t slot = tmpl_slot(q.tmpls, q.n_tmpls);
  HIP_TRY(ensure_sign_ec_ws(c, q, slot), "hipMalloc(sign workspace)");
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->items, q.reqs, q.req_bytes() * q.n, s), "H2D sign requests");
  HIP_TRY(stage(c->arena, q.arena, q.arena_len, s, arena_room(q.arena_len)), "H2D arena");
  HIP_TRY(stage(c->h_ids, q.ids, 32 * q.n_ids, s), "H2D ids");
  HIP_TRY(c->aux0.ensure((CG_EC_SIG_MAX + 32 + 1) * q.n), "hipMalloc(signatures)");
  HIP_TRY(c->status.ensure(q.n), "hipMalloc(status)");
  SignEcReq d = h;
  d.q.reqs = c->items.p;
  d.q.arena = (const uint8_t*)c->arena.p;
  d.q.ids = (const uint8_t*)c->h_ids.p;
  d.q.sigs = (uint8_t*)c->aux0.p;
  d.q.status = (uint8_t*)c->status.p;
  uint8_t* d_nonces = d.q.sigs + CG_EC_SIG_MAX * q.n;
  d.nonces = d_nonces;
  d.sig_len = d_nonces + 32 * q.n;
  hipError_t e = hipMemcpyAsync(d_nonces, h.nonces, 32 * q.n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_sign_ec_call(c, d, slot, s);
  const hipError_t z = hipMemsetAsync(d_nonces, 0, 32 * q.n, s);
  if (e == hipSuccess) e = z;
  HIP_TRY(e, "launch_sign_ec");
  HIP_TRY(hipMemcpyAsync(q.sigs, d.q.sigs, CG_EC_SIG_MAX * q.n, hipMemcpyDeviceToHost, s), "D2H signatures");
  HIP_TRY(hipMemcpyAsync(h.sig_len, d.sig_len, q.n, hipMemcpyDeviceToHost, s), "D2H signature lengths");
  HIP_TRY(hipMemcpyAsync(q.status, d.q.status, q.n, hipMemcpyDeviceToHost, s), "D2H status");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

static int sign_ec_host(const char* fn, cg_ctx* c, const SignEcReq& h) {
  if (const int a = sign_ec_args(fn, c, h, true)) return a;
  if (h.q.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return sign_ec_host_locked(fn, c, h);
}

int cg_ec_sign_tx_ids(cg_ctx* c, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                      const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                      const uint8_t* nonces, uint8_t* sigs_out, uint8_t* sig_len_out, uint8_t* status_out) {
  return sign_ec_host("cg_ec_sign_tx_ids", c,
                      {{reqs, n, true, ids, n_ids, tmpls, n_tmpls, arena, arena_len, sigs_out, status_out}, nonces,
                       sig_len_out});
}

int cg_ec_sign_tx_ids_device(cg_ctx* c, const uint8_t* d_ids, uint64_t n_ids, const cg_sign_req* d_reqs, uint64_t n,
                             const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena, uint64_t arena_len,
                             const uint8_t* d_nonces, uint8_t* d_sigs, uint8_t* d_sig_len, uint8_t* d_status,
                             void* hip_stream) {
  return sign_ec_device("cg_ec_sign_tx_ids_device", c,
                        {{d_reqs, n, true, d_ids, n_ids, tmpls, n_tmpls, d_arena, arena_len, d_sigs, d_status}, d_nonces,
                         d_sig_len}, hip_stream);
}

int cg_ec_sign_batch(cg_ctx* c, const cg_sign_item* items, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                     const uint8_t* nonces, uint8_t* sigs_out, uint8_t* sig_len_out, uint8_t* status_out) {
  return sign_ec_host("cg_ec_sign_batch", c,
                      {{items, n, false, nullptr, 0, nullptr, 0, arena, arena_len, sigs_out, status_out}, nonces,
                       sig_len_out});
}

// ---------------------------------------------------------------- RSA-PSS signing (sign_rsa.hip)
static_assert(sizeof(cg_rsa_signer) == 52, "cg_rsa_signer layout");

// With the ctx lock held. The store: [signer records][cg_rsa_signer table][secret bytes][status n], each
// part 256-aligned; the table and the secret bytes are zeroed on the stream right behind the expansion.
static int rsa_signers_load_locked(cg_ctx* c, const cg_rsa_signer* signers, uint32_t n, const uint8_t* secrets,
                                   uint64_t secrets_len, uint8_t* status_out) {
  if (const int rc = enter(c, "cg_rsa_signers_load")) return rc;
  rsa_signers_drop(c);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t recs_b = al(cg::rsa_signer_bytes() * n), tab_b = al(sizeof(cg_rsa_signer) * (size_t)n),
               sec_b = al(secrets_len + 4);
  HIP_TRY(c->rsa_signers.ensure_exact(recs_b + tab_b + sec_b + al(n)), "hipMalloc(RSA signers)");
  uint8_t* base = (uint8_t*)c->rsa_signers.p;
  uint8_t *d_tab = base + recs_b, *d_sec = d_tab + tab_b, *d_st = d_sec + sec_b;
  hipStream_t s = c->stream;
  hipError_t e;
  {
    Call call(c, Call::kHost);
    e = call.open();
    if (e == hipSuccess) e = hipMemsetAsync(base, 0, recs_b + tab_b + sec_b + al(n), s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab, signers, sizeof(cg_rsa_signer) * (size_t)n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && secrets_len) e = hipMemcpyAsync(d_sec, secrets, secrets_len, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = cg::launch_rsa_signer_expand(d_tab, n, d_sec, secrets_len, base, d_st, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_tab, 0, tab_b + sec_b, s);
    if (e == hipSuccess) e = hipMemcpyAsync(status_out, d_st, n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = call.close();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) {
    rsa_signers_drop(c);  // nothing half-loaded, no secret left behind
    return hip_fail(e, "cg_rsa_signers_load");
  }
  c->n_rsa_signers = n;
  return CG_OK;
}

static int rsa_signers_load_args(const char* fn, const cg_rsa_signer* signers, uint32_t n, const uint8_t* secrets,
                                 uint64_t secrets_len, const uint8_t* status_out) {
  if (n == 0 || n > CG_SIGNERS_MAX) return fail(CG_ERR_ARG, "%s: 1 .. CG_SIGNERS_MAX signers", fn);
  if (!signers || !status_out || (secrets_len && !secrets)) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  if (secrets_len >= (1ull << 32)) return fail(CG_ERR_ARG, "%s: secrets_len must be below 2^32", fn);
  return CG_OK;
}

int cg_rsa_signers_load(cg_ctx* c, const cg_rsa_signer* signers, uint32_t n, const uint8_t* secrets,
                        uint64_t secrets_len, uint8_t* status_out) {
  if (!c) return fail(CG_ERR_ARG, "cg_rsa_signers_load: ctx is NULL");
  if (const int a = rsa_signers_load_args("cg_rsa_signers_load", signers, n, secrets, secrets_len, status_out)) return a;
  std::lock_guard<std::mutex> g(c->mu);
  return rsa_signers_load_locked(c, signers, n, secrets, secrets_len, status_out);
}

int cg_rsa_signers_clear(cg_ctx* c) {
  if (!c) return fail(CG_ERR_ARG, "cg_rsa_signers_clear: ctx is NULL");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
  rsa_signers_drop(c);
  return CG_OK;
}

// One RSA-PSS sign call: a SignReq (sigs: the 512-byte slots) with the salts and the 16-bit lengths.
struct SignRsaReq {
  SignReq q;
  const uint8_t* salts;
  uint16_t* sig_len;
};

static int sign_rsa_args(const char* fn, cg_ctx* c, const SignRsaReq& r, bool host) {
  if (const int a = sign_args(fn, c, r.q, host)) return a;
  if (r.q.n && (!r.salts || !r.sig_len)) return fail(CG_ERR_ARG, "%s: NULL salt / length buffer", fn);
  return CG_OK;
}

static hipError_t ensure_sign_rsa_ws(cg_ctx* c, const SignReq& q, uint64_t slot) {
  return ensure_all({{&c->signrsaws, cg::sign_rsa_ws_bytes(chunk_of(c, q.n))},
                     {&c->msgs, q.fused ? cg::tx_msgs_head(q.n_tmpls, slot) : 1},
                     {&c->tmpls, sizeof(cg_signable_tmpl) * (q.n_tmpls ? q.n_tmpls : 1)}});
}

// Every launch of the call over the device tables `r` on `s` (launch_sign_ec_call's shape); the workspace is
// zeroed behind the last kernel whatever happened before (it holds the last chunk's H and salts).
static hipError_t launch_sign_rsa_call(cg_ctx* c, const SignRsaReq& r, uint64_t slot, hipStream_t s) {
  const SignReq& d = r.q;
  hipError_t e = hipSuccess;
  const cg_signable_tmpl* dt = (const cg_signable_tmpl*)c->tmpls.p;
  if (d.fused) {
    if (d.n_tmpls) e = hipMemcpyAsync(c->tmpls.p, d.tmpls, sizeof(cg_signable_tmpl) * d.n_tmpls, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = cg::launch_tx_sig_templates(dt, d.n_tmpls, d.arena, d.arena_len, slot, d.ids, d.n_ids, (uint8_t*)c->msgs.p, s);
  }
  const std::vector<uint64_t> bounds = cg::equal_bounds(d.n, chunk_of(c, d.n));
  for (size_t k = 0; e == hipSuccess && k + 1 < bounds.size(); ++k) {
    const uint64_t first = bounds[k], cnt = bounds[k + 1] - first;
    const cg::SignRsaArgs a = {(const uint8_t*)d.reqs + first * d.req_bytes(), cnt, d.fused, c->rsa_signers.p,
                               c->n_rsa_signers, d.arena, d.arena_len, (const uint8_t*)c->msgs.p, dt, d.n_tmpls, d.n_ids,
                               r.salts + 32 * first, d.sigs + CG_RSA_SIG_MAX * first, r.sig_len + first,
                               d.status + first, c->signrsaws.p};
    e = cg::launch_sign_rsa(a, s);
  }
  const hipError_t z = hipMemsetAsync(c->signrsaws.p, 0, cg::sign_rsa_ws_bytes(chunk_of(c, d.n)), s);
  return e != hipSuccess ? e : z;
}

static int sign_rsa_device(const char* fn, cg_ctx* c, const SignRsaReq& d, void* hip_stream) {
  if (const int a = sign_rsa_args(fn, c, d, false)) return a;
  if (d.q.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  if (c->n_rsa_signers == 0) return fail(CG_ERR_ARG, "%s: no RSA signers loaded (cg_rsa_signers_load)", fn);
  const uint64_t slot = tmpl_slot(d.q.tmpls, d.q.n_tmpls);
  HIP_TRY(ensure_sign_rsa_ws(c, d.q, slot), "hipMalloc(sign workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(launch_sign_rsa_call(c, d, slot, call.stream()), "launch_sign_rsa");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

// A host-buffer call with the ctx lock held. Staged in aux0: [signatures 512 n][salts 32 n][lengths 2 n];
// the staged salts are zeroed on the stream behind the kernels, whatever happened before.
static int sign_rsa_host_locked(const char* fn, cg_ctx* c, const SignRsaReq& h) {
  if (const int rc = enter(c, fn)) return rc;
  if (c->n_rsa_signers == 0) return fail(CG_ERR_ARG, "%s: no RSA signers loaded (cg_rsa_signers_load)", fn);
  const SignReq& q = h.q;
  const uint64_t slot = tmpl_slot(q.tmpls, q.n_tmpls);
  HIP_TRY(ensure_sign_rsa_ws(c, q, slot), "hipMalloc(sign workspace)");
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  HIP_TRY(stage(c->items, q.reqs, q.req_bytes() * q.n, s), "H2D sign requests");
  HIP_TRY(stage(c->arena, q.arena, q.arena_len, s, arena_room(q.arena_len)), "H2D arena");
  HIP_TRY(stage(c->h_ids, q.ids, 32 * q.n_ids, s), "H2D ids");
  HIP_TRY(c->aux0.ensure((CG_RSA_SIG_MAX + 32 + 2) * q.n), "hipMalloc(signatures)");
  HIP_TRY(c->status.ensure(q.n), "hipMalloc(status)");
  SignRsaReq d = h;
  d.q.reqs = c->items.p;
  d.q.arena = (const uint8_t*)c->arena.p;
  d.q.ids = (const uint8_t*)c->h_ids.p;
  d.q.sigs = (uint8_t*)c->aux0.p;
  d.q.status = (uint8_t*)c->status.p;
  uint8_t* d_salts = d.q.sigs + CG_RSA_SIG_MAX * q.n;
  d.salts = d_salts;
  d.sig_len = (uint16_t*)(d_salts + 32 * q.n);
  hipError_t e = hipMemcpyAsync(d_salts, h.salts, 32 * q.n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_sign_rsa_call(c, d, slot, s);
  const hipError_t z = hipMemsetAsync(d_salts, 0, 32 * q.n, s);
  if (e == hipSuccess) e = z;
  HIP_TRY(e, "launch_sign_rsa");
  HIP_TRY(hipMemcpyAsync(q.sigs, d.q.sigs, CG_RSA_SIG_MAX * q.n, hipMemcpyDeviceToHost, s), "D2H signatures");
  HIP_TRY(hipMemcpyAsync(h.sig_len, d.sig_len, 2 * q.n, hipMemcpyDeviceToHost, s), "D2H signature lengths");
  HIP_TRY(hipMemcpyAsync(q.status, d.q.status, q.n, hipMemcpyDeviceToHost, s), "D2H status");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

static int sign_rsa_host(const char* fn, cg_ctx* c, const SignRsaReq& h) {
  if (const int a = sign_rsa_args(fn, c, h, true)) return a;
  if (h.q.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return sign_rsa_host_locked(fn, c, h);
}

int cg_rsa_sign_tx_ids(cg_ctx* c, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                       const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                       const uint8_t* salts, uint8_t* sigs_out, uint16_t* sig_len_out, uint8_t* status_out) {
  return sign_rsa_host("cg_rsa_sign_tx_ids", c,
                       {{reqs, n, true, ids, n_ids, tmpls, n_tmpls, arena, arena_len, sigs_out, status_out}, salts,
                        sig_len_out});
}

int cg_rsa_sign_tx_ids_device(cg_ctx* c, const uint8_t* d_ids, uint64_t n_ids, const cg_sign_req* d_reqs, uint64_t n,
                              const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena, uint64_t arena_len,
                              const uint8_t* d_salts, uint8_t* d_sigs, uint16_t* d_sig_len, uint8_t* d_status,
                              void* hip_stream) {
  return sign_rsa_device("cg_rsa_sign_tx_ids_device", c,
                         {{d_reqs, n, true, d_ids, n_ids, tmpls, n_tmpls, d_arena, arena_len, d_sigs, d_status}, d_salts,
                          d_sig_len}, hip_stream);
}

int cg_rsa_sign_batch(cg_ctx* c, const cg_sign_item* items, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                      const uint8_t* salts, uint8_t* sigs_out, uint16_t* sig_len_out, uint8_t* status_out) {
  return sign_rsa_host("cg_rsa_sign_batch", c,
                       {{items, n, false, nullptr, 0, nullptr, 0, arena, arena_len, sigs_out, status_out}, salts,
                        sig_len_out});
}

// ---------------------------------------------------------------- key derivation (derive_keys.hip)
static_assert(sizeof(cg_derive_parent) == 16 && sizeof(cg_derive_req) == 16, "derive request layouts");

// One derive call (reqs != null) or public-key call (reqs == null: `secrets` is the input, of `scheme`):
// the caller's tables, all in host memory or all in HBM.
struct DeriveReq {
  const cg_derive_parent* parents;
  uint32_t n_parents;
  const cg_derive_req* reqs;
  uint64_t n;
  const uint8_t* arena;
  uint64_t arena_len;
  uint8_t scheme;
  uint8_t* secrets;
  uint8_t* pubs;
  uint8_t* status;
  uint8_t* retries;  // optional
  bool derives() const { return reqs != nullptr; }
};

static int derive_args(const char* fn, cg_ctx* c, const DeriveReq& q, bool derives, bool host) {
  if (!c) return fail(CG_ERR_ARG, "%s: ctx is NULL", fn);
  if (q.n && (!q.secrets || !q.pubs || !q.status)) return fail(CG_ERR_ARG, "%s: NULL secret / public key / status buffer", fn);
  if (derives) {
    if (q.n && !q.reqs) return fail(CG_ERR_ARG, "%s: requests is NULL", fn);
    if (q.n_parents && !q.parents) return fail(CG_ERR_ARG, "%s: parents is NULL", fn);
    if (host && q.arena_len && !q.arena) return fail(CG_ERR_ARG, "%s: arena is NULL", fn);
  } else if (q.scheme != CG_EDDSA_ED25519_SHA512 && q.scheme != CG_ECDSA_SECP256K1_SHA256 &&
             q.scheme != CG_ECDSA_SECP256R1_SHA256) {
    return fail(CG_ERR_ARG, "%s: this scheme has no key derivation (Crypto.deriveKeyPair: UnsupportedOperationException)", fn);
  }
  return CG_OK;
}

// Every launch of the call over the device tables `d` on `s`: the parents' midstates, then each chunk of
// at most the context's chunk items over the one workspace, which is zeroed behind the last kernel
// whatever happened before (it holds the midstates and the last chunk's d and digits).
static hipError_t launch_derive_call(cg_ctx* c, const DeriveReq& d, hipStream_t s) {
  const uint64_t per = chunk_of(c, d.n);
  cg::DeriveArgs a = {d.parents, d.n_parents, d.reqs,    per,      d.arena,  d.arena_len,   d.scheme,
                      c->derive_force, d.secrets, d.pubs, d.status, d.retries, c->derivews.p, c->btab};
  hipError_t e = d.derives() ? c->eng->launch_derive_parents(a, s) : hipSuccess;
  const std::vector<uint64_t> bounds = cg::equal_bounds(d.n, per);
  for (size_t k = 0; e == hipSuccess && k + 1 < bounds.size(); ++k) {
    const uint64_t first = bounds[k];
    a.n = bounds[k + 1] - first;
    a.d_reqs = d.reqs ? d.reqs + first : nullptr;
    a.d_secrets = d.secrets + 32 * first;
    a.d_pubs = d.pubs + 64 * first;
    a.d_status = d.status + first;
    a.d_retries = d.retries ? d.retries + first : nullptr;
    e = c->eng->launch_derive(a, s);
  }
  const hipError_t z = hipMemsetAsync(c->derivews.p, 0, c->eng->derive_ws_bytes(d.n_parents, per), s);
  return e != hipSuccess ? e : z;
}

static hipError_t ensure_derive_ws(cg_ctx* c, const DeriveReq& q) {
  return ensure_all({{&c->derivews, c->eng->derive_ws_bytes(q.n_parents, chunk_of(c, q.n))}});
}

static int derive_device(const char* fn, cg_ctx* c, const DeriveReq& d, bool derives, void* hip_stream) {
  if (const int a = derive_args(fn, c, d, derives, false)) return a;
  if (d.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (const int rc = enter(c, fn)) return rc;
  HIP_TRY(ensure_derive_ws(c, d), "hipMalloc(derive workspace)");
  Call call(c, Call::kDevice);
  HIP_TRY(call.open(hip_stream), "hipStreamWaitEvent");
  HIP_TRY(launch_derive_call(c, d, call.stream()), "launch_derive");
  HIP_TRY(call.close(), "hipEventRecord");
  return CG_OK;
}

// A host-buffer call with the ctx lock held. Staged on the device: the parents (keys), the requests
// (items), the arena with the parents' key bytes, and [secrets 32 n][pubs 64 n][retries n] (aux0). The
// staged arena and secrets are zeroed on the stream behind the copies back: no key byte stays in HBM.
static int derive_host_locked(const char* fn, cg_ctx* c, const DeriveReq& h) {
  if (const int rc = enter(c, fn)) return rc;
  HIP_TRY(ensure_derive_ws(c, h), "hipMalloc(derive workspace)");
  hipStream_t s = c->stream;
  Call call(c, Call::kHost);
  HIP_TRY(call.open(), "hipStreamWaitEvent");
  DeriveReq d = h;
  HIP_TRY(c->aux0.ensure(97 * h.n), "hipMalloc(derived keys)");
  HIP_TRY(c->status.ensure(h.n), "hipMalloc(status)");
  d.secrets = (uint8_t*)c->aux0.p;
  d.pubs = d.secrets + 32 * h.n;
  d.retries = h.retries ? d.pubs + 64 * h.n : nullptr;
  d.status = (uint8_t*)c->status.p;
  if (h.derives()) {
    HIP_TRY(stage(c->keys, h.parents, sizeof(cg_derive_parent) * (size_t)h.n_parents, s), "H2D parents");
    HIP_TRY(stage(c->items, h.reqs, sizeof(cg_derive_req) * h.n, s), "H2D derive requests");
    HIP_TRY(stage(c->arena, h.arena, h.arena_len, s, arena_room(h.arena_len)), "H2D arena");
    d.parents = (const cg_derive_parent*)c->keys.p;
    d.reqs = (const cg_derive_req*)c->items.p;
    d.arena = (const uint8_t*)c->arena.p;
  } else {
    HIP_TRY(hipMemcpyAsync(d.secrets, h.secrets, 32 * h.n, hipMemcpyHostToDevice, s), "H2D private keys");
  }
  hipError_t e = launch_derive_call(c, d, s);
  if (e == hipSuccess && h.derives()) e = hipMemcpyAsync(h.secrets, d.secrets, 32 * h.n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h.pubs, d.pubs, 64 * h.n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && h.retries) e = hipMemcpyAsync(h.retries, d.retries, h.n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h.status, d.status, h.n, hipMemcpyDeviceToHost, s);
  // the staged secrets, whatever happened before
  const hipError_t z0 = hipMemsetAsync(d.secrets, 0, 32 * h.n, s);
  const hipError_t z1 = h.derives() && h.arena_len ? hipMemsetAsync(c->arena.p, 0, h.arena_len, s) : hipSuccess;
  if (e == hipSuccess) e = z0 != hipSuccess ? z0 : z1;
  HIP_TRY(e, "launch_derive / copies");
  HIP_TRY(call.close(), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return CG_OK;
}

static int derive_host(const char* fn, cg_ctx* c, const DeriveReq& h, bool derives) {
  if (const int a = derive_args(fn, c, h, derives, true)) return a;
  if (h.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(c->mu);
  return derive_host_locked(fn, c, h);
}

int cg_derive_keys(cg_ctx* c, const cg_derive_parent* parents, uint32_t n_parents, const cg_derive_req* reqs, uint64_t n,
                   const uint8_t* arena, uint64_t arena_len, uint8_t* secrets_out, uint8_t* pubs_out,
                   uint8_t* status_out, uint8_t* retries_out) {
  return derive_host("cg_derive_keys", c,
                     {parents, n_parents, reqs, n, arena, arena_len, 0, secrets_out, pubs_out, status_out, retries_out}, true);
}

int cg_derive_keys_device(cg_ctx* c, const cg_derive_parent* d_parents, uint32_t n_parents, const cg_derive_req* d_reqs,
                          uint64_t n, const uint8_t* d_arena, uint64_t arena_len, uint8_t* d_secrets, uint8_t* d_pubs,
                          uint8_t* d_status, uint8_t* d_retries, void* hip_stream) {
  return derive_device("cg_derive_keys_device", c,
                       {d_parents, n_parents, d_reqs, n, d_arena, arena_len, 0, d_secrets, d_pubs, d_status, d_retries},
                       true, hip_stream);
}

int cg_public_keys(cg_ctx* c, uint32_t scheme, const uint8_t* secrets, uint64_t n, uint8_t* pubs_out,
                   uint8_t* status_out) {
  return derive_host("cg_public_keys", c,
                     {nullptr, 0, nullptr, n, nullptr, 0, (uint8_t)(scheme < 256 ? scheme : 0), (uint8_t*)secrets, pubs_out,
                      status_out, nullptr}, false);
}

int cg_public_keys_device(cg_ctx* c, uint32_t scheme, const uint8_t* d_secrets, uint64_t n, uint8_t* d_pubs,
                          uint8_t* d_status, void* hip_stream) {
  return derive_device("cg_public_keys_device", c,
                       {nullptr, 0, nullptr, n, nullptr, 0, (uint8_t)(scheme < 256 ? scheme : 0), (uint8_t*)d_secrets,
                        d_pubs, d_status, nullptr}, false, hip_stream);
}

// ---------------------------------------------------------------- several devices (pool.h)
struct cg_pool {
  std::vector<cg_ctx*> ctx;
  std::vector<uint8_t> healthy;
  std::mutex mu;
};

int cg_pool_open(cg_pool** out, const int32_t* devices, uint32_t n_slots, const cg_config* cfg) {
  if (!out) return fail(CG_ERR_ARG, "cg_pool_open: out is NULL");
  *out = nullptr;
  if (n_slots == 0 || !devices) return fail(CG_ERR_ARG, "cg_pool_open: no devices");
  cg_pool* p = new cg_pool();
  for (uint32_t k = 0; k < n_slots; ++k) {
    cg_config c = cfg ? *cfg : cg_config{};
    c.device = devices[k];
    cg_ctx* x = nullptr;
    const int rc = cg_open(&x, &c);
    if (rc != CG_OK) {
      const std::string why = g_err;
      cg_pool_close(p);
      char buf[64];
      snprintf(buf, sizeof buf, "cg_pool_open: slot %u: ", k);
      g_err = buf + why;
      return rc;
    }
    p->ctx.push_back(x);
    p->healthy.push_back(1);
  }
  *out = p;
  return CG_OK;
}

void cg_pool_close(cg_pool* p) {
  if (!p) return;
  for (cg_ctx* c : p->ctx) cg_close(c);
  delete p;
}

uint32_t cg_pool_slots(const cg_pool* p) { return p ? (uint32_t)p->ctx.size() : 0; }

int cg_pool_slot_healthy(const cg_pool* p, uint32_t slot) {
  if (!p || slot >= p->ctx.size()) return -1;
  return p->healthy[slot] ? 1 : 0;
}

int cg_pool_inject_fault(cg_pool* p, uint32_t slot, int on) {
  if (!p || slot >= p->ctx.size()) return fail(CG_ERR_ARG, "cg_pool_inject_fault: bad slot");
  std::lock_guard<std::mutex> g(p->mu);
  std::lock_guard<std::mutex> gc(p->ctx[slot]->mu);
  p->ctx[slot]->fault = on != 0;
  if (!on) p->healthy[slot] = 1;
  return CG_OK;
}

// pool_run over one shard function; stats and the error message as cg_pool_verify_batch
// with the pool lock held
static int pool_call_locked(cg_pool* p, uint64_t n_items, uint8_t* status_out, cg_pool_stats* stats, const char* name,
                            const std::function<int(cg_ctx*, uint64_t, uint64_t)>& shard) {
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::string> errs(p->ctx.size());
  cg::PoolReport rep;
  const int rc = cg::pool_run(p->healthy, n_items, status_out,
                              [&](uint32_t slot, uint64_t first, uint64_t count) {
                                cg_ctx* c = p->ctx[slot];
                                std::lock_guard<std::mutex> gc(c->mu);
                                const int r = shard(c, first, count);
                                if (r != CG_OK) errs[slot] = g_err;  // g_err is this worker thread's
                                return r;
                              },
                              [&](uint32_t slot) {  // re-probe: no drill fault, the device answers
                                cg_ctx* c = p->ctx[slot];
                                std::lock_guard<std::mutex> gc(c->mu);
                                if (c->fault || hipSetDevice(c->device) != hipSuccess) return false;
                                const hipError_t q = hipStreamQuery(c->stream);
                                return q == hipSuccess || q == hipErrorNotReady;
                              },
                              &rep);
  if (stats) {
    stats->shards = rep.shards;
    stats->reruns = rep.reruns;
    stats->failed_slots = rep.failed_slots;
    stats->reserved = 0;
    stats->not_run = rep.not_run;
    stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (rc != CG_OK) {
    std::string m = std::string(name) + (rc == CG_ERR_DEVICE ? ": no healthy slot could run every shard;"
                                                             : ": a shard failed (not a device fault);");
    for (size_t k = 0; k < errs.size(); ++k)
      if (!errs[k].empty()) m += " [slot " + std::to_string(k) + "] " + errs[k];
    g_err = m;
  }
  return rc;
}
static int pool_call(cg_pool* p, uint64_t n_items, uint8_t* status_out, cg_pool_stats* stats, const char* name,
                     const std::function<int(cg_ctx*, uint64_t, uint64_t)>& shard) {
  std::lock_guard<std::mutex> g(p->mu);
  return pool_call_locked(p, n_items, status_out, stats, name, shard);
}

int cg_pool_verify_tx_signatures(cg_pool* p, const cg_key* keys, uint32_t n_keys, const uint8_t* ids, uint64_t n_ids,
                                 const cg_txsig* sigs, uint64_t n_sigs, const cg_signable_tmpl* tmpls,
                                 uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len, uint32_t mode,
                                 uint8_t* status_out, cg_pool_stats* stats) {
  const char* fn = "cg_pool_verify_tx_signatures";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  const TxsigReq h = {keys,  n_keys,  ids,   n_ids,     {sigs, (uint32_t)sizeof(cg_txsig)}, n_sigs,
                      tmpls, n_tmpls, arena, arena_len, mode,                               status_out};
  int a = txsig_args(fn, p->ctx[0], h);
  if (a == CG_OK) a = txsig_buffer_args(fn, h, true);
  if (a != CG_OK) return a;
  return pool_call(p, n_sigs, status_out, stats, fn, [&](cg_ctx* c, uint64_t first, uint64_t count) {
    TxsigReq shard = h;
    shard.sigs = h.sigs.from(first);
    shard.n_sigs = count;
    shard.status = status_out + first;
    return verify_txsig_host_locked(c, shard, nullptr, nullptr);
  });
}

// The whole call on one live slot (a signature may reference any transaction's id, so the call is not
// sharded): pool_run over a single unit, i.e. the first live slot, and on a device fault the next one.
int cg_pool_verify_transactions(cg_pool* p, const cg_tx* txs, uint64_t n_tx, const cg_component* comps,
                                uint64_t n_comps, const cg_key* keys, uint32_t n_keys, const cg_txsig* sigs,
                                uint64_t n_sigs, const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                uint64_t arena_len, uint32_t mode, uint8_t* ids_out, uint8_t* tx_status_out,
                                uint8_t* sig_status_out, cg_pool_stats* stats) {
  if (!p) return fail(CG_ERR_ARG, "cg_pool_verify_transactions: pool is NULL");
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "cg_pool_verify_transactions: empty pool");
  const TxnReq h = {txs,   n_tx,    comps, n_comps,   keys, n_keys,  sigs,          n_sigs,
                    tmpls, n_tmpls, arena, arena_len, mode, ids_out, tx_status_out, sig_status_out};
  if (const int a = txn_args("cg_pool_verify_transactions", h, true)) return a;
  for (uint64_t i = 0; i < n_sigs; ++i) sig_status_out[i] = CG_NOT_RUN;
  if (n_tx == 0 && n_sigs == 0) return CG_OK;
  uint8_t unit = CG_NOT_RUN;
  const int rc = pool_call(p, 1, &unit, stats, "cg_pool_verify_transactions", [&](cg_ctx* c, uint64_t, uint64_t) {
    const int r = verify_transactions_host_locked(c, h);
    if (r != CG_OK)
      for (uint64_t i = 0; i < n_sigs; ++i) sig_status_out[i] = CG_NOT_RUN;
    return r;
  });
  if (stats) stats->not_run = rc == CG_OK ? 0 : n_sigs;
  return rc;
}

// The signer set on every slot. A slot whose load fails with a device fault is marked unhealthy (it
// holds no set: a later sign call on it is refused, and the pool moves on as for a fault).
int cg_pool_signers_load(cg_pool* p, const uint8_t* seeds, uint32_t n, uint8_t* pubkeys_out) {
  const char* fn = "cg_pool_signers_load";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  if (n == 0 || n > CG_SIGNERS_MAX) return fail(CG_ERR_ARG, "%s: 1 .. CG_SIGNERS_MAX signers", fn);
  if (!seeds || !pubkeys_out) return fail(CG_ERR_ARG, "%s: NULL buffer", fn);
  std::lock_guard<std::mutex> g(p->mu);
  std::vector<uint8_t> pub(32 * (size_t)n);
  bool any = false;
  int last = CG_ERR_DEVICE;
  for (size_t k = 0; k < p->ctx.size(); ++k) {
    cg_ctx* c = p->ctx[k];
    std::lock_guard<std::mutex> gc(c->mu);
    const bool drill = c->fault;  // the drill fails every call; the set is loaded all the same, for the
    c->fault = false;             // moment the drill is cleared
    const int rc = signers_load_locked(c, seeds, n, any ? pub.data() : pubkeys_out);
    c->fault = drill;
    if (rc == CG_OK) any = true;
    else if (rc == CG_ERR_DEVICE) p->healthy[k] = 0;
    if (rc != CG_OK) last = rc;
  }
  return any ? CG_OK : last;
}

int cg_pool_signers_clear(cg_pool* p) {
  if (!p) return fail(CG_ERR_ARG, "cg_pool_signers_clear: pool is NULL");
  std::lock_guard<std::mutex> g(p->mu);
  for (cg_ctx* c : p->ctx) {
    std::lock_guard<std::mutex> gc(c->mu);
    if (hipSetDevice(c->device) == hipSuccess) signers_drop(c);
  }
  return CG_OK;
}

// The whole call on one live slot, and on a device fault the next one (cg_pool_verify_transactions'
// pattern: pool_run over a single unit).
int cg_pool_sign_tx_ids(cg_pool* p, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                        const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                        uint8_t* sigs_out, uint8_t* status_out, cg_pool_stats* stats) {
  const char* fn = "cg_pool_sign_tx_ids";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  const SignReq h = {reqs, n, true, ids, n_ids, tmpls, n_tmpls, arena, arena_len, sigs_out, status_out};
  if (const int a = sign_args(fn, p->ctx[0], h, true)) return a;
  if (n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(p->mu);  // one scope: the signer sets cannot change between the check and the call
  bool any = false;
  for (cg_ctx* c : p->ctx) {
    std::lock_guard<std::mutex> gc(c->mu);
    any = any || c->n_signers != 0;
  }
  // no signers anywhere: the caller's mistake, and nothing is written
  if (!any) return fail(CG_ERR_ARG, "%s: no signers loaded (cg_pool_signers_load)", fn);
  auto blank = [&]() {
    memset(status_out, CG_NOT_RUN, n);
    memset(sigs_out, 0, 64 * n);
  };
  blank();
  uint8_t unit = CG_NOT_RUN;
  const int rc = pool_call_locked(p, 1, &unit, stats, fn, [&](cg_ctx* c, uint64_t, uint64_t) {
    // a slot whose load failed holds no set: it refuses the call as a slot without capacity does
    // (pool.h: the call moves to the next live slot, the slot's health is untouched)
    if (!c->fault && c->n_signers == 0) return fail(CG_ERR_NOMEM, "%s: this slot holds no signer set (its load failed)", fn);
    const int r = sign_host_locked(fn, c, h);
    if (r != CG_OK) blank();
    return r;
  });
  if (stats) stats->not_run = rc == CG_OK ? 0 : n;
  return rc;
}

// The ECDSA signer set on every slot, and cg_ec_sign_tx_ids whole on one live slot (the three calls above).
int cg_pool_ec_signers_load(cg_pool* p, const uint8_t* schemes, const uint8_t* secrets, uint32_t n, uint8_t* pubs_out,
                            uint8_t* status_out) {
  const char* fn = "cg_pool_ec_signers_load";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  if (const int a = ec_signers_load_args(fn, schemes, secrets, n, pubs_out, status_out)) return a;
  std::lock_guard<std::mutex> g(p->mu);
  std::vector<uint8_t> pub(64 * (size_t)n), st(n);
  bool any = false;
  int last = CG_ERR_DEVICE;
  for (size_t k = 0; k < p->ctx.size(); ++k) {
    cg_ctx* c = p->ctx[k];
    std::lock_guard<std::mutex> gc(c->mu);
    const bool drill = c->fault;  // as cg_pool_signers_load: loaded all the same, for the moment the
    c->fault = false;             // drill is cleared
    const int rc = ec_signers_load_locked(c, schemes, secrets, n, any ? pub.data() : pubs_out, any ? st.data() : status_out);
    c->fault = drill;
    if (rc == CG_OK) any = true;
    else if (rc == CG_ERR_DEVICE) p->healthy[k] = 0;
    if (rc != CG_OK) last = rc;
  }
  return any ? CG_OK : last;
}

int cg_pool_ec_signers_clear(cg_pool* p) {
  if (!p) return fail(CG_ERR_ARG, "cg_pool_ec_signers_clear: pool is NULL");
  std::lock_guard<std::mutex> g(p->mu);
  for (cg_ctx* c : p->ctx) {
    std::lock_guard<std::mutex> gc(c->mu);
    if (hipSetDevice(c->device) == hipSuccess) ec_signers_drop(c);
  }
  return CG_OK;
}

int cg_pool_ec_sign_tx_ids(cg_pool* p, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                           const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                           const uint8_t* nonces, uint8_t* sigs_out, uint8_t* sig_len_out, uint8_t* status_out,
                           cg_pool_stats* stats) {
  const char* fn = "cg_pool_ec_sign_tx_ids";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  const SignEcReq h = {{reqs, n, true, ids, n_ids, tmpls, n_tmpls, arena, arena_len, sigs_out, status_out}, nonces,
                       sig_len_out};
  if (const int a = sign_ec_args(fn, p->ctx[0], h, true)) return a;
  if (n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(p->mu);  // one scope: the signer sets cannot change between the check and the call
  bool any = false;
  for (cg_ctx* c : p->ctx) {
    std::lock_guard<std::mutex> gc(c->mu);
    any = any || c->n_ec_signers != 0;
  }
  if (!any) return fail(CG_ERR_ARG, "%s: no ECDSA signers loaded (cg_pool_ec_signers_load)", fn);
  auto blank = [&]() {
    memset(status_out, CG_NOT_RUN, n);
    memset(sigs_out, 0, CG_EC_SIG_MAX * n);
    memset(sig_len_out, 0, n);
  };
  blank();
  uint8_t unit = CG_NOT_RUN;
  const int rc = pool_call_locked(p, 1, &unit, stats, fn, [&](cg_ctx* c, uint64_t, uint64_t) {
    if (!c->fault && c->n_ec_signers == 0) return fail(CG_ERR_NOMEM, "%s: this slot holds no signer set (its load failed)", fn);
    const int r = sign_ec_host_locked(fn, c, h);
    if (r != CG_OK) blank();
    return r;
  });
  if (stats) stats->not_run = rc == CG_OK ? 0 : n;
  return rc;
}

// The RSA signer set on every slot, and cg_rsa_sign_tx_ids whole on one live slot (as the ECDSA forms above).
int cg_pool_rsa_signers_load(cg_pool* p, const cg_rsa_signer* signers, uint32_t n, const uint8_t* secrets,
                             uint64_t secrets_len, uint8_t* status_out) {
  const char* fn = "cg_pool_rsa_signers_load";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  if (const int a = rsa_signers_load_args(fn, signers, n, secrets, secrets_len, status_out)) return a;
  std::lock_guard<std::mutex> g(p->mu);
  std::vector<uint8_t> st(n);
  bool any = false;
  int last = CG_ERR_DEVICE;
  for (size_t k = 0; k < p->ctx.size(); ++k) {
    cg_ctx* c = p->ctx[k];
    std::lock_guard<std::mutex> gc(c->mu);
    const bool drill = c->fault;  // as cg_pool_signers_load: loaded all the same, for the moment the
    c->fault = false;             // drill is cleared
    const int rc = rsa_signers_load_locked(c, signers, n, secrets, secrets_len, any ? st.data() : status_out);
    c->fault = drill;
    if (rc == CG_OK) any = true;
    else if (rc == CG_ERR_DEVICE) p->healthy[k] = 0;
    if (rc != CG_OK) last = rc;
  }
  return any ? CG_OK : last;
}

int cg_pool_rsa_signers_clear(cg_pool* p) {
  if (!p) return fail(CG_ERR_ARG, "cg_pool_rsa_signers_clear: pool is NULL");
  std::lock_guard<std::mutex> g(p->mu);
  for (cg_ctx* c : p->ctx) {
    std::lock_guard<std::mutex> gc(c->mu);
    if (hipSetDevice(c->device) == hipSuccess) rsa_signers_drop(c);
  }
  return CG_OK;
}

int cg_pool_rsa_sign_tx_ids(cg_pool* p, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                            const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                            const uint8_t* salts, uint8_t* sigs_out, uint16_t* sig_len_out, uint8_t* status_out,
                            cg_pool_stats* stats) {
  const char* fn = "cg_pool_rsa_sign_tx_ids";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  const SignRsaReq h = {{reqs, n, true, ids, n_ids, tmpls, n_tmpls, arena, arena_len, sigs_out, status_out}, salts,
                        sig_len_out};
  if (const int a = sign_rsa_args(fn, p->ctx[0], h, true)) return a;
  if (n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(p->mu);  // one scope: the signer sets cannot change between the check and the call
  bool any = false;
  for (cg_ctx* c : p->ctx) {
    std::lock_guard<std::mutex> gc(c->mu);
    any = any || c->n_rsa_signers != 0;
  }
  if (!any) return fail(CG_ERR_ARG, "%s: no RSA signers loaded (cg_pool_rsa_signers_load)", fn);
  auto blank = [&]() {
    memset(status_out, CG_NOT_RUN, n);
    memset(sigs_out, 0, CG_RSA_SIG_MAX * n);
    memset(sig_len_out, 0, 2 * n);
  };
  blank();
  uint8_t unit = CG_NOT_RUN;
  const int rc = pool_call_locked(p, 1, &unit, stats, fn, [&](cg_ctx* c, uint64_t, uint64_t) {
    if (!c->fault && c->n_rsa_signers == 0) return fail(CG_ERR_NOMEM, "%s: this slot holds no signer set (its load failed)", fn);
    const int r = sign_rsa_host_locked(fn, c, h);
    if (r != CG_OK) blank();
    return r;
  });
  if (stats) stats->not_run = rc == CG_OK ? 0 : n;
  return rc;
}

// cg_derive_keys / cg_public_keys whole on one live slot, and on a device fault the next one
// (cg_pool_sign_tx_ids' pattern).
static int pool_derive(const char* fn, cg_pool* p, const DeriveReq& h, bool derives, cg_pool_stats* stats) {
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  if (const int a = derive_args(fn, p->ctx[0], h, derives, true)) return a;
  if (h.n == 0) return CG_OK;
  std::lock_guard<std::mutex> g(p->mu);
  auto blank = [&]() {
    memset(h.status, CG_NOT_RUN, h.n);
    if (derives) memset(h.secrets, 0, 32 * h.n);
    memset(h.pubs, 0, 64 * h.n);
    if (h.retries) memset(h.retries, 0, h.n);
  };
  blank();
  uint8_t unit = CG_NOT_RUN;
  const int rc = pool_call_locked(p, 1, &unit, stats, fn, [&](cg_ctx* c, uint64_t, uint64_t) {
    const int r = derive_host_locked(fn, c, h);
    if (r != CG_OK) blank();
    return r;
  });
  if (stats) stats->not_run = rc == CG_OK ? 0 : h.n;
  return rc;
}

int cg_pool_derive_keys(cg_pool* p, const cg_derive_parent* parents, uint32_t n_parents, const cg_derive_req* reqs,
                        uint64_t n, const uint8_t* arena, uint64_t arena_len, uint8_t* secrets_out, uint8_t* pubs_out,
                        uint8_t* status_out, uint8_t* retries_out, cg_pool_stats* stats) {
  return pool_derive("cg_pool_derive_keys", p,
                     {parents, n_parents, reqs, n, arena, arena_len, 0, secrets_out, pubs_out, status_out, retries_out}, true,
                     stats);
}

int cg_pool_public_keys(cg_pool* p, uint32_t scheme, const uint8_t* secrets, uint64_t n, uint8_t* pubs_out,
                        uint8_t* status_out, cg_pool_stats* stats) {
  return pool_derive("cg_pool_public_keys", p,
                     {nullptr, 0, nullptr, n, nullptr, 0, (uint8_t)(scheme < 256 ? scheme : 0), (uint8_t*)secrets, pubs_out,
                      status_out, nullptr}, false, stats);
}

int cg_pool_verify_tx_signatures_packed(cg_pool* p, const cg_key* keys, uint32_t n_keys, const uint8_t* ids,
                                        uint64_t n_ids, const cg_txsig_packed* sigs, uint64_t n_sigs,
                                        const uint8_t* sig_bytes, uint64_t sig_bytes_len,
                                        const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                        uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                                        cg_pool_stats* stats) {
  const char* fn = "cg_pool_verify_tx_signatures_packed";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  const TxsigReq h = {keys,    n_keys, ids,       n_ids, {sigs, (uint32_t)sizeof(cg_txsig_packed)}, n_sigs,    tmpls,
                      n_tmpls, arena,  arena_len, mode,  status_out, sig_bytes, 0, sig_bytes_len};
  int a = txsig_args(fn, p->ctx[0], h);
  if (a == CG_OK) a = txsig_buffer_args(fn, h, true);
  if (a != CG_OK) return a;
  // a shard [first, first + count) starts at the stream offset of record `first`: the sum of the spans
  // before it, in one threaded pass over the table (a prefix per 2^16-record block), looked up per shard
  const uint64_t B = 1u << 16, nb = (n_sigs + B - 1) / B;
  std::vector<uint64_t> blk(nb + 1, 0);
  {
    const unsigned nt = std::max(1u, std::min<unsigned>(16, (unsigned)nb));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
      th.emplace_back([&, t] {
        for (uint64_t b = nb * t / nt; b < nb * (t + 1) / nt; ++b) {
          uint64_t sp = 0;
          for (uint64_t i = b * B; i < std::min(n_sigs, (b + 1) * B); ++i) sp += ((uint64_t)sigs[i].sig_len + 3u) & ~(uint64_t)3;
          blk[b + 1] = sp;
        }
      });
    for (std::thread& x : th) x.join();
    for (uint64_t b = 0; b < nb; ++b) blk[b + 1] += blk[b];
  }
  auto stream_at = [&](uint64_t i) {
    uint64_t o = blk[i / B];
    for (uint64_t j = (i / B) * B; j < i; ++j) o += ((uint64_t)sigs[j].sig_len + 3u) & ~(uint64_t)3;
    return o;
  };
  return pool_call(p, n_sigs, status_out, stats, fn, [&](cg_ctx* c, uint64_t first, uint64_t count) {
    const uint64_t o = std::min(stream_at(first), sig_bytes_len);
    TxsigReq shard = h;
    shard.sigs = h.sigs.from(first);
    shard.n_sigs = count;
    shard.status = status_out + first;
    shard.sig_bytes = sig_bytes + o;
    shard.sig_bytes_len = sig_bytes_len - o;
    return verify_txsig_host_locked(c, shard, nullptr, nullptr);
  });
}

int cg_pool_verify_required_signatures_packed(cg_pool* p, const cg_key* keys, uint32_t n_keys, const uint8_t* ids,
                                              uint64_t n_ids, const cg_txsig_packed* sigs, uint64_t n_sigs,
                                              const uint8_t* sig_bytes, uint64_t sig_bytes_len,
                                              const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                              uint64_t arena_len, uint32_t mode, const uint32_t* key_class,
                                              const cg_tx_check* checks, uint64_t n_tx, const uint32_t* reqs,
                                              uint32_t n_reqs, const cg_req_node* nodes, uint32_t n_nodes,
                                              uint8_t* status_out, cg_tx_verdict* verdicts_out,
                                              uint8_t* req_status_out, cg_pool_stats* stats) {
  const char* fn = "cg_pool_verify_required_signatures_packed";
  if (!p) return fail(CG_ERR_ARG, "%s: pool is NULL", fn);
  if (p->ctx.empty()) return fail(CG_ERR_ARG, "%s: empty pool", fn);
  const cg::SigTable table = {sigs, (uint32_t)sizeof(cg_txsig_packed)};
  const cg::TxvSet h = {key_class, checks, n_tx, reqs, n_reqs, nodes, n_nodes, verdicts_out, req_status_out};
  int a = txv_args(fn, table, n_sigs, sigs, n_keys, keys, h);
  if (a == CG_OK) a = txv_reserved(fn, h);
  if (a != CG_OK) return a;
  std::vector<uint8_t> own;
  if (!status_out && n_sigs) {
    own.assign(n_sigs, CG_NOT_RUN);
    status_out = own.data();
  }
  // the existing pool call: shards, re-run on a fault; what no slot ran stays CG_NOT_RUN
  const int rc = cg_pool_verify_tx_signatures_packed(p, keys, n_keys, ids, n_ids, sigs, n_sigs, sig_bytes, sig_bytes_len,
                                                     tmpls, n_tmpls, arena, arena_len, mode, status_out, stats);
  if (rc != CG_OK && rc != CG_ERR_DEVICE) {
    txv_fill_not_run(h);
    return rc;
  }
  if (n_tx == 0 && n_reqs == 0) return rc;
  const std::string first_err = rc != CG_OK ? g_err : std::string();
  // the reduction over the gathered statuses, on the first slot that runs it
  int vr = CG_ERR_DEVICE;
  {
    std::lock_guard<std::mutex> g(p->mu);
    for (size_t k = 0; k < p->ctx.size() && vr != CG_OK; ++k) {
      if (!p->healthy[k]) continue;
      cg_ctx* c = p->ctx[k];
      std::lock_guard<std::mutex> gc(c->mu);
      vr = tx_verdicts_host_locked(c, table, n_sigs, status_out, keys, n_keys, h);
      if (vr == CG_ERR_DEVICE) p->healthy[k] = 0;
      else if (vr != CG_OK) break;
    }
  }
  if (vr != CG_OK) {
    if (vr == CG_ERR_DEVICE && g_err.empty()) g_err = std::string(fn) + ": no healthy slot could run the reduction";
    txv_fill_not_run(h);
    return vr;
  }
  if (rc != CG_OK) g_err = first_err;
  return rc;
}

int cg_pool_verify_batch(cg_pool* p, const cg_key* keys, uint32_t n_keys, const cg_item* items, uint64_t n_items,
                         const uint8_t* arena, uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                         cg_pool_stats* stats) {
  if (!p) return fail(CG_ERR_ARG, "cg_pool_verify_batch: pool is NULL");
  const cg::VerifyReq h = {keys, n_keys, items, n_items, arena, arena_len, mode, status_out};
  if (const int a = batch_args("cg_pool_verify_batch", h, true)) return a;
  return pool_call(p, n_items, status_out, stats, "cg_pool_verify_batch", [&](cg_ctx* c, uint64_t first, uint64_t count) {
    cg::VerifyReq shard = h;  // the items and the status bytes narrowed
    shard.d_items = items + first;
    shard.n_items = count;
    shard.d_status = status_out + first;
    return verify_host_locked(c, shard, nullptr);
  });
}

}  // extern "C"
