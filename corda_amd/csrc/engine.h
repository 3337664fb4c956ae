// Internal interface between the C ABI host code (cordagpu.cpp) and the HIP kernels.
#pragma once
#include <functional>
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/cordagpu.h"
#include "launch_schedule.h"

// Types shared by every build of the kernels. The radix-dependent translation units (verify.hip,
// verify_ed.hip, verify_ec.hip, plan_sort.hip) are compiled once per fixed-base table radix, the extra
// builds with `cg` renamed (Makefile VARIANTS: -Dcg=cg24 / -Dcg=cg22), so these types live in a
// namespace the rename does not touch and the C ABI layer hands the same objects to any build.
namespace cgt {


struct DeviceConsts;  // opaque
// The wide-table pools of a call (keyws.h EdWideSlot / EcWideSlot arrays; host-allocated), one per
// scheme family; caps 0 = no key gets wide tables.
struct WidePool {
  void* ed = nullptr;
  void* ec = nullptr;
  uint32_t cap_ed = 0, cap_ec = 0;
  uint32_t min_ed = 0, min_ec = 0;  // items per key from which a key gets wide tables, per family
  // The pools are laid out by `slots`, the capacity they were allocated for (a slot's address does
  // not move between calls); cap_ed / cap_ec only limit how many keys may be wide in this call.
  uint32_t slots = 0;
  // The context's wide-table cache (key_cache.h; keyws.h KeyCache lays it out): null = off, every
  // call builds the tables of its wide keys. cache_dirty: empty it at the start of this call.
  void* cache = nullptr;
  uint32_t cache_bits = 32;  // home entries of the cache's index: 2^bits (tests narrow it)
  bool cache_dirty = false;
};

// Side streams + events owned by a context. Key preparation forks off the caller's stream:
// the two ECDSA curves' tables and the Ed25519 row tables are built on side streams (each is a
// latency-bound chain of doublings on few waves), while the caller's stream goes on with the
// work that needs only decoded keys (the plan, the SHA-512 challenges). Each consumer waits
// for its `ready` event just before it reads tables: ready[0] secp256r1, [1] secp256k1,
// [2] Ed25519.
// Key prep fork: side[0] / side[1] build the secp256r1 / secp256k1 keys (decode -> chain -> tab),
// side[2] the Ed25519 keys; `start` orders them after the main stream's earlier work,
// ready[c] is what the ladders on the main stream wait for.
// Item stages: each curve's ECDSA front runs on its side stream (after its decode there, between
// ec_front_go and ec_front_done[c]) beside the challenge hashes on the main stream. The row-0
// ladders (keys with few items, keyws.h) run on the side stream that built their class's tables,
// after `front` (the hashes on the main stream), while the main stream runs the full-table
// ladders; the Ed25519 finish follows on side[2]; the main stream joins on row0[k]. A few row-0
// waves (long: 252 doublings) then overlap the full-table launch instead of trailing it.
// Per-stage timing (cg_config.flags & CG_FLAG_STAGE_TIMING): a pair of events around each stage's
// launches, recorded on the stream the stage runs on, so a stage's duration is measured where it
// ran even when other stages overlap it on other streams. Read (and reset) with cg_stage_times.
struct StageTimer {
  struct Rec {
    int stage;
    hipEvent_t a, b;
  };
  // At most kMaxRecs launches are recorded between two cg_stage_times calls (later launches are
  // not timed); event pairs are recycled through `spare`, so a context that never reads its stage
  // times holds a bounded number of events.
  static constexpr size_t kMaxRecs = 4096;
  std::vector<Rec> recs, spare;
  int mark(int stage, hipStream_t s) {
    if (recs.size() >= kMaxRecs) return -1;
    Rec r{stage, nullptr, nullptr};
    if (!spare.empty()) {
      r.a = spare.back().a;
      r.b = spare.back().b;
      spare.pop_back();
    } else {
      if (hipEventCreate(&r.a) != hipSuccess) return -1;
      if (hipEventCreate(&r.b) != hipSuccess) {
        (void)hipEventDestroy(r.a);
        return -1;
      }
    }
    (void)hipEventRecord(r.a, s);
    recs.push_back(r);
    return (int)recs.size() - 1;
  }
  void done(int idx, hipStream_t s) {
    if (idx >= 0) (void)hipEventRecord(recs[idx].b, s);
  }
};
#define CG_TIME(fork, stage, stream, launch)                                   \
  do {                                                                          \
    const int _t = (fork).timer ? (fork).timer->mark((stage), (stream)) : -1;  \
    launch;                                                                     \
    if (_t >= 0) (fork).timer->done(_t, (stream));                             \
  } while (0)

// Key-table builds deferred by launch_keyprep until the first chunk's plan is sorted (the sort's
// decoupled look-back stalls when the table builds hold the SIMDs), then enqueued by launch_items.
// The schedule's part (launch_schedule.h Pending: deferred or not, which families need row-0 / full
// tables (false only when the host counts prove none does: KeyUses::host_counts), the skip mask) and
// what the builds' launchers need.
struct PendingTabs : cgs::Pending {
  const cg_key* keys = nullptr;
  uint32_t n_keys = 0;
  void* keyprep = nullptr;
  WidePool wide;
};

struct Fork {
  hipStream_t side[3];
  hipEvent_t start, ready[3], front, row0[3];
  StageTimer* timer;  // null unless the ctx was opened with CG_FLAG_STAGE_TIMING
  hipEvent_t planned = nullptr;  // plan sorted (main): the deferred table builds fork from it
  // ECDSA fronts on side[k]: main's plan done / curve k's front done
  hipEvent_t ec_front_go = nullptr, ec_front_done[2] = {nullptr, nullptr};
  mutable PendingTabs pending;
  hipEvent_t mark = nullptr;  // CG_HOST_TRACE: recorded on the main stream before a back's final joins
  // Host hook launch_items_front runs once between a chunk's plan and its hashes (the host
  // tx-signature path copies the chunk's signature bytes there, after its plan is enqueued)
  const std::function<hipError_t()>* mid_front = nullptr;
};

// A signature table in either record form: `stride` is sizeof(cg_txsig) or sizeof(cg_txsig_packed).
struct SigTable {
  const void* p = nullptr;
  uint32_t stride = sizeof(cg_txsig);
  bool packed() const { return stride == sizeof(cg_txsig_packed); }
  SigTable from(uint64_t first) const { return {(const uint8_t*)p + first * stride, stride}; }  // records first, first + 1, ...
};
// f(the table's records, typed by its stride)
template <class F>
auto with_records(const SigTable& t, F&& f) {
  return !t.packed() ? f((const cg_txsig*)t.p) : f((const cg_txsig_packed*)t.p);
}

// One verify call as its caller states it: the key table, the items, the arena, the mode and the
// status bytes, plus the engine's spliced-message workspace (d_msgs / msgs_len: read by items flagged
// CG_ITEM_MSG_WS (keyws.h); caller items never carry that flag). Every other field is required.
struct VerifyReq {
  const cg_key* d_keys;
  uint32_t n_keys;
  const cg_item* d_items;
  uint64_t n_items;
  const uint8_t* d_arena;
  uint64_t arena_len;
  uint32_t mode;
  uint8_t* d_status;
  const uint8_t* d_msgs = nullptr;
  uint64_t msgs_len = 0;
};

// What the item stages of one chunk read and write: the request narrowed to the chunk's items and
// status bytes, the call's workspaces and the chunk's item workspace. Every field is required but
// `wide` (null: no key of the call has wide tables).
struct ItemArgs : VerifyReq {
  const void* d_keyprep;
  void* d_item_ws;
  const void* d_btab;
  const WidePool* wide;
};

// Where the per-key use counts come from when there is no verify-item table yet: a signature table
// in HBM (sampled on the device) or exact counts (n_keys u32 in HBM, made by the host).
struct KeyUses {
  SigTable sigs;
  const uint32_t* counts = nullptr;
  uint64_t n = 0;  // signatures the counts cover (sizes the wide pools)
  // optional host copies of the key table and of `counts` (the host-buffer tx-signature path): the
  // host then knows, as k_key_classify will, which families need row-0 / full tables
  const cg_key* host_keys = nullptr;
  const uint32_t* host_counts = nullptr;
};

// One chunk of an Ed25519 sign call (sign_ed.hip): the chunk's requests (cg_sign_req over SignableData
// splices when `fused`, else cg_sign_item over arena bytes), the context's signer store, and the chunk's
// signature and status bytes. d_ws holds sign_ws_bytes(n) bytes; d_msgs / d_tmpls (fused only) are the
// splice workspace launch_tx_sig_templates made and the template table it was made from.
struct SignArgs {
  const void* d_reqs;
  uint64_t n;
  bool fused;
  const void* d_signers;
  uint32_t n_signers;
  const uint8_t* d_arena;
  uint64_t arena_len;
  const uint8_t* d_msgs;
  const cg_signable_tmpl* d_tmpls;
  uint32_t n_tmpls;
  uint64_t n_ids;
  uint8_t* d_sigs;
  uint8_t* d_status;
  void* d_ws;
  const void* d_btab;
};

// One chunk of an ECDSA sign call (sign_ec.hip): SignArgs' request forms over the context's ECDSA signer
// store, the chunk's nonces (32 bytes per request) and its 72-byte signature slots, length and status
// bytes. d_ws holds sign_ec_ws_bytes(n) bytes.
struct SignEcArgs {
  const void* d_reqs;
  uint64_t n;
  bool fused;
  const void* d_signers;
  uint32_t n_signers;
  const uint8_t* d_arena;
  uint64_t arena_len;
  const uint8_t* d_msgs;
  const cg_signable_tmpl* d_tmpls;
  uint32_t n_tmpls;
  uint64_t n_ids;
  const uint8_t* d_nonces;
  uint8_t* d_sigs;
  uint8_t* d_sig_len;
  uint8_t* d_status;
  void* d_ws;
  const void* d_btab;
};

// One chunk of an RSA-PSS sign call (sign_rsa.hip): SignArgs' request forms over the context's RSA signer
// store, the chunk's salts (32 bytes per request) and its 512-byte signature slots, 16-bit lengths and
// status bytes. d_ws holds sign_rsa_ws_bytes(n) bytes.
struct SignRsaArgs {
  const void* d_reqs;
  uint64_t n;
  bool fused;
  const void* d_signers;
  uint32_t n_signers;
  const uint8_t* d_arena;
  uint64_t arena_len;
  const uint8_t* d_msgs;
  const cg_signable_tmpl* d_tmpls;
  uint32_t n_tmpls;
  uint64_t n_ids;
  const uint8_t* d_salts;
  uint8_t* d_sigs;
  uint16_t* d_sig_len;
  uint8_t* d_status;
  void* d_ws;
};

// One chunk of a key-derivation call (derive_keys.hip). With d_reqs: cg_derive_keys, d_secrets is
// written. Without: cg_public_keys, d_secrets holds the private keys of `scheme` and is only read.
// d_ws holds derive_ws_bytes(n_parents, n) bytes and starts with the call's parent midstates
// (launch_derive_parents, once per call, before the chunks).
struct DeriveArgs {
  const cg_derive_parent* d_parents;
  uint32_t n_parents;
  const cg_derive_req* d_reqs;
  uint64_t n;
  const uint8_t* d_arena;
  uint64_t arena_len;
  uint8_t scheme;
  uint32_t force_retries;  // CG_TEST_DERIVE_FORCE_RETRIES
  uint8_t* d_secrets;
  uint8_t* d_pubs;
  uint8_t* d_status;
  uint8_t* d_retries;  // optional
  void* d_ws;
  const void* d_btab;
};

// One build of the radix-dependent kernels: the entry points cordagpu.cpp calls through a context's
// variant (cg_config.table_bytes_max picks it at cg_open). Each build defines cg::variant() (renamed
// cg24::variant() / cg22::variant() in the others).
struct EngineVariant {
  uint32_t fixed_base_bits;  // radix 2^bits of the constant B / G tables
  hipError_t (*upload_constants)();
  size_t (*keyprep_bytes)(uint32_t n_keys);
  size_t (*wide_bytes)(uint32_t n_keys, uint64_t n_items, uint32_t max_slots);
  size_t (*wide_slot_bytes)();
  WidePool (*make_wide_pool)(void* base, uint32_t n_keys, uint64_t n_items, uint32_t max_slots, uint32_t alloc_slots);
  uint32_t (*wide_slots)(uint32_t n_keys, uint64_t n_items, uint32_t max_slots);
  size_t (*key_cache_bytes)(uint32_t slots);
  size_t (*btab_bytes)();
  size_t (*btab_scratch_bytes)();
  hipError_t (*init_btab)(void* d_btab, void* d_scratch, hipStream_t stream);
  size_t (*item_ws_bytes)(uint64_t n_items);
  hipError_t (*launch_keyprep)(const VerifyReq& r, void* d_keyprep, hipStream_t stream, const Fork& fork,
                               const WidePool* wide, const KeyUses* src);
  hipError_t (*launch_key_tables)(const Fork& fork, hipStream_t stream);
  hipError_t (*launch_items)(const ItemArgs& a, hipStream_t stream, const Fork& fork);
  hipError_t (*launch_items_plan)(const ItemArgs& a, hipStream_t stream, const Fork& fork);
  hipError_t (*launch_items_front)(const ItemArgs& a, hipStream_t stream, const Fork& fork, bool planned);
  hipError_t (*launch_items_back)(const ItemArgs& a, hipStream_t stream, const Fork& fork);
  // the Ed25519 signer (sign_ed.hip)
  size_t (*signer_bytes)();
  size_t (*sign_ws_bytes)(uint64_t n);
  hipError_t (*launch_signer_expand)(const uint8_t* d_seeds, uint32_t n, void* d_signers, uint8_t* d_pubkeys,
                                     const void* d_btab, hipStream_t stream);
  hipError_t (*launch_sign)(const SignArgs& a, hipStream_t stream);
  // key derivation (derive_keys.hip)
  size_t (*derive_ws_bytes)(uint32_t n_parents, uint64_t n);
  hipError_t (*launch_derive_parents)(const DeriveArgs& a, hipStream_t stream);
  hipError_t (*launch_derive)(const DeriveArgs& a, hipStream_t stream);
  // the ECDSA signer (sign_ec.hip)
  size_t (*ec_signer_bytes)();
  size_t (*sign_ec_ws_bytes)(uint64_t n);
  hipError_t (*launch_ec_signer_expand)(const uint8_t* d_schemes, const uint8_t* d_secrets, uint32_t n, void* d_signers,
                                        uint8_t* d_pubs, uint8_t* d_status, const void* d_btab, hipStream_t stream);
  hipError_t (*launch_sign_ec)(const SignEcArgs& a, hipStream_t stream);
};

}  // namespace cgt

namespace cg {

using cgt::DeriveArgs;
using cgt::EngineVariant;
using cgt::Fork;
using cgt::ItemArgs;
using cgt::PendingTabs;
using cgt::SignArgs;
using cgt::SignEcArgs;
using cgt::SignRsaArgs;
using cgt::SigTable;
using cgt::StageTimer;
using cgt::VerifyReq;
using cgt::WidePool;
using cgt::with_records;

// this build's entry points (verify.hip)
const EngineVariant& variant();

// Upload the constant tables (curve constants, base-point tables) for the current device.
hipError_t upload_constants();

// Bytes of per-key workspace for n_keys keys.
size_t keyprep_bytes(uint32_t n_keys);
// Wide-table pools for a call of n_items over n_keys (keyws.h: keys with many items get one table
// row per radix-2^8 digit): bytes, and the pool view over `base` (caps 0 when nothing can be wide).
size_t wide_bytes(uint32_t n_keys, uint64_t n_items, uint32_t max_slots = 8192u);
size_t wide_slot_bytes();  // one Ed25519 + one ECDSA wide slot
constexpr uint32_t kKeyWideMax = 8192u;  // keyws.h KEY_WIDE_MAX (static_assert in verify.hip)
// alloc_slots: the slots the buffer at `base` was allocated for (0: as many as this call may use)
WidePool make_wide_pool(void* base, uint32_t n_keys, uint64_t n_items, uint32_t max_slots = 8192u,
                        uint32_t alloc_slots = 0);
uint32_t wide_slots(uint32_t n_keys, uint64_t n_items, uint32_t max_slots);  // slots such a call may use
size_t key_cache_bytes(uint32_t slots);  // the wide-table cache's bookkeeping for a pool of `slots` slots

// Constant base-point row table: size and one-time initialisation (per context).
size_t btab_bytes();
size_t btab_scratch_bytes();  // temporary scratch of init_btab (free once it has run)
hipError_t init_btab(void* d_btab, void* d_scratch, hipStream_t stream);
// Bytes of per-item workspace (projective Ed25519 results awaiting the batched inversion).
size_t item_ws_bytes(uint64_t n_items);
using cgt::KeyUses;
// The key tables of r's keys. With `src`, or else with r.d_items, each key's table is sized by the
// number of items that use it (keyws.h; `src` when the items are not made yet: r.d_items is then not
// read); with neither (cg_prepare_keys_device), every key gets full tables.
hipError_t launch_keyprep(const VerifyReq& r, void* d_keyprep, hipStream_t stream, const Fork& fork,
                          const WidePool* wide, const KeyUses* src);
// Start the table builds launch_keyprep deferred (no-op if already started): a host-buffer call
// starts them before it blocks on the first chunk's arena copy, so they overlap that copy.
hipError_t launch_key_tables(const Fork& fork, hipStream_t stream);
// The item stages of one chunk: launch_items_front, then launch_items_back.
hipError_t launch_items(const ItemArgs& a, hipStream_t stream, const Fork& fork);
// launch_items in two halves: the front (status checks, plan sort, challenge hashes, ECDSA prep and
// s^-1: needs only the decoded keys) and the back (ladders, finish: need the key tables). Between the
// two a caller with a second item workspace may enqueue the next chunk's front, so the first chunk's
// wait for the key tables is spent on the second chunk's fronts (cordagpu.cpp launch_chunked).
// The front's plan sort can be enqueued on its own first (`planned` = true then skips it in the
// front): onesweep's decoupled look-back stalls when the table builds hold the SIMDs, so a caller
// with two chunks sorts both before the first front starts the table builds.
hipError_t launch_items_plan(const ItemArgs& a, hipStream_t stream, const Fork& fork);
hipError_t launch_items_front(const ItemArgs& a, hipStream_t stream, const Fork& fork, bool planned);
hipError_t launch_items_back(const ItemArgs& a, hipStream_t stream, const Fork& fork);

// The Ed25519 signer (sign_ed.hip; EdDSAEngine.engineSign behind Crypto.doSign). The signer store holds
// signer_bytes() per signer (launch_signer_expand fills it from the 32-byte seeds and writes each key's
// 32-byte Abyte to d_pubkeys); launch_sign signs one chunk over a workspace of sign_ws_bytes(n) bytes,
// which holds secrets (every r and its table digits) until the caller zeroes it.
size_t signer_bytes();
size_t sign_ws_bytes(uint64_t n);
hipError_t launch_signer_expand(const uint8_t* d_seeds, uint32_t n, void* d_signers, uint8_t* d_pubkeys,
                                const void* d_btab, hipStream_t stream);
hipError_t launch_sign(const SignArgs& a, hipStream_t stream);

// Key derivation (derive_keys.hip; Crypto.deriveKeyPair). launch_derive_parents fills the head of the
// workspace (derive_ws_bytes(n_parents, n) bytes: the parents' HMAC midstates, then one chunk's slots)
// once per call, launch_derive runs one chunk over it. The workspace holds secrets (midstates, d, the
// digits) until the caller zeroes it. derive_upload_constants: this translation unit's curve constants.
hipError_t derive_upload_constants();
size_t derive_ws_bytes(uint32_t n_parents, uint64_t n);
hipError_t launch_derive_parents(const DeriveArgs& a, hipStream_t stream);
hipError_t launch_derive(const DeriveArgs& a, hipStream_t stream);

// The ECDSA signer (sign_ec.hip; BC's ECDSASigner.generateSignature behind Crypto.doSign, k given by the
// caller). The signer store holds ec_signer_bytes() per signer (launch_ec_signer_expand fills it from the
// scheme bytes and the 32-byte big-endian d, and writes X || Y and a load status per signer);
// launch_sign_ec signs one chunk over a workspace of sign_ec_ws_bytes(n) bytes, which holds secrets (every
// k and its k G) until the caller zeroes it. sign_ec_upload_constants: this translation unit's curve
// constants.
hipError_t sign_ec_upload_constants();
size_t ec_signer_bytes();
size_t sign_ec_ws_bytes(uint64_t n);
hipError_t launch_ec_signer_expand(const uint8_t* d_schemes, const uint8_t* d_secrets, uint32_t n, void* d_signers,
                                   uint8_t* d_pubs, uint8_t* d_status, const void* d_btab, hipStream_t stream);
hipError_t launch_sign_ec(const SignEcArgs& a, hipStream_t stream);

// RSA_SHA256 (verify_rsa.hip; radix-independent, used only by contexts opened with CG_FLAG_RSA).
// Key records for a key table (launch_rsa_keyprep fills them: accepted keys get their Montgomery
// constants, every other key a "not accepted" mark), and one pass over a call's items after its
// ladders: the items whose key was accepted are listed on the device (d_rsalist: the count, then the
// list; rsa_list_bytes) and verified, overwriting the CG_UNSUPPORTED k_misc_status gave them. Nothing
// comes back to the host. Calls of more than kRsaSegment items run the pass per segment.
constexpr uint64_t kRsaSegment = 1ull << 30;
size_t rsa_keys_bytes(uint32_t n_keys);
size_t rsa_list_bytes(uint64_t n_items);
hipError_t launch_rsa_keyprep(const VerifyReq& r, void* d_rsakeys, hipStream_t stream);
hipError_t launch_rsa_items(const VerifyReq& r, const void* d_rsakeys, void* d_rsalist, hipStream_t stream);

// The RSA-PSS signer (sign_rsa.hip; BC's PSSSigner.generateSignature behind Crypto.doSign, the salt given by
// the caller; radix-independent). The signer store holds rsa_signer_bytes() per signer
// (launch_rsa_signer_expand fills it from the cg_rsa_signer table and the staged secret bytes, which must be
// readable to secrets_len rounded up to 4, and writes a load status per signer); launch_sign_rsa signs one
// chunk over a workspace of sign_rsa_ws_bytes(n) bytes, which holds secrets (H and the salt of every
// request) until the caller zeroes it.
size_t rsa_signer_bytes();
size_t sign_rsa_ws_bytes(uint64_t n);
hipError_t launch_rsa_signer_expand(const void* d_signers_in, uint32_t n, const uint8_t* d_secrets, uint64_t secrets_len,
                                    void* d_store, uint8_t* d_status, hipStream_t stream);
hipError_t launch_sign_rsa(const SignRsaArgs& a, hipStream_t stream);

// Hashing kernels
hipError_t launch_sha256(const cg_span* d_spans, uint64_t n, const uint8_t* d_arena, uint64_t arena_len,
                         uint8_t* d_out, hipStream_t stream);
hipError_t launch_sha512(const cg_span* d_spans, uint64_t n, const uint8_t* d_arena, uint64_t arena_len,
                         uint8_t* d_out, hipStream_t stream);

// WireTransaction ids: leaf hashing + per-tx Merkle levels. `d_leaf_ws` must hold
// tx_ws_bytes(n_comps) bytes.
// workspace sections start 256-aligned
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t tx_ws_bytes(uint64_t n_comps);
// The workspace's component -> transaction map (0xffffffff: no transaction claims the component).
uint32_t* tx_ws_map(uint8_t* d_leaf_ws, uint64_t n_comps);
// launch_tx_ids without the roots: statuses and the leaf hashes, 8 big-endian words at
// d_leaf_ws[32 * component] (build_filtered.hip walks them).
hipError_t launch_tx_leaves(const cg_tx* d_txs, uint64_t n_tx, const cg_component* d_comps, uint64_t n_comps,
                            const uint8_t* d_arena, uint64_t arena_len, uint8_t* d_status, uint8_t* d_leaf_ws,
                            hipStream_t stream);
hipError_t launch_tx_ids(const cg_tx* d_txs, uint64_t n_tx, const cg_component* d_comps, uint64_t n_comps,
                         const uint8_t* d_arena, uint64_t arena_len, uint8_t* d_ids, uint8_t* d_status,
                         uint8_t* d_leaf_ws, hipStream_t stream);

// Transaction pipeline: per-signature verify items over SignableData splices. d_msgs (the message
// workspace, tx_msgs_head(n_tmpls, slot) bytes) holds the splice header, the templates' SHA-256
// midstates and their images (`slot` bytes each, a multiple of 16); no message is materialised.
uint64_t tx_msgs_head(uint32_t n_tmpls, uint64_t slot);
hipError_t launch_tx_sig_items(const cg_txsig* d_sigs, uint64_t n_sigs, const cg_signable_tmpl* d_tmpls,
                               uint32_t n_tmpls, const uint8_t* d_tx_status, uint64_t n_tx, const uint8_t* d_ids,
                               const uint8_t* d_arena, uint64_t arena_len, uint64_t slot, cg_item* d_items,
                               uint8_t* d_msgs, hipStream_t stream);
// The same in two steps: the templates' midstates + images once per call (tx_sig_templates), then
// any contiguous range [first, first + n) of the signatures (tx_sig_range: its verify items and
// spliced messages; every signature keeps its own message slot).
hipError_t launch_tx_sig_templates(const cg_signable_tmpl* d_tmpls, uint32_t n_tmpls, const uint8_t* d_arena,
                                   uint64_t arena_len, uint64_t slot, const uint8_t* d_ids, uint64_t n_ids,
                                   uint8_t* d_msgs, hipStream_t stream);
hipError_t launch_tx_sig_range(const cg_txsig* d_sigs, uint64_t first, uint64_t n, const cg_signable_tmpl* d_tmpls,
                               uint32_t n_tmpls, const uint8_t* d_tx_status, uint64_t n_tx, const uint8_t* d_ids,
                               uint64_t arena_len, uint64_t slot, cg_item* d_items, uint8_t* d_msgs,
                               hipStream_t stream);

// The 12-byte signature table (cg_txsig_packed): records [first, first + n) become verify items like
// launch_tx_sig_range's, each signature's offset recovered by a prefix scan of round_up(sig_len, 4):
// per 256-record block sums, an exclusive scan of those, then each block's own scan in the item kernel.
// Signature j sits at sig_region + (offset of j in the signature stream) in the arena; one that runs
// past sig_bytes_len of the stream gets CG_NOT_RUN. Either
// `d_bases` holds the stream offset of every 256-record block of the whole table (tx_sig12_bases over
// [0, n_all); `first` must then be a multiple of 256), or the range's blocks are summed and scanned
// here, starting at stream offset `base`, into d_scratch (tx_sig12_scratch_bytes(n) bytes).
size_t tx_sig12_scratch_bytes(uint64_t n);
hipError_t launch_tx_sig12_bases(const cg_txsig_packed* d_sigs, uint64_t first, uint64_t n, uint64_t base,
                                 uint64_t* d_bases, hipStream_t stream);
hipError_t launch_tx_sig12_range(const cg_txsig_packed* d_sigs, uint64_t first, uint64_t n, uint64_t sig_region,
                                 uint64_t sig_bytes_len, uint64_t base, const uint64_t* d_bases,
                                 const cg_signable_tmpl* d_tmpls,
                                 uint32_t n_tmpls, uint64_t n_tx, uint64_t arena_len, cg_item* d_items,
                                 void* d_scratch, hipStream_t stream);

// Merkle roots over independent leaf lists.
hipError_t launch_merkle_roots(const uint8_t* d_leaves, const uint64_t* d_first, const uint32_t* d_count,
                               uint64_t n, uint8_t* d_roots, uint8_t* d_status, uint8_t* d_ws,
                               const uint64_t* d_wsoff, hipStream_t stream);

// Tear-offs (filtered.hip): leaf hashes, then one lane per filtered transaction. `d_ws` must
// hold ftx_ws_bytes(n_leaves) bytes.
size_t ftx_ws_bytes(uint64_t n_leaves);
hipError_t launch_filtered(const cg_filtered_tx* d_ftxs, uint64_t n_ftx, const cg_pmt_node* d_nodes, uint64_t n_nodes,
                           const cg_filtered_leaf* d_leaves, uint64_t n_leaves, const uint8_t* d_arena,
                           uint64_t arena_len, uint8_t* d_status, uint8_t* d_ws, hipStream_t stream);

// Tear-off building (build_filtered.hip). Each form is two enqueues, so that a host form can read the
// totals in between: count (the leaf stages, the count walk, the scan: d_totals is complete behind it)
// and emit (the tables). BuildOut: the caller's tables and capacities. `d_ws` must hold
// build_ws_bytes(n_tx, n_comps) resp. build_pt_ws_bytes(n, leaf_total) bytes, `d_leaf_ws`
// tx_ws_bytes(n_comps).
struct BuildOut {
  uint64_t out_base;
  cg_filtered_tx* ftxs;
  cg_pmt_node* nodes;
  uint64_t node_cap;
  cg_filtered_leaf* leaves;
  uint64_t leaf_cap;
  uint8_t* out;
  uint64_t out_cap;
  uint8_t* status;
  cg_build_totals* totals;
};
struct BuildTxIn {
  const cg_tx* txs;
  uint64_t n_tx;
  const cg_component* comps;
  uint64_t n_comps;
  const uint8_t* arena;
  uint64_t arena_len;
  const uint8_t* visible;
};
struct BuildPtIn {
  const uint8_t* leaves;
  uint64_t n_leaf_hashes;
  const uint64_t* first;
  const uint32_t* count;
  uint64_t n;
  uint64_t leaf_total;
  const uint8_t* include;
  uint64_t n_inc_hashes;
  const uint64_t* inc_first;
  const uint32_t* inc_count;
};
size_t build_ws_bytes(uint64_t n_tx, uint64_t n_comps);
hipError_t launch_build_filtered_count(const BuildTxIn& in, const BuildOut& o, uint8_t* d_leaf_ws, uint8_t* d_ws,
                                       hipStream_t stream);
hipError_t launch_build_filtered_emit(const BuildTxIn& in, const BuildOut& o, uint8_t* d_leaf_ws, uint8_t* d_ws,
                                      hipStream_t stream);
size_t build_pt_ws_bytes(uint64_t n, uint64_t leaf_total);
hipError_t launch_build_pt_count(const BuildPtIn& in, const BuildOut& o, uint8_t* d_ws, hipStream_t stream);
hipError_t launch_build_pt_emit(const BuildPtIn& in, const BuildOut& o, uint8_t* d_ws, hipStream_t stream);


// Per-transaction verdicts (txverdict.hip). One call's tables and results, all on one side of the bus:
// the caller's (host or device) or the context's staged copies.
struct TxvSet {
  const uint32_t* key_class = nullptr;
  const cg_tx_check* checks = nullptr;
  uint64_t n_tx = 0;  // below 2^32 (the entry points check)
  const uint32_t* reqs = nullptr;
  uint32_t n_reqs = 0;
  const cg_req_node* nodes = nullptr;
  uint32_t n_nodes = 0;
  cg_tx_verdict* verdicts = nullptr;
  uint8_t* req_status = nullptr;
};
// req_status preset to CG_REQ_HOST, then the lane-per-transaction kernel and the wave-per-transaction
// kernel over the list it leaves in d_ws (tx_verdicts_ws_bytes(n_tx) bytes).
size_t tx_verdicts_ws_bytes(uint64_t n_tx);
hipError_t launch_tx_verdicts(const SigTable& d_sigs, uint64_t n_sigs, const uint8_t* d_status, const cg_key* d_keys,
                              uint32_t n_keys, const TxvSet& d, void* d_ws, hipStream_t stream);

}  // namespace cg
