// The launch schedule of the verify calls, with no HIP in it: which stage goes to which of the four
// streams, in what order, and which event records and stream waits order them. verify.hip and
// cordagpu.cpp instantiate it over HIP (thin tables from these enums to streams, events and
// launchers); tests/native/launch_schedule_test.cpp instantiates exactly this code over a fake that
// logs every call, and tests/test_launch_schedule.py audits the logs for stream races (DESIGN.md,
// "The launch schedule").
//
// Two levels, as the code is layered:
//   Schedule<Ops>   one engine build's key preparation and item stages (verify.hip)
//   chunked / prepare_keys / verify_items over an Eng   a call's sequencing (cordagpu.cpp)
//
// Ops: type Error, constant kOk, and
//   Error record(Event, Stream); Error wait(Stream, Event);
//   Error run(Stage, Stream, int chunk, int half);   (chunk / half -1: a whole-call key stage)
//   bool mid_hook();       a host hook is waiting for the next front (Fork::mid_front)
//   void before_joins();   a trace marker ahead of a back's final joins (Fork::mark)
#pragma once

namespace cgs {

enum Stream { MAIN, SIDE0, SIDE1, SIDE2, kStreams };  // SIDEk: family k (0 secp256r1, 1 secp256k1, 2 Ed25519)

enum Event {
  EV_START,          // MAIN: use counts and classification done, the side streams fork
  EV_PLANNED,        // MAIN: the deferred table builds fork
  EV_READY0, EV_READY1, EV_READY2,  // SIDEk: family k's tables built
  EV_FRONT,          // MAIN: twice per back (hashes done; Ed25519 ladders done)
  EV_ROW0_0, EV_ROW0_1, EV_ROW0_2,  // SIDEk: the chunk's work there done
  EV_EC_FRONT_GO,    // MAIN: the chunk is planned
  EV_EC_FRONT_DONE0, EV_EC_FRONT_DONE1,  // SIDEk: curve k's front done
  kEvents
};

// One value per launcher group that goes to one stream in one go. The per-family groups are
// consecutive in side-stream order, so family k's is Stage(ST_..._R1 + k).
enum Stage {
  ST_KEY_INIT, ST_KEY_USES, ST_KEY_COUNTS, ST_KEY_USES_TXSIG, ST_KC_BEGIN, ST_KEY_CLASSIFY, ST_KC_CLAIM,
  ST_CHAINS_R1, ST_CHAINS_K1, ST_CHAINS_ED,
  ST_WIDE_TABS_R1, ST_WIDE_TABS_K1, ST_WIDE_TABS_ED,  // with the cache's commit
  ST_FULL_TABS_R1, ST_FULL_TABS_K1, ST_FULL_TABS_ED,  // full / quarter / row-0 tables
  ST_ED_ABYTE,
  ST_MISC_STATUS, ST_PLAN,
  ST_EC_FRONT_R1, ST_EC_FRONT_K1, ST_ED_FRONT,
  ST_ROW0_LADDER_R1, ST_ROW0_LADDER_K1, ST_ROW0_LADDER_ED,
  ST_FULL_LADDER_R1, ST_FULL_LADDER_K1, ST_FULL_LADDER_ED,
  ST_WIDE_LADDER_R1, ST_WIDE_LADDER_K1, ST_WIDE_LADDER_ED,
  ST_ED_FINISH, ST_MODE_GUARD,
  ST_RSA_KEYPREP, ST_RSA_ITEMS,
  ST_PREPARE_HOOK, ST_MID_HOOK,  // host hooks of the tx-signature forms, opaque, on MAIN
  ST_NONE,
  kStages = ST_NONE
};

inline Stream side(int k) { return Stream(SIDE0 + k); }
inline Event ready(int k) { return Event(EV_READY0 + k); }
inline Event row0(int k) { return Event(EV_ROW0_0 + k); }
inline Stage stage(Stage r1, int k) { return Stage(r1 + k); }

// What the schedule keeps from a call's key preparation for its item stages, and for the item
// stages of a later call (cg_prepare_keys_device + cg_verify_items_device).
struct Pending {
  bool on = false;  // the table builds are deferred until the first front
  // per family: whether any key of it gets row-0 / quarter / full tables; false only when the
  // host counts prove none does, so the near-empty launches do not queue behind the wide builds
  bool need_full[3] = {true, true, true};
  unsigned skip_mask = 0;  // bit f: !need_full[f] (k_key_classify checks it, k_mode_guard enforces it)
  bool wide_ed = false, wide_ec = false;  // the deferred builds' wide pools have slots
};

// A call's key preparation as the host knows it.
struct KeyPlan {
  bool any_keys = true;
  Stage uses = ST_NONE;  // ST_KEY_USES, ST_KEY_COUNTS, ST_KEY_USES_TXSIG, or none
  bool counted = true;   // tables sized by the call's key uses (else every key gets full tables, now)
  bool cache = false;    // the wide-table cache is on
  bool wide_ed = false, wide_ec = false;
  bool need_full[3] = {true, true, true};
};

// One chunk's item stages: its number, the item workspace it uses, and whether the pools have slots.
struct Chunk {
  int chunk = 0, half = 0;
  bool wide_ed = false, wide_ec = false;
};

template <class Ops>
class Schedule {
 public:
  using Error = typename Ops::Error;
  Schedule(Ops& ops, Pending& p) : ops_(ops), p_(p) {}

  // The key tables of a call: use counts, classification and the cache's passes on MAIN, then the
  // fork: each family's decode and row-base chains on its side stream. The table builds follow at
  // once for an uncounted call, else with the first front (or key_tables()). Abyte stays on MAIN.
  Error keyprep(const KeyPlan& k) {
    // a call with no keys must not inherit the previous call's skip (k_mode_guard reads it)
    p_.skip_mask = 0;
    for (int f = 0; f < 3; ++f) p_.need_full[f] = true;
    if (!k.any_keys) return Ops::kOk;
    for (int f = 0; f < 3; ++f) {
      p_.need_full[f] = k.need_full[f];
      if (!k.need_full[f]) p_.skip_mask |= 1u << f;
    }
    run(ST_KEY_INIT, MAIN);
    if (k.uses != ST_NONE) run(k.uses, MAIN);
    if (k.cache) run(ST_KC_BEGIN, MAIN);
    run(ST_KEY_CLASSIFY, MAIN);
    if (k.cache) run(ST_KC_CLAIM, MAIN);
    Error e = ops_.record(EV_START, MAIN);
    for (int s = 0; s < 3 && e == Ops::kOk; ++s) e = ops_.wait(side(s), EV_START);
    if (e != Ops::kOk) return e;
    for (int s = 0; s < 3; ++s) run(stage(ST_CHAINS_R1, s), side(s));
    p_.on = true;
    p_.wide_ed = k.wide_ed;
    p_.wide_ec = k.wide_ec;
    if (!k.counted) e = key_tables();
    if (e != Ops::kOk) return e;
    run(ST_ED_ABYTE, MAIN);
    return Ops::kOk;
  }

  // The deferred table builds, forked from MAIN at this point (no-op if already started): Ed25519
  // first (its ladder runs first); per family the wide tables, then the full / row-0 ones, behind
  // the family's own chains and waiting for no other family.
  Error key_tables() {
    if (!p_.on) return Ops::kOk;
    p_.on = false;
    Error e = ops_.record(EV_PLANNED, MAIN);
    if (e != Ops::kOk) return e;
    static const int order[3] = {2, 0, 1};
    for (int k : order) {
      e = ops_.wait(side(k), EV_PLANNED);
      if (e != Ops::kOk) return e;
      if (k == 2 ? p_.wide_ed : p_.wide_ec) run(stage(ST_WIDE_TABS_R1, k), side(k));
      if (p_.need_full[k]) run(stage(ST_FULL_TABS_R1, k), side(k));
      e = ops_.record(ready(k), side(k));
      if (e != Ops::kOk) return e;
    }
    return e;
  }

  Error items_plan(const Chunk& c) {
    ops_.run(ST_MISC_STATUS, MAIN, c.chunk, c.half);
    return ops_.run(ST_PLAN, MAIN, c.chunk, c.half);
  }

  // The front of a chunk: plan (unless sorted ahead), the first one starts the table builds, a
  // waiting host hook runs, then each curve's ECDSA front on its side stream beside the challenge
  // hashes on MAIN. The side streams wait for everything on MAIN so far: this chunk's plan, and the
  // ladders of the chunk two back, which read the item workspace this front writes.
  Error items_front(const Chunk& c, bool planned) {
    Error e = Ops::kOk;
    if (!planned) e = items_plan(c);
    if (e == Ops::kOk) e = key_tables();
    if (e == Ops::kOk && ops_.mid_hook()) e = ops_.run(ST_MID_HOOK, MAIN, c.chunk, c.half);
    if (e != Ops::kOk) return e;
    e = ops_.record(EV_EC_FRONT_GO, MAIN);
    for (int k = 0; k < 2 && e == Ops::kOk; ++k) {
      e = ops_.wait(side(k), EV_EC_FRONT_GO);
      if (e != Ops::kOk) break;
      ops_.run(stage(ST_EC_FRONT_R1, k), side(k), c.chunk, c.half);
      e = ops_.record(Event(EV_EC_FRONT_DONE0 + k), side(k));
    }
    if (e != Ops::kOk) return e;
    ops_.run(ST_ED_FRONT, MAIN, c.chunk, c.half);
    return Ops::kOk;
  }

  // The back of a chunk: row-0 / quarter ladders on the side streams after their tables there and
  // the hashes on MAIN; full- and wide-table ladders on MAIN, each family's after its tables (and a
  // curve's after its front); the Ed25519 finish on SIDE2 beside the ECDSA ladders; then MAIN joins
  // every side stream, so a chunk ends with nothing in flight beside MAIN.
  Error items_back(const Chunk& c) {
    Error e = ops_.record(EV_FRONT, MAIN);
    for (int k = 0; k < 3 && e == Ops::kOk; ++k) e = ops_.wait(side(k), EV_FRONT);
    if (e != Ops::kOk) return e;
    static const int order[3] = {2, 0, 1};
    for (int k : order)
      if (p_.need_full[k]) ops_.run(stage(ST_ROW0_LADDER_R1, k), side(k), c.chunk, c.half);
    for (int k = 0; k < 3 && e == Ops::kOk; ++k) e = ops_.record(row0(k), side(k));
    if (e != Ops::kOk) return e;
    (void)ops_.wait(MAIN, ready(2));
    ops_.run(ST_FULL_LADDER_ED, MAIN, c.chunk, c.half);
    if (c.wide_ed) ops_.run(ST_WIDE_LADDER_ED, MAIN, c.chunk, c.half);
    e = ops_.record(EV_FRONT, MAIN);
    if (e == Ops::kOk) e = ops_.wait(SIDE2, EV_FRONT);
    if (e != Ops::kOk) return e;
    ops_.run(ST_ED_FINISH, SIDE2, c.chunk, c.half);
    e = ops_.record(row0(2), SIDE2);
    if (e != Ops::kOk) return e;
    for (int k = 0; k < 2; ++k) {
      (void)ops_.wait(MAIN, ready(k));
      (void)ops_.wait(MAIN, Event(EV_EC_FRONT_DONE0 + k));
      ops_.run(stage(ST_FULL_LADDER_R1, k), MAIN, c.chunk, c.half);
      if (c.wide_ec) ops_.run(stage(ST_WIDE_LADDER_R1, k), MAIN, c.chunk, c.half);
    }
    ops_.before_joins();
    for (int k = 0; k < 3; ++k) (void)ops_.wait(MAIN, row0(k));
    if (p_.skip_mask) ops_.run(ST_MODE_GUARD, MAIN, c.chunk, c.half);
    return Ops::kOk;
  }

 private:
  void run(Stage s, Stream on) { (void)ops_.run(s, on, -1, -1); }
  Ops& ops_;
  Pending& p_;
};

// ---- a call's sequencing over an engine build.
// Eng: type Error, constant kOk, and
//   Error keyprep(); Error rsa_keyprep(); Error key_tables();
//   Error prepare(unsigned k);                      the tx-signature forms' hook ahead of chunk k's front
//   Error plan(unsigned k, int half); Error front(unsigned k, int half, bool planned);
//   Error back(unsigned k, int half); void chunk_enqueued(unsigned k);
//   Error rsa_pass(Error);                          the RSA item pass, behind the last back
//   Error wait(Stream, Event);

struct CallPlan {
  unsigned chunks = 1;
  bool two = false;             // two item workspaces: chunk k uses half k & 1
  bool hook = false;            // a prepare hook makes chunk k's items just before its front
  bool hook_blocks = false;     // and copies from host memory, blocking the enqueuing thread
};

// Key tables once for the whole call, then the items in chunks, in one of three orders: a blocking
// hook: front k, back k; two workspaces: front k + 1 before back k (the first chunk's wait for the
// key tables is spent on the next chunk's front); one workspace: serial. Without a hook both first
// plans sort before the table builds start (their look-back stalls behind the builds); a blocking
// hook starts the builds first, so that they overlap the first chunk's copies.
template <class Eng>
typename Eng::Error chunked(Eng& g, const CallPlan& c) {
  using Error = typename Eng::Error;
  const Error ok = Eng::kOk;
  Error e = g.keyprep();
  if (e == ok) e = g.rsa_keyprep();
  const bool two = c.two && c.chunks > 1;
  const bool pre_plan = two && !c.hook;
  auto half = [&](unsigned k) { return two ? int(k & 1) : 0; };
  auto front = [&](unsigned k) {
    if (c.hook) {
      const Error w = g.prepare(k);
      if (w != ok) return w;
    }
    return g.front(k, half(k), pre_plan && k < 2);
  };
  if (e == ok && pre_plan) e = g.plan(0, half(0));
  if (e == ok && pre_plan) e = g.plan(1, half(1));
  if (e == ok && c.hook && c.hook_blocks) e = g.key_tables();
  if (c.hook_blocks) {
    for (unsigned k = 0; k < c.chunks && e == ok; ++k) {
      e = front(k);
      if (e == ok) e = g.back(k, half(k));
      g.chunk_enqueued(k);
    }
    return g.rsa_pass(e);
  }
  if (e == ok) e = front(0);
  for (unsigned k = 0; k < c.chunks && e == ok; ++k) {
    if (!two && k > 0) e = front(k);
    if (two && k + 1 < c.chunks && e == ok) e = front(k + 1);
    if (e == ok) e = g.back(k, half(k));
  }
  return g.rsa_pass(e);
}

// cg_prepare_keys_device: every key gets full tables, built at once on the side streams. MAIN then
// waits for each family's builds, so that the call's end (the call scope's `done`, recorded on MAIN)
// is the end of its device work: the caller may rewrite its key bytes, and the context's next call
// its key workspace. `join` = false is the schedule before that fix, kept for the audit to show
// what it let through.
template <class Eng>
typename Eng::Error prepare_keys(Eng& g, bool any_keys, bool join = true) {
  typename Eng::Error e = g.keyprep();
  if (e == Eng::kOk) e = g.rsa_keyprep();
  for (int k = 0; k < 3 && e == Eng::kOk && any_keys && join; ++k) e = g.wait(MAIN, ready(k));
  return e;
}

// cg_verify_items_device: the items of prepared keys, chunk after chunk over one workspace.
template <class Eng>
typename Eng::Error verify_items(Eng& g, unsigned chunks) {
  typename Eng::Error e = Eng::kOk;
  for (unsigned k = 0; k < chunks && e == Eng::kOk; ++k) {
    e = g.front(k, 0, false);
    if (e == Eng::kOk) e = g.back(k, 0);
  }
  return g.rsa_pass(e);
}

}  // namespace cgs
