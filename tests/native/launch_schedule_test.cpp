// CPU driver of corda_amd/csrc/launch_schedule.h (inside corda_amd/csrc/call_scope.h's call scope)
// for tests/test_launch_schedule.py: the schedule over a backend that logs every record, wait and
// stage instead of making it, so the test can audit the order for stream races. No HIP.
//
// A log is tokens separated by blanks: rec(event,stream)  wait(stream,event)  stage@stream for a
// whole-call stage, stage@stream[chunk/half] for an item stage. Streams: M the context's own,
// S0 S1 S2 its side streams (families r1, k1, ed), C a caller's stream the calls are bridged from.
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <sstream>
#include <string>

#include "../../corda_amd/csrc/call_scope.h"
#include "../../corda_amd/csrc/launch_schedule.h"

namespace {

const char* const kStream[] = {"M", "S0", "S1", "S2"};
const char* const kEvent[cgs::kEvents] = {"start", "planned", "ready0", "ready1", "ready2", "front", "row0_0", "row0_1",
                                          "row0_2", "ec_go", "ec_done0", "ec_done1"};
const char* const kStage[cgs::kStages] = {
    "key_init", "key_uses", "key_counts", "key_uses_txsig", "kc_begin", "key_classify", "kc_claim",
    "chains_r1", "chains_k1", "chains_ed", "wide_tabs_r1", "wide_tabs_k1", "wide_tabs_ed",
    "full_tabs_r1", "full_tabs_k1", "full_tabs_ed", "ed_abyte", "misc_status", "plan",
    "ec_front_r1", "ec_front_k1", "ed_front", "row0_ladder_r1", "row0_ladder_k1", "row0_ladder_ed",
    "full_ladder_r1", "full_ladder_k1", "full_ladder_ed", "wide_ladder_r1", "wide_ladder_k1", "wide_ladder_ed",
    "ed_finish", "mode_guard", "rsa_keyprep", "rsa_items", "prepare_hook", "mid_hook"};

struct Log {
  std::string text;
  std::set<std::string> drop;  // "stream:event": these waits are not made
  void add(const std::string& t) { text += t + " "; }
  void wait(const std::string& s, const std::string& e) {
    if (!drop.count(s + ":" + e)) add("wait(" + s + "," + e + ")");
  }
};

struct FakeOps {
  using Error = int;
  static constexpr Error kOk = 0;
  Log& log;
  bool mid = false;  // a blocking prepare hook left its second half for the front
  Error record(cgs::Event e, cgs::Stream s) {
    log.add(std::string("rec(") + kEvent[e] + "," + kStream[s] + ")");
    return kOk;
  }
  Error wait(cgs::Stream s, cgs::Event e) {
    log.wait(kStream[s], kEvent[e]);
    return kOk;
  }
  Error run(cgs::Stage st, cgs::Stream s, int chunk, int half) {
    std::string t = std::string(kStage[st]) + "@" + kStream[s];
    if (chunk >= 0) t += "[" + std::to_string(chunk) + "/" + std::to_string(half) + "]";
    log.add(t);
    if (st == cgs::ST_MID_HOOK) mid = false;
    return kOk;
  }
  bool mid_hook() const { return mid; }
  void before_joins() {}
};

// A call over the fake: what cordagpu.cpp's adapter does with the context's engine build.
struct FakeEng {
  using Error = int;
  static constexpr Error kOk = 0;
  FakeOps& ops;
  cgs::Pending& pending;
  cgs::KeyPlan keys;
  bool rsa = false;
  int hook = 0;  // 1: a prepare hook; 2: one that blocks and leaves a mid hook
  bool wide_ed = false, wide_ec = false;
  cgs::Schedule<FakeOps> sched{ops, pending};
  cgs::Chunk chunk(unsigned k, int half) const {
    cgs::Chunk c;
    c.chunk = (int)k;
    c.half = half;
    c.wide_ed = wide_ed;
    c.wide_ec = wide_ec;
    return c;
  }
  Error keyprep() { return sched.keyprep(keys); }
  Error rsa_keyprep() { return rsa && keys.any_keys ? ops.run(cgs::ST_RSA_KEYPREP, cgs::MAIN, -1, -1) : kOk; }
  Error key_tables() { return sched.key_tables(); }
  Error prepare(unsigned k) {
    ops.run(cgs::ST_PREPARE_HOOK, cgs::MAIN, (int)k, -1);
    if (hook == 2) ops.mid = true;
    return kOk;
  }
  Error plan(unsigned k, int half) { return sched.items_plan(chunk(k, half)); }
  Error front(unsigned k, int half, bool planned) { return sched.items_front(chunk(k, half), planned); }
  Error back(unsigned k, int half) { return sched.items_back(chunk(k, half)); }
  void chunk_enqueued(unsigned) {}
  Error rsa_pass(Error e) { return e == kOk && rsa ? ops.run(cgs::ST_RSA_ITEMS, cgs::MAIN, -1, -1) : e; }
  Error wait(cgs::Stream s, cgs::Event e) { return ops.wait(s, e); }
};

// call_scope.h's Api over the same log: stream 1 is M, 5 the caller's; events 'd' done, 'b' bridge.
struct ScopeApi {
  using Stream = int;
  using Event = char;
  using Error = int;
  static constexpr Error kOk = 0;
  Log& log;
  static std::string sn(Stream s) { return s == 1 ? "M" : s == 5 ? "C" : "copy"; }
  static std::string en(Event e) { return e == 'd' ? "done" : "bridge"; }
  Error record(Event e, Stream s) {
    log.add("rec(" + en(e) + "," + sn(s) + ")");
    return kOk;
  }
  Error wait(Stream s, Event e) {
    log.wait(sn(s), en(e));
    return kOk;
  }
  Error sync(Stream s) {
    log.add("sync(" + sn(s) + ")");
    return kOk;
  }
};

using Args = std::map<std::string, std::string>;
int num(const Args& a, const char* k, int dflt) {
  const auto it = a.find(k);
  return it == a.end() ? dflt : atoi(it->second.c_str());
}

}  // namespace

// Runs `spec` and writes the log to out. spec: segments separated by ';', each a word and key=value
// settings:
//   drop S:E             the fake makes no wait of stream S for event E (from here on)
//   fill | reuse         the caller writes its buffers on C ahead of a call / rewrites its keys and
//                        arena and reads the status bytes on C behind it
//   verify chunks= two= hook= skip= wed= wec= cache= uses=none|items|counts|txsig rsa= keys= bridged=
//   prepare keys= rsa= join= bridged=
//   items chunks= rsa= bridged=
// One context (call state, pending tables) serves every call of the spec. Returns 0, -1 for a bad
// spec, or the size needed when out is short.
extern "C" int ls_run(const char* spec, char* out, unsigned cap) {
  Log log;
  FakeOps ops{log};
  cgs::Pending pending;
  ScopeApi api{log};
  cg::CallState<ScopeApi> st;
  st.stream = 1;
  st.copy = 2;
  st.done = 'd';
  st.bridge = 'b';
  std::stringstream segs(spec);
  std::string seg;
  while (std::getline(segs, seg, ';')) {
    std::stringstream ws(seg);
    std::string word, kv;
    if (!(ws >> word)) continue;
    Args a;
    while (ws >> kv) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) a[kv] = "";
      else a[kv.substr(0, eq)] = kv.substr(eq + 1);
    }
    if (word == "drop") {
      for (const auto& d : a) log.drop.insert(d.first);
      continue;
    }
    if (word == "fill" || word == "reuse") {
      log.add("caller_" + word + "@C");
      continue;
    }
    FakeEng g{ops, pending};
    g.rsa = num(a, "rsa", 0);
    cg::CallScope<ScopeApi> scope(api, st, cg::CallScope<ScopeApi>::kDevice);
    if (scope.open(num(a, "bridged", 1) ? 5 : 0) != 0) return -1;
    int e = 0;
    if (word == "verify") {
      const std::string uses = a.count("uses") ? a["uses"] : "items";
      g.keys.any_keys = num(a, "keys", 1);
      g.keys.uses = uses == "items" ? cgs::ST_KEY_USES : uses == "counts" ? cgs::ST_KEY_COUNTS
                  : uses == "txsig" ? cgs::ST_KEY_USES_TXSIG : cgs::ST_NONE;
      g.keys.cache = num(a, "cache", 0);
      g.keys.wide_ed = g.wide_ed = num(a, "wed", 0);
      g.keys.wide_ec = g.wide_ec = num(a, "wec", 0);
      for (int f = 0; f < 3; ++f) g.keys.need_full[f] = !((num(a, "skip", 0) >> f) & 1);
      g.hook = num(a, "hook", 0);
      cgs::CallPlan p;
      p.chunks = (unsigned)num(a, "chunks", 1);
      p.two = num(a, "two", 0);
      p.hook = g.hook != 0;
      p.hook_blocks = g.hook == 2;
      e = cgs::chunked(g, p);
    } else if (word == "prepare") {
      g.keys.any_keys = num(a, "keys", 1);
      g.keys.counted = false;
      e = cgs::prepare_keys(g, g.keys.any_keys, num(a, "join", 1));
    } else if (word == "items") {
      e = cgs::verify_items(g, (unsigned)num(a, "chunks", 1));
    } else {
      return -1;
    }
    if (e != 0 || scope.close() != 0) return -1;
  }
  if (log.text.size() + 1 > cap) return (int)log.text.size() + 1;
  memcpy(out, log.text.c_str(), log.text.size() + 1);
  return 0;
}

// The stage names, blank-separated, in enum order.
extern "C" int ls_stages(char* out, unsigned cap) {
  std::string s;
  for (int i = 0; i < cgs::kStages; ++i) s += std::string(kStage[i]) + " ";
  if (s.size() + 1 > cap) return -1;
  memcpy(out, s.c_str(), s.size() + 1);
  return 0;
}
