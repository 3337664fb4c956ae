// CPU driver of corda_amd/csrc/call_scope.h for tests/test_call_scope.py: the scope over a stream
// API that logs every call instead of making it, so the test can compare the exact sequence of
// records, waits and synchronisations on each exit path. No HIP.
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../corda_amd/csrc/call_scope.h"

namespace {

// streams: 1 the context's own, 2 its copy stream, 7 / 8 callers'. events: 'd' done, 'b' bridge.
struct FakeApi {
  using Stream = int;
  using Event = char;
  using Error = int;
  static constexpr Error kOk = 0;
  std::string log;
  int calls = 0, fail_at = 0;  // the fail_at-th call (1-based) of this scope's run returns an error
  Error step(const std::string& what) {
    log += what + ") ";
    return ++calls == fail_at ? 9 : kOk;
  }
  Error record(Event e, Stream s) { return step(std::string("rec(") + e + "," + std::to_string(s)); }
  Error wait(Stream s, Event e) { return step("wait(" + std::to_string(s) + "," + e); }
  Error sync(Stream s) { return step("sync(" + std::to_string(s)); }
};
using State = cg::CallState<FakeApi>;
using Scope = cg::CallScope<FakeApi>;

State fresh() {
  State st;
  st.stream = 1;
  st.copy = 2;
  st.done = 'd';
  st.bridge = 'b';
  return st;
}

// One call: open on `caller`, then close (exit 'c'), leave early (exit 'e'), or never open (exit 'n').
// Appends "| run=<stream> open=<rc> close=<rc>" and the state the call left.
void call(FakeApi& api, State& st, Scope::Form form, int caller, char exit_by, int fail_at = 0) {
  api.calls = 0;
  api.fail_at = fail_at;
  int run = 0, orc = -1, crc = -1;
  {
    Scope sc(api, st, form);
    if (exit_by != 'n') {
      orc = sc.open(caller);
      run = sc.stream();
      if (exit_by == 'c') crc = sc.close();
    }
  }
  char buf[96];
  snprintf(buf, sizeof buf, "| run=%d open=%d close=%d caller=%d done_rec=%d; ", run, orc, crc, st.caller, (int)st.done_rec);
  api.log += buf;
}

}  // namespace

// Runs the named case and writes its log to out. Returns 0, or -1 for an unknown case / short buffer.
extern "C" int cs_case(const char* name, char* out, unsigned cap) {
  FakeApi api;
  State st = fresh();
  const std::string n = name;
  const Scope::Form D = Scope::kDevice, H = Scope::kHost;
  if (n == "null_caller") call(api, st, D, 0, 'c');
  else if (n == "own_stream") call(api, st, D, 1, 'c');
  else if (n == "bridged") call(api, st, D, 7, 'c');
  else if (n == "bridge_off") { st.bridged = false; call(api, st, D, 7, 'c'); }
  else if (n == "no_bridge_event") { st.bridge = 0; call(api, st, D, 7, 'c'); }
  else if (n == "bridge_record_fails") call(api, st, D, 7, 'c', 1);
  else if (n == "bridge_wait_fails") call(api, st, D, 7, 'c', 2);
  else if (n == "second_call_waits") { call(api, st, D, 7, 'c'); call(api, st, D, 8, 'c'); }
  else if (n == "second_call_host") { call(api, st, D, 7, 'c'); call(api, st, H, 0, 'c'); }
  else if (n == "early_exit_device") call(api, st, D, 7, 'e');
  else if (n == "early_exit_device_unbridged") call(api, st, D, 0, 'e');
  else if (n == "early_exit_host") call(api, st, H, 0, 'e');
  else if (n == "close_record_fails") call(api, st, D, 7, 'c', 3);
  else if (n == "close_wait_back_fails") call(api, st, D, 7, 'c', 4);
  else if (n == "open_wait_fails") { call(api, st, D, 7, 'c'); call(api, st, D, 7, 'e', 3); }
  else if (n == "exit_before_open") { call(api, st, D, 7, 'n'); call(api, st, H, 0, 'n'); }
  else if (n == "after_a_failed_call") { call(api, st, D, 7, 'e'); call(api, st, D, 8, 'c'); call(api, st, H, 0, 'c'); }
  else return -1;
  if (api.log.size() + 1 > cap) return -1;
  memcpy(out, api.log.c_str(), api.log.size() + 1);
  return 0;
}
