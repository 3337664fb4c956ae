// The stream ordering of one C-ABI call on a context, with no HIP in it, so that
// tests/native/call_scope_test.cpp runs exactly this code on the CPU over a fake that logs the calls.
//
// A context's calls share its workspace, whatever stream each runs on: `done` marks the end of the
// last call's device work, and the next call waits for it first. A device call on a
// caller's stream is bridged onto the context's own stream (stream bridge): that stream
// waits for what the caller enqueued before the call, and at the call's end the caller's stream
// waits for `done`, so the call stays ordered on the caller's stream.
//
// close() is the success path. A scope that was opened and is destroyed without it (any early
// return) does the same ordering best-effort and reports nothing, so the first error stays the one
// the caller sees: `done` is recorded behind whatever the call enqueued, a bridged caller's stream
// waits for it (the caller cannot reuse its buffers under kernels still in flight), `caller` is
// cleared; a host form also drains the context's main and copy streams, so no copy that reads the
// caller's memory or a local buffer, or writes the caller's results, outlives the call. A scope that
// never opened does nothing.
//
// Api: types Stream, Event, Error, the constant kOk, and
//   Error record(Event, Stream); Error wait(Stream, Event); Error sync(Stream);
#pragma once

namespace cg {

// What a context keeps between calls.
template <class Api>
struct CallState {
  typename Api::Stream stream{};  // the context's own stream, on a hardware queue of its own
  typename Api::Stream copy{};    // the host forms' copy stream
  typename Api::Event done{};     // the end of the last call's device work, whatever stream it ran on
  typename Api::Event bridge{};   // a caller stream's point of entry
  bool done_rec = false;
  bool bridged = true;            // off (CG_STREAM_BRIDGE=0): device calls run on the caller's stream itself
  typename Api::Stream caller{};  // the stream the current device call is bridged from
};

template <class Api>
class CallScope {
 public:
  using Stream = typename Api::Stream;
  using Error = typename Api::Error;
  enum Form { kDevice, kHost };

  CallScope(Api& api, CallState<Api>& st, Form form) : api_(api), st_(st), form_(form) {}
  CallScope(const CallScope&) = delete;
  ~CallScope() {
    if (!open_) return;
    finish();
    if (form_ != kHost) return;
    (void)api_.sync(st_.stream);
    (void)api_.sync(st_.copy);
  }
  // The stream the call runs on (stream()), ordered after the caller's earlier work and the context's
  // last call. A null caller stream or the context's own: that stream. Another: bridged, unless the
  // bridge is off or its record or wait fails, and then the caller's stream itself.
  Error open(Stream caller = Stream{}) {
    open_ = true;
    st_.caller = Stream{};
    run_ = st_.stream;
    if (caller != Stream{} && caller != st_.stream) {
      if (st_.bridged && st_.bridge != typename Api::Event{} && api_.record(st_.bridge, caller) == Api::kOk &&
          api_.wait(st_.stream, st_.bridge) == Api::kOk)
        st_.caller = caller;
      else
        run_ = caller;
    }
    return st_.done_rec ? api_.wait(run_, st_.done) : Api::kOk;
  }
  Stream stream() const { return run_; }
  // After the call's last enqueue: `done` recorded, a bridged caller's stream behind it.
  Error close() {
    open_ = false;
    return finish();
  }

 private:
  Error finish() {
    Error e = api_.record(st_.done, run_);
    if (e == Api::kOk) st_.done_rec = true;
    if (e == Api::kOk && st_.caller != Stream{}) e = api_.wait(st_.caller, st_.done);
    st_.caller = Stream{};
    return e;
  }
  Api& api_;
  CallState<Api>& st_;
  const Form form_;
  bool open_ = false;
  Stream run_{};
};

}  // namespace cg
