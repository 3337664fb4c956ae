"""The call scope every C-ABI entry point goes through (corda_amd/csrc/call_scope.h), on the CPU:
tests/native/call_scope_test.cpp drives it over a stream API that logs each call, and the exact
sequence of event records, stream waits and synchronisations is compared with a table.

Streams: 1 the context's own, 2 its copy stream, 7 and 8 callers'. Events: d = done, b = bridge.
`rec(e,s)` records e on s, `wait(s,e)` makes s wait for e, `sync(s)` drains s. After `|`: the stream
the call ran on, what open() and close() returned (-1: not called, 9: the injected failure), and
what the call left in the context.

SUCCESS is what the free functions the scope replaced did (stream_of, then order_in; order_out at
the end), written down from them before they went:
  stream_of   caller = null; a null stream or the context's own -> the context's stream, no call;
              bridge off, no bridge event, rec(b,caller) fails or wait(1,b) fails -> the caller's
              stream, in that order; else caller = the stream, run on 1.
  order_in    done_rec ? wait(run,d) : nothing.
  order_out   rec(d,run); ok -> done_rec = true; ok and caller -> wait(caller,d); caller = null; the
              first error is returned.
EXITS is the contract for the paths that had no code: an early return after open() orders the
caller's stream behind whatever was enqueued, a host form also drains both streams, and a scope
that never opened makes no call."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "libcallscopetest.so")

OK = "| run=%d open=0 close=0 caller=0 done_rec=1; "
BRIDGED_7 = "rec(b,7) wait(1,b) rec(d,1) wait(7,d) " + OK % 1

SUCCESS = {
    "null_caller": "rec(d,1) " + OK % 1,                      # the first call waits for nothing
    "own_stream": "rec(d,1) " + OK % 1,
    "bridged": BRIDGED_7,
    "bridge_off": "rec(d,7) " + OK % 7,
    "no_bridge_event": "rec(d,7) " + OK % 7,
    "bridge_record_fails": "rec(b,7) rec(d,7) " + OK % 7,
    "bridge_wait_fails": "rec(b,7) wait(1,b) rec(d,7) " + OK % 7,
    "second_call_waits": BRIDGED_7 + "rec(b,8) wait(1,b) wait(1,d) rec(d,1) wait(8,d) " + OK % 1,
    "second_call_host": BRIDGED_7 + "wait(1,d) rec(d,1) " + OK % 1,
    "close_record_fails": "rec(b,7) wait(1,b) rec(d,1) | run=1 open=0 close=9 caller=0 done_rec=0; ",
    "close_wait_back_fails": "rec(b,7) wait(1,b) rec(d,1) wait(7,d) | run=1 open=0 close=9 caller=0 done_rec=1; ",
}

LEFT = "| run=1 open=%d close=-1 caller=0 done_rec=1; "
NEVER = "| run=0 open=-1 close=-1 caller=0 done_rec=0; "
EXITS = {
    "early_exit_device": "rec(b,7) wait(1,b) rec(d,1) wait(7,d) " + LEFT % 0,
    "early_exit_device_unbridged": "rec(d,1) " + LEFT % 0,
    "early_exit_host": "rec(d,1) sync(1) sync(2) " + LEFT % 0,
    "open_wait_fails": BRIDGED_7 + "rec(b,7) wait(1,b) wait(1,d) rec(d,1) wait(7,d) " + LEFT % 9,
    "exit_before_open": NEVER + NEVER,
    # the call after a failed one waits for the failed one's leftovers, and so does the one after it
    "after_a_failed_call": ("rec(b,7) wait(1,b) rec(d,1) wait(7,d) " + LEFT % 0 +
                            "rec(b,8) wait(1,b) wait(1,d) rec(d,1) wait(8,d) " + OK % 1 +
                            "wait(1,d) rec(d,1) " + OK % 1),
}


def _lib():
    src = os.path.join(HERE, "native", "call_scope_test.cpp")
    hdr = os.path.join(HERE, "..", "corda_amd", "csrc", "call_scope.h")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO, src])
    L = ctypes.CDLL(SO)
    L.cs_case.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint]
    return L


def _run(name):
    buf = ctypes.create_string_buffer(1024)
    assert _lib().cs_case(name.encode(), buf, len(buf)) == 0, name
    return buf.value.decode()


@pytest.mark.parametrize("name", sorted(SUCCESS))
def test_open_and_close_make_the_calls_the_free_functions_made(name):
    assert _run(name) == SUCCESS[name]


@pytest.mark.parametrize("name", sorted(EXITS))
def test_every_other_exit_closes_the_scope(name):
    assert _run(name) == EXITS[name]


def test_the_header_has_no_hip_in_it():
    src = open(os.path.join(HERE, "..", "corda_amd", "csrc", "call_scope.h")).read()
    assert "#include" not in src and "hipStream" not in src and "hipEvent" not in src
