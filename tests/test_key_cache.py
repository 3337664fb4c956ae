"""The wide-table cache's bookkeeping (corda_amd/csrc/key_cache.h) on the CPU, through the stand-alone
program tests/native/key_cache_test.cpp: random call sequences (overlapping, shrinking and oversized
key sets, duplicate key rows, failed calls, indexes narrowed to one or two home entries) through the
functions the device kernels call, against a dictionary. The program checks that a hit's owner bytes
equal the key's, that a claim never takes a slot hit in the same call, that two keys share a slot
only with equal scheme and bytes, that hot keys within the capacity all get slots, that pending
owners never hit, and that the cache is empty after "dirty". The same program is also built with
the host sanitizers and run on its own."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "key_cache_test.cpp")
HDR = os.path.join(HERE, "..", "corda_amd", "csrc", "key_cache.h")


def _build(exe, extra):
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, SRC])
    return exe


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok: "), p.stdout


def test_key_cache_against_a_dictionary():
    _run(_build(os.path.join(HERE, "native", "key_cache_test"), []))


def test_key_cache_under_the_host_sanitizers():
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main() { return 0; }", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    _run(_build(os.path.join(HERE, "native", "key_cache_test_san"),
                ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))
