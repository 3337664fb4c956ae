"""Tear-off building on the CPU: the host build of corda_amd/csrc/pmt_build.h (the walk and the by-value
inclusion rule that build_filtered.hip's lanes run, tests/native/pmt_build_test.cpp) against
oracle.corda: partial_tree_postorder(partial_tree_build(merkle_tree(h), incl)) and merkle_root. Every mask
at every leaf count 1..9 (P = 1, 2, 4, 8, 16; padding blocks of 1, 2, 4 and 1 + 2 + 4 leaves), seeded
random masks at 16, 17, 33 and 100 leaves, the deep trees of build_filtered_ref.deep_masks (31 .. 4097 leaves,
levels 5 .. 13: the stack above level 7, the largest hidden blocks, the zeroHash padding of P / 2 - 1 leaves as
hidden blocks of every size), and the rules of the bare form; the same cases once more through the program
built with -fsanitize=address,undefined."""
import os
import struct
import subprocess

import numpy as np
import pytest

from build_filtered_ref import DEEP_COUNTS, DEEP_MASKS, bare_cases, deep_masks, leaf_hashes
from oracle import corda as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "pmt_build_test.cpp")
DEPS = [SRC] + [os.path.join(HERE, "..", "corda_amd", "csrc", h) for h in ("pmt_build.h", "sha2.h", "fe25519.h")] + \
    [os.path.join(HERE, "..", "include", "cordagpu.h")]
BY_INDEX = 0xFFFFFFFF


def build_program(out, flags):
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-o", out + ".tmp", SRC])
        os.replace(out + ".tmp", out)
    return out


def deep_cases():
    """(leaves, mask) for every mask of deep_masks at every leaf count of DEEP_COUNTS, count-major."""
    out = []
    for n in DEEP_COUNTS:
        hs = leaf_hashes(n, n)
        out += [(hs, mask) for mask in deep_masks(n).values()]
    return out


def mask_cases():
    """(leaves, mask) for every mask at n = 1..9, seeded random masks at n = 16, 17, 33, 100, and the deep trees."""
    out = []
    for n in range(1, 10):
        hs = leaf_hashes(n, n)
        for bits in range(1 << n):
            out.append((hs, [(bits >> i) & 1 for i in range(n)]))
    rng = np.random.default_rng(20)
    for n in (16, 17, 33, 100):
        hs = leaf_hashes(n, n)
        for density in (0.03, 0.1, 0.3, 0.5, 0.9):
            for _ in range(6):
                out.append((hs, [int(x) for x in rng.random(n) < density]))
        out.append((hs, [0] * (n - 1) + [1]))
        out.append((hs, [1] + [0] * (n - 1)))
    return out + deep_cases()


def to_file(cases, path):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for leaves, sel, by_index in cases:
            f.write(struct.pack("<II", len(leaves), BY_INDEX if by_index else len(sel)))
            f.write(b"".join(leaves))
            f.write(bytes(sel) if by_index else b"".join(sel))


def expected(leaves, sel, by_index):
    """The output line's content from the oracle: status, stream, root."""
    if not leaves:
        return 1, None, None
    include = [h for h, v in zip(leaves, sel) if v] if by_index else sel
    try:
        pt = O.partial_tree_build(O.merkle_tree(leaves), include)
    except O.MerkleTreeException:
        return 5, None, None
    except ValueError:
        return 4, None, None
    return 0, O.partial_tree_postorder(pt), O.merkle_root(leaves)


def parse(line):
    parts = line.split()
    if parts[0] != "0":
        return int(parts[0]), None, None, None
    stream = []
    for tok in parts[1:-2]:
        kind, _, hx = tok.partition(":")
        stream.append((int(kind), bytes.fromhex(hx) if hx else None))
    assert parts[-2].startswith("root:") and parts[-1].startswith("counts:"), line[-200:]
    return 0, stream, bytes.fromhex(parts[-2][5:]), [int(x) for x in parts[-1][7:].split(",")]


def check(cases, exe, tmp_path):
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.txt")
    to_file(cases, fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout + r.stderr[-3000:]
    lines = open(fout).read().splitlines()
    assert len(lines) == len(cases)
    statuses = set()
    for k, (case, line) in enumerate(zip(cases, lines)):
        assert "MISMATCH" not in line, (k, line[-200:])
        st, stream, root, counts = parse(line)
        want_st, want_stream, want_root = expected(*case)
        assert st == want_st, (k, case[1])
        statuses.add(st)
        if st == 0:
            assert stream == want_stream, (k, len(case[0]), case[1])
            assert root == want_root, k
            p = 1
            while p < len(case[0]):
                p <<= 1
            assert counts == [len(stream), sum(1 for kind, _ in stream if kind), p - 1], k
    return statuses


@pytest.fixture(scope="module")
def program():
    return build_program(os.path.join(HERE, "native", "pmt_build_test"), [])


def test_every_mask_up_to_nine_leaves_and_random_masks(program, tmp_path):
    cases = [(hs, m, True) for hs, m in mask_cases()]
    n_deep = len(DEEP_COUNTS) * len(DEEP_MASKS)
    assert len(cases) == sum(1 << n for n in range(1, 10)) + 4 * 32 + n_deep
    # what the deep cases are there for, as the oracle sees them: at P / 2 + 1 leaves with only the last one
    # included, the left half is one hidden block of level top - 1 and the padding is one hidden block of every
    # level below that; with everything included the padding alone is cut
    deep = {(len(hs), name): (hs, m) for (hs, m, _), name in zip(cases[-n_deep:], DEEP_MASKS * len(DEEP_COUNTS))}
    assert max(DEEP_COUNTS) > 1 << 12 and {33, 257, 1025, 4097} <= set(DEEP_COUNTS)
    for n in (33, 257, 1025, 4097):
        top = (n - 2).bit_length() + 1
        assert 1 << top == 2 * (n - 1) and deep[n, "last"][1] == [0] * (n - 1) + [1] and sum(deep[n, "first"][1]) == 1
        kinds = [k for k, _ in expected(*deep[n, "last"], True)[1]]
        assert kinds == [1, 2] + [1, 0] * (top - 1) + [0]
        assert sum(deep[n, "split"][1]) == 2 and deep[n, "split"][1][n - 2:] == [1, 1]
        kinds = [k for k, _ in expected(*deep[n, "all"], True)[1]]
        assert kinds.count(2) == n and kinds.count(1) == top - 1
    assert check(cases, program, tmp_path) == {0}


def test_bare_form_rules(program, tmp_path):
    cases = [(hs, inc, False) for hs, inc in bare_cases()]
    assert [expected(*c)[0] for c in cases[:13]] == [5, 5, 5, 5, 5, 4, 4, 0, 0, 0, 0, 1, 1]
    assert check(cases, program, tmp_path) == {0, 1, 4, 5}


def test_under_the_host_sanitizers(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main() { return 0; }", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    exe = build_program(os.path.join(HERE, "native", "pmt_build_test_san"),
                        ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    cases = [(hs, m, True) for hs, m in mask_cases()] + [(hs, inc, False) for hs, inc in bare_cases()]
    assert check(cases, exe, tmp_path) == {0, 1, 4, 5}
