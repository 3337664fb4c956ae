"""Generates tests/golden/encoding_sweep.json: the expected statuses of the encoding sweeps of
tests/encoding_sweep.py (mutated, truncated, extended and over-long ECDSA and Ed25519 signatures and
keys, and the status precedence matrix), from the Python oracle.

The sweeps themselves are rebuilt by tests/encoding_sweep.py from the base vectors; the file
records

  base      the base vectors (scalars, nonces, seed, raw keys, base signatures), so a test can tell a
            change of the builders from a change of a verdict;
  expect    per sweep (a..e) and mode (doverify / isvalid) one digit per item, in sweep order: the
            status code, 9 for NOT_RUN (encoding_sweep.DIGIT);
  meta      per sweep the item count and the count per status name and mode.

Every status is oracle.corda.verify_item's, except an item whose key index lies behind the key
table: Crypto.kt has no such input, include/cordagpu.h gives it NOT_RUN.

usage: python tests/golden/gen_encoding_sweep.py   (about a minute on 8 cores)
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import encoding_sweep as ES  # noqa: E402
from oracle import corda  # noqa: E402

MODES = (("doverify", corda.MODE_DOVERIFY), ("isvalid", corda.MODE_ISVALID))
PATH = os.path.join(HERE, "encoding_sweep.json")


def oracle_status(job):
    it, mode = job
    if it.past:
        return corda.NOT_RUN
    return corda.verify_item(it.scheme, it.fmt, it.key, it.sig, it.msg, mode)


def counts(digits):
    out = {}
    for c in digits:
        name = corda.STATUS_NAMES[ES.STATUS_OF_DIGIT[c]]
        out[name] = out.get(name, 0) + 1
    return out


def main():
    expect, meta = {}, {}
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        for name in sorted(ES.SWEEPS):
            items = ES.sweep(name)
            expect[name] = {}
            meta[name] = {"items": len(items)}
            for mode_name, mode in MODES:
                digits = ES.digits_of(ex.map(oracle_status, [(it, mode) for it in items], chunksize=32))
                expect[name][mode_name] = digits
                meta[name][mode_name] = counts(digits)
            print(name, meta[name], flush=True)
    meta["generator"] = "tests/golden/gen_encoding_sweep.py"
    meta["note"] = "expect = oracle.corda.verify_item over tests/encoding_sweep.py's sweeps; 9 = NOT_RUN (key index past the table)"
    with open(PATH, "w") as f:
        f.write('{"meta": %s,\n"base": %s,\n"expect": {\n' % (json.dumps(meta), json.dumps(ES.base_record())))
        f.write(",\n".join('"%s": %s' % (n, json.dumps(expect[n])) for n in sorted(expect)))
        f.write("\n}}\n")
    print(os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
