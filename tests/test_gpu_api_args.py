"""Every argument refusal of the verify, transactions, tx-signature, verdict and tear-off building entry
points (the cg_pool_* twins included), in the order the library checks them: the return code is CG_ERR_ARG and
cg_last_error gives the exact text. The table was written down from the checks in
corda_amd/csrc/cordagpu.cpp, entry point by entry point in source order; a call with two faults at
once pins which check comes first (a device form has no check of the key table, so there the mode
wins). No refused call touches a result buffer or enqueues anything.

Not here: "RSA keys were not prepared" (cg_verify_items_device on a CG_FLAG_RSA context: the one call
that prepares the keys prepares the RSA records too) and "empty pool" (cg_pool_open refuses a pool
without slots)."""
import numpy as np
import pytest

from corda_amd import _lib
from corda_amd import batch as B

pytestmark = pytest.mark.gpu

NULL_SIG = "NULL signature / status buffer"
TMPL16 = "more than 65536 templates (cg_txsig.tmpl is 16-bit)"
OUTSIDE = "the signature stream lies outside the arena"
TXV_SIG = "NULL signature table / status"
STRIDE = "sig_stride is neither 12 (cg_txsig_packed) nor 24 (cg_txsig)"
N_TX = "more than 2^32 - 1 transactions"
RESERVED = "cg_tx_check.reserved must be 0"
INNER = "cg_pool_verify_tx_signatures_packed"  # cg_pool_verify_required_signatures_packed runs it after its own checks

BATCH = "keys n_keys items n_items arena arena_len mode status"
TXN = "txs n_tx comps n_comps keys n_keys sigs n_sigs tmpls n_tmpls arena arena_len mode ids tx_status sig_status"
TXSIG = "keys n_keys ids n_ids sigs n_sigs tmpls n_tmpls arena arena_len mode status"
TXSIG12 = "keys n_keys ids n_ids sigs n_sigs stream stream_len tmpls n_tmpls arena arena_len mode status"
TABLES = "key_class checks n_tx reqs n_reqs nodes n_nodes"
TXV = "sigs stride n_sigs status keys n_keys " + TABLES + " verdicts req_status"
REQ = TXSIG12.replace(" status", "") + " " + TABLES + " status verdicts req_status"

# the refusals every form of a family shares, in the order they are checked: (faulty arguments, text)
BATCH_DEV = [({"items": None}, "NULL buffer"), ({"status": None}, "NULL buffer"), ({"mode": 2}, "bad mode")]
BATCH_HOST = BATCH_DEV[:2] + [({"keys": None}, "keys is NULL"), ({"arena": None}, "arena is NULL"), BATCH_DEV[2]]
TXN_TX = [({"txs": None}, "NULL tx buffer"), ({"ids": None}, "NULL tx buffer"), ({"tx_status": None}, "NULL tx buffer"),
          ({"sigs": None}, "NULL sig buffer"), ({"sig_status": None}, "NULL sig buffer")]
TXN_DEV = TXN_TX + [({"tmpls": None}, "templates is NULL"), ({"mode": 2}, "bad mode")]
TXN_HOST = TXN_TX + [({"comps": None}, "comps is NULL"), ({"keys": None}, "keys is NULL"),
                     ({"tmpls": None}, "templates is NULL"), ({"arena": None}, "arena is NULL"), ({"mode": 2}, "bad mode")]
TXSIG_HEAD = [({"keys": None}, "keys is NULL"), ({"ids": None}, "ids is NULL"), ({"tmpls": None}, "templates is NULL"),
              ({"n_tmpls": 0x10001}, TMPL16), ({"mode": 2}, "bad mode")]
TXSIG_ALL = [({"sigs": None}, NULL_SIG), ({"status": None}, NULL_SIG)] + TXSIG_HEAD
STREAM_DEV = [({"stream": 65}, OUTSIDE), ({"stream": 60, "stream_len": 5}, OUTSIDE)]
STREAM_HOST = [({"arena": None}, "arena is NULL"), ({"stream": None}, "sig_bytes is NULL")]
TXV_TABLES = [({"checks": None}, "NULL checks / verdicts"), ({"verdicts": None}, "NULL checks / verdicts"),
              ({"n_tx": 1 << 32}, N_TX), ({"reqs": None}, "NULL reqs / req_status"),
              ({"req_status": None}, "NULL reqs / req_status"), ({"nodes": None}, "nodes is NULL")]
TXV_ALL = [({"stride": 16}, STRIDE), ({"sigs": None}, TXV_SIG), ({"status": None}, TXV_SIG),
           ({"keys": None}, "keys is NULL")] + TXV_TABLES
BAD_CHECKS = ({"checks": "reserved"}, RESERVED)
KEYS_AND_MODE = {"keys": None, "mode": 2}
# tear-off building: the totals, the fixed-size results, the tables behind a non-zero capacity, the alignment a
# device form asks for (ODD: the valid pointer plus one), then the inputs
BUILD_OUT = "out_base ftxs node_rows node_cap leaves leaf_cap out out_cap status totals"
BUILD_TX = "txs n_tx comps n_comps arena arena_len visible " + BUILD_OUT
BUILD_PT = "leaf_hashes first count n include inc_first inc_count " + BUILD_OUT
BUILD_PT_DEV = "leaf_hashes n_leaf_hashes first count n leaf_total include n_inc_hashes inc_first inc_count " + BUILD_OUT
ODD = "the valid pointer plus one"
BUILD_HEAD = [({k: None}, "NULL buffer") for k in ("totals", "ftxs", "status")] + \
    [({k: None}, "NULL table") for k in ("node_rows", "leaves", "out")]
BUILD_ALIGN = [({"out": ODD}, "out is not 16-byte aligned")]
BUILD_TX_IN = [({k: None}, "NULL buffer") for k in ("txs", "comps", "visible")]
BUILD_PT_IN = [({k: None}, "NULL buffer") for k in ("first", "count", "inc_first", "inc_count")]
BUILD_PT_DEV_IN = BUILD_PT_IN + [({k: None}, "NULL buffer") for k in ("leaf_hashes", "include")] + \
    [({k: ODD}, "a hash table is not 4-byte aligned") for k in ("leaf_hashes", "include")]
TABLE_FIRST = ({"out": None, "first": None, "txs": None}, "NULL table")

# entry point -> (its arguments after the handle, what follows them, the refusals in order, the two-fault call)
ENTRIES = {
    "cg_verify_batch_device": (BATCH, "hip", BATCH_DEV, (KEYS_AND_MODE, "bad mode")),
    "cg_prepare_keys_device": ("keys n_keys arena arena_len", "hip", [({"keys": None}, "keys is NULL")], None),
    "cg_verify_items_device": (BATCH, "hip", BATCH_DEV + [
        ({"n_keys": 0xFFFFFFFF}, "keys were not prepared (call cg_prepare_keys_device)")], (KEYS_AND_MODE, "bad mode")),
    "cg_verify_batch": (BATCH, "stats", BATCH_HOST, (KEYS_AND_MODE, "keys is NULL")),
    "cg_pool_verify_batch": (BATCH, "stats", BATCH_HOST, (KEYS_AND_MODE, "keys is NULL")),
    "cg_verify_transactions_device": (TXN, "hip", TXN_DEV, (KEYS_AND_MODE, "bad mode")),
    "cg_verify_transactions": (TXN, "", TXN_HOST, (KEYS_AND_MODE, "keys is NULL")),
    "cg_pool_verify_transactions": (TXN, "stats", TXN_HOST, (KEYS_AND_MODE, "keys is NULL")),
    "cg_verify_tx_signatures_device": (TXSIG, "hip", TXSIG_ALL, (KEYS_AND_MODE, "keys is NULL")),
    "cg_verify_tx_signatures_packed_device": (TXSIG12, "hip", TXSIG_ALL + STREAM_DEV,
                                              ({"stream": 65, "mode": 2}, "bad mode")),
    "cg_verify_tx_signatures_packed": (TXSIG12, "stats", TXSIG_ALL + STREAM_HOST, (KEYS_AND_MODE, "keys is NULL")),
    "cg_verify_tx_signatures": (TXSIG, "stats", TXSIG_ALL + STREAM_HOST[:1], (KEYS_AND_MODE, "keys is NULL")),
    "cg_pool_verify_tx_signatures": (TXSIG, "stats", TXSIG_ALL + STREAM_HOST[:1], (KEYS_AND_MODE, "keys is NULL")),
    "cg_pool_verify_tx_signatures_packed": (TXSIG12, "stats", TXSIG_ALL + STREAM_HOST, (KEYS_AND_MODE, "keys is NULL")),
    "cg_tx_verdicts_device": (TXV, "hip", TXV_ALL, ({"keys": None, "stride": 16}, STRIDE)),
    "cg_tx_verdicts": (TXV, "", TXV_ALL + [BAD_CHECKS], ({"keys": None, "stride": 16}, STRIDE)),
    "cg_verify_required_signatures_packed_device": (REQ, "hip", TXSIG_ALL + TXV_TABLES + STREAM_DEV,
                                                    ({"checks": None, "stream": 65}, "NULL checks / verdicts")),
    # status_out may be NULL in the host form: no refusal
    "cg_verify_required_signatures_packed": (REQ, "stats", [TXSIG_ALL[0]] + TXSIG_HEAD + TXV_TABLES + [BAD_CHECKS]
                                             + STREAM_HOST, (KEYS_AND_MODE, "keys is NULL")),
    # the pool form checks its tables first, then runs the pool's packed call, which reports under its own name
    "cg_pool_verify_required_signatures_packed": (
        REQ, "stats", [({"sigs": None}, TXV_SIG), ({"keys": None}, "keys is NULL")] + TXV_TABLES + [BAD_CHECKS]
        + [(bad, (INNER, text)) for bad, text in TXSIG_HEAD[1:] + STREAM_HOST], (KEYS_AND_MODE, "keys is NULL")),
    "cg_build_filtered_device": (BUILD_TX, "hip", BUILD_HEAD + BUILD_ALIGN + BUILD_TX_IN, TABLE_FIRST),
    "cg_build_filtered": (BUILD_TX, "", BUILD_HEAD + BUILD_TX_IN + [({"arena": None}, "NULL buffer")], TABLE_FIRST),
    "cg_build_partial_trees_device": (BUILD_PT_DEV, "hip", BUILD_HEAD + BUILD_ALIGN + BUILD_PT_DEV_IN, TABLE_FIRST),
    "cg_build_partial_trees": (BUILD_PT, "", BUILD_HEAD + BUILD_PT_IN, TABLE_FIRST),
}
COUNTS = dict(n_keys=1, n_items=1, n_tx=1, n_comps=1, n_sigs=1, n_tmpls=1, n_ids=1, n_reqs=1, n_nodes=1, arena_len=64,
              mode=0, stride=12, out_base=0, node_cap=1, leaf_cap=1, out_cap=32, n=1, leaf_total=1, n_leaf_hashes=1,
              n_inc_hashes=1)
RESULTS = ("status", "ids", "tx_status", "sig_status", "verdicts", "req_status", "ftxs", "node_rows", "leaves", "out",
           "totals")


def test_every_refusal_in_order(engine):
    import torch
    from corda_amd.engine import EnginePool
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    h_in, h_out = np.zeros(4096, np.uint8), np.full(4096, 0xA5, np.uint8)
    h_fill = np.full(4096, 0xA5, np.uint8)  # what the pool's required-signatures form marks "nothing ran" on a refusal
    d_in = torch.zeros(4096, dtype=torch.uint8, device=dev)
    d_out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    reserved = np.zeros(1, B.TX_CHECK_DTYPE)
    reserved["reserved"] = 1
    torch.cuda.synchronize()
    n_calls = 0
    with EnginePool([0]) as pool:
        for name, (params, tail, refusals, both) in ENTRIES.items():
            device, inner_fill = tail == "hip", name == "cg_pool_verify_required_signatures_packed"
            good = dict(COUNTS)
            for k in params.split():
                if k in RESULTS:
                    good[k] = (d_out.data_ptr() if device else
                               h_fill.ctypes.data if inner_fill and k != "status" else h_out.ctypes.data)
                elif k == "stream":  # the 12-byte form's stream: a host buffer, or an offset into the device arena
                    good[k] = 0 if device else h_in.ctypes.data
                elif k == "stream_len":
                    good[k] = 16
                elif k == "tmpls":  # host memory in every form
                    good[k] = h_in.ctypes.data
                elif k not in good:
                    good[k] = d_in.data_ptr() if device else h_in.ctypes.data
            handle = pool._h if name.startswith("cg_pool_") else engine._h

            def call(bad, h=handle):
                a = dict(good, **{k: good[k] + 1 if v is ODD else v for k, v in bad.items() if k in good})
                if a.get("checks") == "reserved":
                    a["checks"] = reserved.ctypes.data
                return getattr(L, name)(h, *[a[k] for k in params.split()], *([None] if tail else []))

            assert call({}, None) == -1
            assert _lib.last_error() == f"{name}: {'pool' if name.startswith('cg_pool_') else 'ctx'} is NULL"
            for bad, text in refusals + ([both] if both else []):
                fn, text = text if isinstance(text, tuple) else (name, text)
                assert call(bad) == -1, (name, bad)
                assert _lib.last_error() == f"{fn}: {text}", (name, bad)
                n_calls += 1
    torch.cuda.synchronize()
    assert n_calls > 150
    assert np.all(h_out == 0xA5) and bool(torch.all(d_out == 0xA5)), "a refused call wrote to a result buffer"
