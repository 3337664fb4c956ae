"""One MI355X verification context (``cg_ctx``) per device, over the C ABI.

``Engine.verify(batch)`` is the batch form of Crypto.isValid / Crypto.doVerify
(core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:474-484,553-559): one status byte
per item, codes as in include/cordagpu.h. ``Engine.verify_device`` is the same on
buffers already resident in HBM (raw device pointers, e.g. ``torch.Tensor.data_ptr()``).
"""
import collections
import ctypes

import numpy as np

from . import _lib
from .batch import COMPONENT_DTYPE, FLEAF_DTYPE, FTX_DTYPE, KEY_DTYPE, PMT_NODE_DTYPE, MODE_DOVERIFY, SPAN_DTYPE, TMPL_DTYPE, TX_DTYPE, TXSIG_DTYPE
from .batch import BUILD_TOTALS_DTYPE
from .batch import REQ_NODE_DTYPE, TX_CHECK_DTYPE, TX_VERDICT_DTYPE, TXSIG12_DTYPE
from .batch import SIGN_ITEM_DTYPE, SIGN_REQ_DTYPE
from .batch import DERIVE_PARENT_DTYPE, DERIVE_REQ_DTYPE


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


class Engine:
    def __init__(self, device=0, chunk_items=0, stage_timing=False, host_threads=0, table_bytes_max=0, rsa=False,
                 key_cache=True):
        """key_cache=False: CG_FLAG_NO_KEY_CACHE, every call builds its hot keys' wide tables. rsa: CG_FLAG_RSA, RSA_SHA256 items with a key the device decode accepts are verified on the
        GPU (off: they stay UNSUPPORTED, as every other RSA key does either way); host_threads: cg_config.host_threads (0: CG_HOST_THREADS, else the CPU quota divided by the
        contexts open in this process); table_bytes_max: HBM the constant fixed-base tables may take
        (0: automatic; include/cordagpu.h, corda_amd/csrc/table_budget.h)."""
        L = _lib.lib()
        flags = (_lib.FLAG_STAGE_TIMING if stage_timing else 0) | (_lib.FLAG_RSA if rsa else 0)
        flags |= 0 if key_cache else _lib.FLAG_NO_KEY_CACHE
        cfg = _lib.cg_config(device, flags, 0, 0, chunk_items, host_threads, 0, table_bytes_max)
        h = ctypes.c_void_p()
        _lib.check(L.cg_open(ctypes.byref(h), ctypes.byref(cfg)), f"cg_open(device={device})")
        self._h = h
        self.device = device
        self.rsa = bool(rsa)
        self.last_stats = None

    def info(self):
        """cg_context_info: device, fixed_base_bits (26 / 24 / 22), table_bytes, host_threads, chunk_items."""
        inf = _lib.cg_info()
        _lib.check(_lib.lib().cg_context_info(self._h, ctypes.byref(inf)), "cg_context_info")
        return {k: getattr(inf, k) for k, _ in _lib.cg_info._fields_ if k != "reserved"}

    def close(self):
        if self._h:
            _lib.lib().cg_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stage_times(self):
        """{stage: (ms, launches)} since the last read (Engine(stage_timing=True)); waits for the work."""
        n = len(_lib.STAGE_NAMES)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_uint32 * n)()
        rc = _lib.lib().cg_stage_times(self._h, ms, cnt, n)
        if rc < 0:
            _lib.check(rc, "cg_stage_times")
        return {name: (ms[k], cnt[k]) for k, name in enumerate(_lib.STAGE_NAMES)}

    def key_cache_stats(self):
        """cg_key_cache_stats (waits for the context's stream): enabled, slots, and the last call's hits, built,
        evicted and fell_back, each a pair (Ed25519 pool, ECDSA pool)."""
        inf = _lib.cg_key_cache_info()
        _lib.check(_lib.lib().cg_key_cache_stats(self._h, ctypes.byref(inf)), "cg_key_cache_stats")
        out = {"enabled": bool(inf.enabled), "slots": inf.slots}
        for k in ("hits", "built", "evicted", "fell_back"):
            out[k] = tuple(getattr(inf, k))
        return out

    # ------------------------------------------------------------------ signatures
    def verify(self, batch, mode=MODE_DOVERIFY):
        st = np.full(batch.n, 255, dtype=np.uint8)
        stats = _lib.cg_stats()
        rc = _lib.lib().cg_verify_batch(self._h, _p(batch.keys), len(batch.keys), _p(batch.items), batch.n,
                                        _p(batch.arena), batch.arena.size, mode, _p(st), ctypes.byref(stats))
        _lib.check(rc, "cg_verify_batch")
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_stats._fields_}
        return st

    def reserve(self, max_keys, max_items):
        _lib.check(_lib.lib().cg_reserve(self._h, max_keys, max_items), "cg_reserve")

    def verify_device(self, d_keys, n_keys, d_items, n_items, d_arena, arena_len, d_status, mode=MODE_DOVERIFY,
                      stream=0):
        """Asynchronous: enqueues on `stream` (a hipStream_t as int; 0 = the context's stream)."""
        rc = _lib.lib().cg_verify_batch_device(self._h, d_keys, n_keys, d_items, n_items, d_arena, arena_len, mode,
                                               d_status, stream or None)
        _lib.check(rc, "cg_verify_batch_device")

    def prepare_keys_device(self, d_keys, n_keys, d_arena, arena_len, stream=0):
        _lib.check(_lib.lib().cg_prepare_keys_device(self._h, d_keys, n_keys, d_arena, arena_len, stream or None),
                   "cg_prepare_keys_device")

    def verify_items_device(self, d_keys, n_keys, d_items, n_items, d_arena, arena_len, d_status,
                            mode=MODE_DOVERIFY, stream=0):
        rc = _lib.lib().cg_verify_items_device(self._h, d_keys, n_keys, d_items, n_items, d_arena, arena_len, mode,
                                               d_status, stream or None)
        _lib.check(rc, "cg_verify_items_device")

    # ------------------------------------------------------------------ hashing
    @staticmethod
    def _spans(msgs):
        chunks, spans, off = [], np.zeros(len(msgs), dtype=SPAN_DTYPE), 0
        for i, m in enumerate(msgs):
            pad = (-off) % 4
            if pad:
                chunks.append(bytes(pad))
                off += pad
            spans[i] = (off, len(m))
            chunks.append(bytes(m))
            off += len(m)
        arena = np.frombuffer(b"".join(chunks) + bytes(8), dtype=np.uint8).copy()
        return spans, arena

    def sha256(self, msgs):
        spans, arena = self._spans(msgs)
        out = np.zeros(32 * len(msgs), dtype=np.uint8)
        _lib.check(_lib.lib().cg_sha256_batch(self._h, _p(spans), len(msgs), _p(arena), arena.size - 8, _p(out)),
                   "cg_sha256_batch")
        return [out[32 * i:32 * i + 32].tobytes() for i in range(len(msgs))]

    def sha512(self, msgs):
        spans, arena = self._spans(msgs)
        out = np.zeros(64 * len(msgs), dtype=np.uint8)
        _lib.check(_lib.lib().cg_sha512_batch(self._h, _p(spans), len(msgs), _p(arena), arena.size - 8, _p(out)),
                   "cg_sha512_batch")
        return [out[64 * i:64 * i + 64].tobytes() for i in range(len(msgs))]

    def merkle_roots(self, leaf_lists):
        """MerkleTree.getMerkleTree(leaves).hash for each list; returns (roots, status)."""
        n = len(leaf_lists)
        first = np.zeros(n, dtype=np.uint64)
        count = np.zeros(n, dtype=np.uint32)
        flat, pos = [], 0
        for j, lv in enumerate(leaf_lists):
            first[j] = pos
            count[j] = len(lv)
            flat.extend(bytes(x) for x in lv)
            pos += len(lv)
        leaves = np.frombuffer(b"".join(flat) + bytes(32), dtype=np.uint8).copy()
        roots = np.zeros(32 * n, dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        _lib.check(_lib.lib().cg_merkle_roots(self._h, _p(leaves), _p(first), _p(count), n, _p(roots), _p(st)),
                   "cg_merkle_roots")
        return [roots[32 * j:32 * j + 32].tobytes() for j in range(n)], st

    def tx_ids(self, txs, comps, arena):
        """WireTransaction.id for packed transactions (TX_DTYPE / COMPONENT_DTYPE / arena)."""
        assert txs.dtype == TX_DTYPE and comps.dtype == COMPONENT_DTYPE
        ids = np.zeros(32 * len(txs), dtype=np.uint8)
        st = np.zeros(len(txs), dtype=np.uint8)
        _lib.check(_lib.lib().cg_tx_ids(self._h, _p(txs), len(txs), _p(comps), len(comps), _p(arena), arena.size,
                                        _p(ids), _p(st)), "cg_tx_ids")
        return ids.reshape(-1, 32), st

    def tx_ids_device(self, d_txs, n_tx, d_comps, n_comps, d_arena, arena_len, d_ids, d_status, stream=0):
        """Asynchronous device form of tx_ids (every table already in HBM)."""
        _lib.check(_lib.lib().cg_tx_ids_device(self._h, d_txs, n_tx, d_comps, n_comps, d_arena, arena_len, d_ids,
                                               d_status, stream or None), "cg_tx_ids_device")

    def verify_filtered(self, ftxs, nodes, leaves, arena):
        """FilteredTransaction.verify / PartialMerkleTree.verify for packed tear-offs
        (FTX_DTYPE / PMT_NODE_DTYPE / FLEAF_DTYPE / arena, cg_verify_filtered). Returns the
        per-transaction status bytes (0 true, 1 false, 2 MerkleTreeException, 3 malformed)."""
        assert ftxs.dtype == FTX_DTYPE and nodes.dtype == PMT_NODE_DTYPE and leaves.dtype == FLEAF_DTYPE
        st = np.full(len(ftxs), 255, dtype=np.uint8)
        _lib.check(_lib.lib().cg_verify_filtered(self._h, _p(ftxs), len(ftxs), _p(nodes), len(nodes), _p(leaves),
                                                 len(leaves), _p(arena), arena.size, _p(st)), "cg_verify_filtered")
        return st

    def verify_filtered_device(self, d_ftxs, n_ftx, d_nodes, n_nodes, d_leaves, n_leaves, d_arena, arena_len,
                               d_status, stream=0):
        """Asynchronous device form of verify_filtered (every table already in HBM)."""
        _lib.check(_lib.lib().cg_verify_filtered_device(self._h, d_ftxs, n_ftx, d_nodes, n_nodes, d_leaves, n_leaves,
                                                        d_arena, arena_len, d_status, stream or None),
                   "cg_verify_filtered_device")

    @staticmethod
    def _build_tables(n, node_cap, leaf_cap, slot_cap):
        return (np.zeros(n, FTX_DTYPE), np.zeros(node_cap, PMT_NODE_DTYPE), np.zeros(leaf_cap, FLEAF_DTYPE),
                np.zeros(32 * slot_cap, np.uint8), np.full(n, 255, np.uint8), np.zeros(1, BUILD_TOTALS_DTYPE))

    @staticmethod
    def _build_trim(ftxs, nodes, leaves, out, st, totals):
        t = totals[0]
        return (ftxs, nodes[:int(t["n_nodes"])], leaves[:int(t["n_leaves"])], out[:int(t["out_bytes"])], st, t)

    def build_filtered(self, txs, comps, arena, visible, out_base=0):
        """WireTransaction.buildFilteredTransaction for packed transactions (cg_build_filtered): ``visible`` is one
        byte per component. Returns (ftxs, nodes, leaves, out, status, totals): the tables of verify_filtered,
        whose offsets into ``out`` have ``out_base`` added; status 0 built, 1 / 2 / 3 as tx_ids, 6 a visible
        byte that is not 0 or 1 or a visible privacy salt."""
        assert txs.dtype == TX_DTYPE and comps.dtype == COMPONENT_DTYPE
        visible = np.ascontiguousarray(visible, np.uint8)
        assert visible.size == len(comps)
        nc = len(comps)
        t = self._build_tables(len(txs), 4 * nc, nc, len(txs) + 3 * nc)
        ftxs, nodes, leaves, out, st, totals = t
        _lib.check(_lib.lib().cg_build_filtered(self._h, _p(txs), len(txs), _p(comps), nc, _p(arena), arena.size,
                                                _p(visible), out_base, _p(ftxs), _p(nodes), len(nodes), _p(leaves),
                                                len(leaves), _p(out), out.size, _p(st), _p(totals)),
                   "cg_build_filtered")
        return self._build_trim(*t)

    def build_filtered_device(self, d_txs, n_tx, d_comps, n_comps, d_arena, arena_len, d_visible, out_base, d_ftxs,
                              d_nodes, node_cap, d_leaves, leaf_cap, d_out, out_cap, d_status, d_totals, stream=0):
        """Asynchronous device form of build_filtered (every table already in HBM; d_totals: a
        BUILD_TOTALS_DTYPE record, ``over`` set where a capacity was too small)."""
        _lib.check(_lib.lib().cg_build_filtered_device(self._h, d_txs, n_tx, d_comps, n_comps, d_arena, arena_len,
                                                       d_visible, out_base, d_ftxs, d_nodes, node_cap, d_leaves,
                                                       leaf_cap, d_out, out_cap, d_status, d_totals, stream or None),
                   "cg_build_filtered_device")

    @staticmethod
    def _hash_lists(lists):
        first = np.zeros(len(lists), np.uint64)
        count = np.zeros(len(lists), np.uint32)
        flat = []
        for j, lv in enumerate(lists):
            first[j], count[j] = len(flat), len(lv)
            flat.extend(bytes(x) for x in lv)
        if any(len(x) != 32 for x in flat):
            raise ValueError("a SHA-256 hash is 32 bytes")
        return np.frombuffer(b"".join(flat) + bytes(32), np.uint8).copy(), first, count

    def build_partial_trees(self, leaf_lists, include_lists, out_base=0):
        """PartialMerkleTree.build(tree, includeHashes) for each (leaf list, include list) pair
        (cg_build_partial_trees). Returns the tables of build_filtered; status 0 built, 1 no leaves, 4 a zero
        hash in the include list, 5 the included leaves are not the include list."""
        assert len(leaf_lists) == len(include_lists)
        leaves, first, count = self._hash_lists(leaf_lists)
        include, inc_first, inc_count = self._hash_lists(include_lists)
        n, nl, ni = len(leaf_lists), int(count.sum()), int(inc_count.sum())
        t = self._build_tables(n, 4 * nl, ni, n + ni + 2 * nl)
        ftxs, nodes, lrec, out, st, totals = t
        _lib.check(_lib.lib().cg_build_partial_trees(self._h, _p(leaves), _p(first), _p(count), n, _p(include),
                                                     _p(inc_first), _p(inc_count), out_base, _p(ftxs), _p(nodes),
                                                     len(nodes), _p(lrec), len(lrec), _p(out), out.size, _p(st),
                                                     _p(totals)), "cg_build_partial_trees")
        return self._build_trim(*t)

    def build_partial_trees_device(self, d_leaves, n_leaf_hashes, d_first, d_count, n, leaf_total, d_include,
                                   n_inc_hashes, d_inc_first, d_inc_count, out_base, d_ftxs, d_nodes, node_cap,
                                   d_leaves_out, leaf_cap, d_out, out_cap, d_status, d_totals, stream=0):
        """Asynchronous device form of build_partial_trees."""
        _lib.check(_lib.lib().cg_build_partial_trees_device(self._h, d_leaves, n_leaf_hashes, d_first, d_count, n,
                                                            leaf_total, d_include, n_inc_hashes, d_inc_first,
                                                            d_inc_count, out_base, d_ftxs, d_nodes, node_cap,
                                                            d_leaves_out, leaf_cap, d_out, out_cap, d_status,
                                                            d_totals, stream or None),
                   "cg_build_partial_trees_device")

    # ------------------------------------------------------------------ transactions
    def verify_transactions(self, txs, comps, keys, sigs, tmpls, arena, mode=MODE_DOVERIFY):
        """Tx ids + every signature over SignableData(id, metadata) in one call
        (cg_verify_transactions). Returns (ids [n_tx, 32], tx_status, sig_status)."""
        assert txs.dtype == TX_DTYPE and comps.dtype == COMPONENT_DTYPE and keys.dtype == KEY_DTYPE
        assert sigs.dtype == TXSIG_DTYPE and tmpls.dtype == TMPL_DTYPE
        ids = np.zeros(32 * len(txs), dtype=np.uint8)
        txst = np.zeros(len(txs), dtype=np.uint8)
        sst = np.full(len(sigs), 255, dtype=np.uint8)
        rc = _lib.lib().cg_verify_transactions(self._h, _p(txs), len(txs), _p(comps), len(comps), _p(keys), len(keys),
                                               _p(sigs), len(sigs), _p(tmpls), len(tmpls), _p(arena), arena.size,
                                               mode, _p(ids), _p(txst), _p(sst))
        _lib.check(rc, "cg_verify_transactions")
        return ids.reshape(-1, 32), txst, sst

    def verify_transactions_device(self, d_txs, n_tx, d_comps, n_comps, d_keys, n_keys, d_sigs, n_sigs, tmpls,
                                   d_arena, arena_len, d_ids, d_tx_status, d_sig_status, mode=MODE_DOVERIFY,
                                   stream=0):
        """Asynchronous device form; `tmpls` is a host TMPL_DTYPE array (template bytes in the arena)."""
        assert tmpls.dtype == TMPL_DTYPE
        rc = _lib.lib().cg_verify_transactions_device(self._h, d_txs, n_tx, d_comps, n_comps, d_keys, n_keys, d_sigs,
                                                      n_sigs, _p(tmpls), len(tmpls), d_arena, arena_len, mode, d_ids,
                                                      d_tx_status, d_sig_status, stream or None)
        _lib.check(rc, "cg_verify_transactions_device")

    # ------------------------------------------------------------------ signatures over tx ids
    def verify_tx_signatures(self, tb, mode=MODE_DOVERIFY):
        """Batch Crypto.doVerify(txId, TransactionSignature) (cg_verify_tx_signatures, Crypto.kt:499-502):
        ``tb`` is a batch.TxSigBatch; each signature's clear data is SignableData(id, metadata),
        spliced on the device. Returns one status byte per signature; cg_stats in last_stats."""
        st = np.full(len(tb.sigs), 255, dtype=np.uint8)
        stats = _lib.cg_stats()
        rc = _lib.lib().cg_verify_tx_signatures(self._h, _p(tb.keys), len(tb.keys), _p(tb.ids), tb.n_ids, _p(tb.sigs),
                                                len(tb.sigs), _p(tb.tmpls), len(tb.tmpls), _p(tb.arena), tb.arena.size,
                                                mode, _p(st), ctypes.byref(stats))
        _lib.check(rc, "cg_verify_tx_signatures")
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_stats._fields_}
        return st

    def verify_tx_signatures_packed(self, pb, mode=MODE_DOVERIFY):
        """cg_verify_tx_signatures_packed: ``pb`` a batch.PackedTxSigBatch (the 12-byte table and the
        dense signature stream). One status byte per signature; cg_stats in last_stats."""
        st = np.full(pb.n, 255, dtype=np.uint8)
        stats = _lib.cg_stats()
        rc = _lib.lib().cg_verify_tx_signatures_packed(self._h, _p(pb.keys), len(pb.keys), _p(pb.ids), pb.n_ids,
                                                       _p(pb.sigs), pb.n, _p(pb.stream), pb.stream.size, _p(pb.tmpls),
                                                       len(pb.tmpls), _p(pb.arena), pb.arena.size, mode, _p(st),
                                                       ctypes.byref(stats))
        _lib.check(rc, "cg_verify_tx_signatures_packed")
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_stats._fields_}
        return st

    def verify_tx_signatures_packed_device(self, d_keys, n_keys, d_ids, n_ids, d_sigs, n_sigs, sig_bytes_off,
                                           sig_bytes_len, tmpls, d_arena, arena_len, d_status, mode=MODE_DOVERIFY,
                                           stream=0):
        """Asynchronous device form: the signature stream at d_arena[sig_bytes_off, + sig_bytes_len)."""
        assert tmpls.dtype == TMPL_DTYPE
        rc = _lib.lib().cg_verify_tx_signatures_packed_device(self._h, d_keys, n_keys, d_ids, n_ids, d_sigs, n_sigs,
                                                              sig_bytes_off, sig_bytes_len, _p(tmpls), len(tmpls),
                                                              d_arena, arena_len, mode, d_status, stream or None)
        _lib.check(rc, "cg_verify_tx_signatures_packed_device")

    def verify_tx_signatures_device(self, d_keys, n_keys, d_ids, n_ids, d_sigs, n_sigs, tmpls, d_arena, arena_len,
                                    d_status, mode=MODE_DOVERIFY, stream=0):
        """Asynchronous device form; `tmpls` is a host TMPL_DTYPE array (template bytes in the arena)."""
        assert tmpls.dtype == TMPL_DTYPE
        rc = _lib.lib().cg_verify_tx_signatures_device(self._h, d_keys, n_keys, d_ids, n_ids, d_sigs, n_sigs,
                                                       _p(tmpls), len(tmpls), d_arena, arena_len, mode, d_status,
                                                       stream or None)
        _lib.check(rc, "cg_verify_tx_signatures_device")

    # ------------------------------------------------------------------ Ed25519 signing
    def load_signers(self, seeds):
        """cg_signers_load: EdDSAPrivateKeySpec(seed) for each 32-byte seed; replaces the context's signer
        set and returns each key's 32-byte Abyte, for the key-pair check of Crypto.kt:416-419. The
        seeds (bytes-like objects) are copied once, into the array handed to the C ABI, and that array is
        zeroed before this returns; the caller's objects are not touched."""
        return _load_signers(_lib.lib().cg_signers_load, "cg_signers_load", self._h, seeds)

    def clear_signers(self):
        _lib.check(_lib.lib().cg_signers_clear(self._h), "cg_signers_clear")

    def sign_tx_ids(self, sr):
        """Batch Crypto.doSign(keyPair, SignableData(txId, metadata)) (cg_sign_tx_ids, Crypto.kt:415-422;
        NotaryService.kt:77-80): ``sr`` is a batch.SignRequests. Returns (signatures uint8 [n, 64],
        status uint8 [n]); a request that was not signed has 64 zero bytes."""
        assert sr.reqs.dtype == SIGN_REQ_DTYPE and sr.tmpls.dtype == TMPL_DTYPE
        sigs = np.zeros(64 * sr.n, dtype=np.uint8)
        st = np.full(sr.n, 255, dtype=np.uint8)
        rc = _lib.lib().cg_sign_tx_ids(self._h, _p(sr.ids), sr.n_ids, _p(sr.reqs), sr.n, _p(sr.tmpls), len(sr.tmpls),
                                       _p(sr.arena), sr.arena.size, _p(sigs), _p(st))
        _lib.check(rc, "cg_sign_tx_ids")
        return sigs.reshape(-1, 64), st

    def sign_tx_ids_device(self, d_ids, n_ids, d_reqs, n, tmpls, d_arena, arena_len, d_sigs, d_status, stream=0):
        """Asynchronous device form; `tmpls` is a host TMPL_DTYPE array (template bytes in the arena)."""
        assert tmpls.dtype == TMPL_DTYPE
        rc = _lib.lib().cg_sign_tx_ids_device(self._h, d_ids, n_ids, d_reqs, n, _p(tmpls), len(tmpls), d_arena,
                                              arena_len, d_sigs, d_status, stream or None)
        _lib.check(rc, "cg_sign_tx_ids_device")

    def sign(self, signer_msgs):
        """Batch Crypto.doSign(privateKey, clearData) (cg_sign_batch, Crypto.kt:395-402) over
        (signer index, message bytes) pairs. Returns (signatures uint8 [n, 64], status uint8 [n])."""
        n = len(signer_msgs)
        spans, arena = self._spans([m for _, m in signer_msgs])
        items = np.zeros(n, dtype=SIGN_ITEM_DTYPE)
        items["msg_off"], items["msg_len"] = spans["off"], spans["len"]
        items["signer"] = [s for s, _ in signer_msgs]
        sigs = np.zeros(64 * n, dtype=np.uint8)
        st = np.full(n, 255, dtype=np.uint8)
        rc = _lib.lib().cg_sign_batch(self._h, _p(items), n, _p(arena), arena.size - 8, _p(sigs), _p(st))
        _lib.check(rc, "cg_sign_batch")
        return sigs.reshape(-1, 64), st

    # ------------------------------------------------------------------ ECDSA signing
    def load_ec_signers(self, keys):
        """cg_ec_signers_load: replaces the context's ECDSA signer set (separate from the Ed25519 one) with
        ``keys``, (scheme 2 / 3, 32-byte big-endian d) pairs. Returns (X || Y per key, load status uint8
        [n]); a refused key (KEY_INVALID: d = 0 or d >= n; UNSUPPORTED: another scheme) has zero bytes. The
        staging copy of the d bytes is zeroed before this returns."""
        return _load_ec_signers(_lib.lib().cg_ec_signers_load, "cg_ec_signers_load", self._h, keys)

    def clear_ec_signers(self):
        _lib.check(_lib.lib().cg_ec_signers_clear(self._h), "cg_ec_signers_clear")

    def sign_ec_tx_ids(self, sr, nonces):
        """Batch Crypto.doSign(keyPair, SignableData(txId, metadata)) for ECDSA keys (cg_ec_sign_tx_ids):
        ``sr`` is a batch.SignRequests over the ECDSA signer set, ``nonces`` the requests' 32-byte
        big-endian k candidates (what BC's RandomDSAKCalculator.nextK would have drawn). Returns
        (signature slots uint8 [n, 72], lengths uint8 [n], status uint8 [n]); an item with status
        NONCE_REJECTED is the caller's to redraw and resubmit. The nonce array handed to the C ABI is
        zeroed before this returns: a C-contiguous uint8 array is that array (the caller sees it zeroed);
        a list of bytes objects is copied into one, and the caller's immutable copies stay in memory."""
        assert sr.reqs.dtype == SIGN_REQ_DTYPE and sr.tmpls.dtype == TMPL_DTYPE
        fn = _lib.lib().cg_ec_sign_tx_ids
        return _sign_ec(lambda k, sigs, ln, st: fn(self._h, _p(sr.ids), sr.n_ids, _p(sr.reqs), sr.n, _p(sr.tmpls),
                                                   len(sr.tmpls), _p(sr.arena), sr.arena.size, k, sigs, ln, st),
                        "cg_ec_sign_tx_ids", sr.n, nonces)

    def sign_ec_tx_ids_device(self, d_ids, n_ids, d_reqs, n, tmpls, d_arena, arena_len, d_nonces, d_sigs, d_sig_len,
                              d_status, stream=0):
        """Asynchronous device form; `tmpls` is a host TMPL_DTYPE array (template bytes in the arena). The
        caller owns, and zeroes, d_nonces."""
        assert tmpls.dtype == TMPL_DTYPE
        rc = _lib.lib().cg_ec_sign_tx_ids_device(self._h, d_ids, n_ids, d_reqs, n, _p(tmpls), len(tmpls), d_arena,
                                                 arena_len, d_nonces, d_sigs, d_sig_len, d_status, stream or None)
        _lib.check(rc, "cg_ec_sign_tx_ids_device")

    def sign_ec(self, signer_msgs, nonces):
        """Batch Crypto.doSign(privateKey, clearData) for ECDSA keys (cg_ec_sign_batch) over (signer index,
        message bytes) pairs. Returns what sign_ec_tx_ids returns."""
        n = len(signer_msgs)
        spans, arena = self._spans([m for _, m in signer_msgs])
        items = np.zeros(n, dtype=SIGN_ITEM_DTYPE)
        items["msg_off"], items["msg_len"] = spans["off"], spans["len"]
        items["signer"] = [s for s, _ in signer_msgs]
        fn = _lib.lib().cg_ec_sign_batch
        return _sign_ec(lambda k, sigs, ln, st: fn(self._h, _p(items), n, _p(arena), arena.size - 8, k, sigs, ln, st),
                        "cg_ec_sign_batch", n, nonces)

    # ------------------------------------------------------------------ RSA-PSS signing
    def load_rsa_signers(self, keys):
        """cg_rsa_signers_load: replaces the context's RSA signer set (the third one, separate from the
        Ed25519 and ECDSA sets) with ``keys``: RsaSignerKey tuples (n, e, p, q, dp, dq, qinv), e an int, the
        others big-endian bytes-like objects (the fields of a BCRSAPrivateCrtKey). Returns the load status
        uint8 [n]: 0, KEY_INVALID or UNSUPPORTED (include/cordagpu.h). The staging copy of the secret bytes
        is zeroed before this returns."""
        return _load_rsa_signers(_lib.lib().cg_rsa_signers_load, "cg_rsa_signers_load", self._h, keys)

    def clear_rsa_signers(self):
        _lib.check(_lib.lib().cg_rsa_signers_clear(self._h), "cg_rsa_signers_clear")

    def sign_rsa_tx_ids(self, sr, salts):
        """Batch Crypto.doSign(keyPair, SignableData(txId, metadata)) for RSA keys (cg_rsa_sign_tx_ids):
        ``sr`` is a batch.SignRequests over the RSA signer set, ``salts`` the requests' 32-byte salts (what
        BC's PSSSigner would have drawn). Returns (signature slots uint8 [n, 512], lengths uint16 [n],
        status uint8 [n]). The salt array handed to the C ABI is zeroed before this returns, as
        sign_ec_tx_ids does with its nonces."""
        assert sr.reqs.dtype == SIGN_REQ_DTYPE and sr.tmpls.dtype == TMPL_DTYPE
        fn = _lib.lib().cg_rsa_sign_tx_ids
        return _sign_rsa(lambda k, sigs, ln, st: fn(self._h, _p(sr.ids), sr.n_ids, _p(sr.reqs), sr.n, _p(sr.tmpls),
                                                    len(sr.tmpls), _p(sr.arena), sr.arena.size, k, sigs, ln, st),
                         "cg_rsa_sign_tx_ids", sr.n, salts)

    def sign_rsa_tx_ids_device(self, d_ids, n_ids, d_reqs, n, tmpls, d_arena, arena_len, d_salts, d_sigs, d_sig_len,
                               d_status, stream=0):
        """Asynchronous device form; `tmpls` is a host TMPL_DTYPE array (template bytes in the arena). The
        caller owns, and zeroes, d_salts; d_sig_len holds n uint16."""
        assert tmpls.dtype == TMPL_DTYPE
        rc = _lib.lib().cg_rsa_sign_tx_ids_device(self._h, d_ids, n_ids, d_reqs, n, _p(tmpls), len(tmpls), d_arena,
                                                  arena_len, d_salts, d_sigs, d_sig_len, d_status, stream or None)
        _lib.check(rc, "cg_rsa_sign_tx_ids_device")

    def sign_rsa(self, signer_msgs, salts):
        """Batch Crypto.doSign(privateKey, clearData) for RSA keys (cg_rsa_sign_batch) over (signer index,
        message bytes) pairs. Returns what sign_rsa_tx_ids returns."""
        n = len(signer_msgs)
        spans, arena = self._spans([m for _, m in signer_msgs])
        items = np.zeros(n, dtype=SIGN_ITEM_DTYPE)
        items["msg_off"], items["msg_len"] = spans["off"], spans["len"]
        items["signer"] = [s for s, _ in signer_msgs]
        fn = _lib.lib().cg_rsa_sign_batch
        return _sign_rsa(lambda k, sigs, ln, st: fn(self._h, _p(items), n, _p(arena), arena.size - 8, k, sigs, ln, st),
                         "cg_rsa_sign_batch", n, salts)

    # ------------------------------------------------------------------ key derivation
    def derive_keys(self, dr):
        """Batch Crypto.deriveKeyPair(privateKey, seed) (cg_derive_keys, Crypto.kt:646-771): ``dr`` is a
        batch.DeriveRequests. Returns (secrets uint8 [n, 32], public keys uint8 [n, 64], status uint8 [n],
        rehashes uint8 [n]). Ed25519: the child seed, Abyte then 32 zero bytes; ECDSA: d and X || Y,
        big-endian. An item whose status is not 0 has zero bytes; DERIVE_HOST items are the caller's to
        finish (Crypto.derive_key_pairs does, with corda_amd/derive.py)."""
        return _derive_keys(_lib.lib().cg_derive_keys, "cg_derive_keys", self._h, dr)

    def derive_keys_device(self, d_parents, n_parents, d_reqs, n, d_arena, arena_len, d_secrets, d_pubs, d_status,
                           d_retries=None, stream=0):
        """Asynchronous device form: every table in HBM."""
        rc = _lib.lib().cg_derive_keys_device(self._h, d_parents, n_parents, d_reqs, n, d_arena, arena_len, d_secrets,
                                              d_pubs, d_status, d_retries or None, stream or None)
        _lib.check(rc, "cg_derive_keys_device")

    def public_keys(self, scheme, secrets):
        """cg_public_keys: the public key of each 32-byte private key of one scheme (Ed25519: the seed;
        ECDSA: a candidate d, big-endian). Returns (public keys uint8 [n, 64], status uint8 [n]); a
        refused ECDSA candidate has status KEY_REJECTED and zero bytes. The staging copy of the secrets is
        zeroed before this returns."""
        return _public_keys(_lib.lib().cg_public_keys, "cg_public_keys", self._h, scheme, secrets)

    def public_keys_device(self, scheme, d_secrets, n, d_pubs, d_status, stream=0):
        rc = _lib.lib().cg_public_keys_device(self._h, scheme, d_secrets, n, d_pubs, d_status, stream or None)
        _lib.check(rc, "cg_public_keys_device")

    # ------------------------------------------------------------------ per-transaction verdicts
    def tx_verdicts(self, sig_table, status, keys, checks, reqs, nodes, key_class=None):
        """cg_tx_verdicts: verifySignaturesExcept's two steps reduced on the device from one status byte
        per record of ``sig_table`` (TXSIG12_DTYPE or TXSIG_DTYPE). Returns (verdicts TX_VERDICT_DTYPE
        [n_tx], req_status uint8 [n_reqs])."""
        return _tx_verdicts(self._h, sig_table, status, keys, checks, reqs, nodes, key_class)

    def tx_verdicts_device(self, d_sig_table, sig_stride, n_sigs, d_status, d_keys, n_keys, d_key_class, d_checks,
                           n_tx, d_reqs, n_reqs, d_nodes, n_nodes, d_verdicts, d_req_status, stream=0):
        """Asynchronous device form of tx_verdicts (raw HBM pointers; d_key_class may be 0)."""
        rc = _lib.lib().cg_tx_verdicts_device(self._h, d_sig_table, sig_stride, n_sigs, d_status, d_keys, n_keys,
                                              d_key_class or None, d_checks, n_tx, d_reqs or None, n_reqs,
                                              d_nodes or None, n_nodes, d_verdicts, d_req_status or None,
                                              stream or None)
        _lib.check(rc, "cg_tx_verdicts_device")

    def verify_required_signatures_packed(self, pb, checks, reqs, nodes, key_class=None, mode=MODE_DOVERIFY,
                                          want_status=False):
        """cg_verify_required_signatures_packed: ``pb`` a batch.PackedTxSigBatch, verified as
        verify_tx_signatures_packed does, and reduced per transaction behind the last verify chunk.
        Returns (verdicts, req_status), and the per-signature statuses too with want_status."""
        _check_tables(checks, reqs, nodes, key_class, len(pb.keys))
        vd = np.zeros(len(checks), dtype=TX_VERDICT_DTYPE)
        rs = np.full(len(reqs), 255, dtype=np.uint8)
        st = np.full(pb.n, 255, dtype=np.uint8) if want_status else None
        stats = _lib.cg_stats()
        rc = _lib.lib().cg_verify_required_signatures_packed(
            self._h, _p(pb.keys), len(pb.keys), _p(pb.ids), pb.n_ids, _p(pb.sigs), pb.n, _p(pb.stream), pb.stream.size,
            _p(pb.tmpls), len(pb.tmpls), _p(pb.arena), pb.arena.size, mode, _p(key_class), _p(checks), len(checks),
            _p(reqs), len(reqs), _p(nodes), len(nodes), _p(st), _p(vd), _p(rs), ctypes.byref(stats))
        _lib.check(rc, "cg_verify_required_signatures_packed")
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_stats._fields_}
        return (vd, rs, st) if want_status else (vd, rs)

    def verify_required_signatures_packed_device(self, d_keys, n_keys, d_ids, n_ids, d_sigs, n_sigs, sig_bytes_off,
                                                 sig_bytes_len, tmpls, d_arena, arena_len, d_key_class, d_checks, n_tx,
                                                 d_reqs, n_reqs, d_nodes, n_nodes, d_status, d_verdicts, d_req_status,
                                                 mode=MODE_DOVERIFY, stream=0):
        """Asynchronous device form: verify_tx_signatures_packed_device, then the verdict kernels."""
        assert tmpls.dtype == TMPL_DTYPE
        rc = _lib.lib().cg_verify_required_signatures_packed_device(
            self._h, d_keys, n_keys, d_ids, n_ids, d_sigs, n_sigs, sig_bytes_off, sig_bytes_len, _p(tmpls), len(tmpls),
            d_arena, arena_len, mode, d_key_class or None, d_checks, n_tx, d_reqs or None, n_reqs, d_nodes or None,
            n_nodes, d_status, d_verdicts, d_req_status or None, stream or None)
        _lib.check(rc, "cg_verify_required_signatures_packed_device")


def _load_signers(fn, what, h, seeds):
    # each seed goes straight from the caller's object into the one array the C ABI reads: no joined or
    # converted intermediate holds the seeds. That array is zeroed below; the caller's own objects are its own.
    seeds = list(seeds)
    views = [np.frombuffer(s, dtype=np.uint8) for s in seeds]
    if not views or any(v.size != 32 for v in views):
        raise ValueError("an Ed25519 private key is a 32-byte seed; at least one is needed")
    buf = np.zeros(32 * len(seeds), dtype=np.uint8)
    for i, v in enumerate(views):
        buf[32 * i:32 * i + 32] = v
    pub = np.zeros(32 * len(seeds), dtype=np.uint8)
    try:
        rc = fn(h, _p(buf), len(seeds), _p(pub))
    finally:
        ctypes.memset(buf.ctypes.data, 0, buf.size)  # the staging copy (the caller's bytes are its own)
    _lib.check(rc, what)
    return [pub[32 * i:32 * i + 32].tobytes() for i in range(len(seeds))]


def _load_ec_signers(fn, what, h, keys):
    keys = list(keys)
    views = [np.frombuffer(d, dtype=np.uint8) for _, d in keys]
    if not views or any(v.size != 32 for v in views):
        raise ValueError("an ECDSA private key is 32 bytes of d, big-endian; at least one is needed")
    n = len(keys)
    schemes = np.array([s if 0 <= s < 256 else 255 for s, _ in keys], dtype=np.uint8)
    buf = np.zeros(32 * n, dtype=np.uint8)
    for i, v in enumerate(views):
        buf[32 * i:32 * i + 32] = v
    pubs = np.zeros(64 * n, dtype=np.uint8)
    st = np.full(n, 255, dtype=np.uint8)
    try:
        rc = fn(h, _p(schemes), _p(buf), n, _p(pubs), _p(st))
    finally:
        ctypes.memset(buf.ctypes.data, 0, buf.size)  # the staging copy (the caller's bytes are its own)
    _lib.check(rc, what)
    return [pubs[64 * i:64 * i + 64].tobytes() for i in range(n)], st


def nonce_array(nonces, n):
    """The 32 n bytes of a sign call's k candidates, from n bytes-like objects or from a uint8 array. A
    C-contiguous uint8 array is used in place: it is the array the C ABI reads, and the caller sees it zeroed."""
    if isinstance(nonces, np.ndarray):
        buf = nonces.reshape(-1) if nonces.dtype == np.uint8 and nonces.flags.c_contiguous else \
            np.ascontiguousarray(nonces, dtype=np.uint8).reshape(-1)
    else:
        buf = np.zeros(32 * n, dtype=np.uint8)
        for i, k in enumerate(nonces):
            v = np.frombuffer(k, dtype=np.uint8)
            if v.size != 32:
                raise ValueError("a nonce candidate is 32 bytes, big-endian")
            buf[32 * i:32 * i + 32] = v
    if buf.size != 32 * n:
        raise ValueError("one 32-byte nonce candidate per request")
    return buf


def _sign_ec(call, what, n, nonces, allow_partial=False):
    buf = nonce_array(nonces, n)
    sigs = np.zeros(72 * n, dtype=np.uint8)
    ln = np.zeros(n, dtype=np.uint8)
    st = np.full(n, 255, dtype=np.uint8)
    try:
        rc = call(_p(buf), _p(sigs), _p(ln), _p(st))
    finally:
        if buf.size:
            ctypes.memset(buf.ctypes.data, 0, buf.size)  # the array the C ABI read
    if rc != 0 and not allow_partial:
        _lib.check(rc, what)
    return sigs.reshape(-1, 72), ln, st


RsaSignerKey = collections.namedtuple("RsaSignerKey", "n e p q dp dq qinv")
RSA_SIGNER_DTYPE = np.dtype([(f, "<u4") for f in ("n_off", "n_len", "p_off", "p_len", "q_off", "q_len", "dp_off",
                                                  "dp_len", "dq_off", "dq_len", "qinv_off", "qinv_len", "e")])
assert RSA_SIGNER_DTYPE.itemsize == 52  # cg_rsa_signer


def _load_rsa_signers(fn, what, h, keys):
    # as _load_signers: each number goes straight from the caller's object into the one array the C ABI reads
    keys = [RsaSignerKey(*k) for k in keys]
    if not keys:
        raise ValueError("at least one RSA private key is needed")
    n = len(keys)
    table = np.zeros(n, dtype=RSA_SIGNER_DTYPE)
    views = [[np.frombuffer(getattr(k, f), dtype=np.uint8) for f in ("n", "p", "q", "dp", "dq", "qinv")] for k in keys]
    buf = np.zeros(max(sum(v.size for vs in views for v in vs), 1), dtype=np.uint8)
    at = 0
    for i, (k, vs) in enumerate(zip(keys, views)):
        if not 0 <= k.e < 1 << 32:
            raise ValueError("the C ABI's public exponent is 32 bits")
        table[i]["e"] = k.e
        for f, v in zip(("n", "p", "q", "dp", "dq", "qinv"), vs):
            table[i][f + "_off"], table[i][f + "_len"] = at, v.size
            buf[at:at + v.size] = v
            at += v.size
    st = np.full(n, 255, dtype=np.uint8)
    try:
        rc = fn(h, _p(table), n, _p(buf), at, _p(st))
    finally:
        ctypes.memset(buf.ctypes.data, 0, buf.size)  # the staging copy (the caller's bytes are its own)
    _lib.check(rc, what)
    return st


def salt_array(salts, n):
    """The 32 n bytes of a sign call's salts, from n bytes-like objects or from a uint8 array; a C-contiguous
    uint8 array is used in place (nonce_array's rule): the caller sees it zeroed."""
    try:
        return nonce_array(salts, n)
    except ValueError:
        raise ValueError("one 32-byte salt per request") from None


def _sign_rsa(call, what, n, salts, allow_partial=False):
    buf = salt_array(salts, n)
    sigs = np.zeros(512 * n, dtype=np.uint8)
    ln = np.zeros(n, dtype=np.uint16)
    st = np.full(n, 255, dtype=np.uint8)
    try:
        rc = call(_p(buf), _p(sigs), _p(ln), _p(st))
    finally:
        if buf.size:
            ctypes.memset(buf.ctypes.data, 0, buf.size)  # the array the C ABI read
    if rc != 0 and not allow_partial:
        _lib.check(rc, what)
    return sigs.reshape(-1, 512), ln, st


def _public_keys(fn, what, h, scheme, secrets, stats=None):
    views = [np.frombuffer(s, dtype=np.uint8) for s in secrets]
    if any(v.size != 32 for v in views):
        raise ValueError("a private key is 32 bytes (an Ed25519 seed, or an ECDSA d big-endian)")
    n = len(views)
    buf = np.zeros(32 * n, dtype=np.uint8)
    for i, v in enumerate(views):
        buf[32 * i:32 * i + 32] = v
    pubs = np.zeros(64 * n, dtype=np.uint8)
    st = np.full(n, 255, dtype=np.uint8)
    args = [h, scheme, _p(buf), n, _p(pubs), _p(st)]
    try:
        rc = fn(*args, ctypes.byref(stats)) if stats is not None else fn(*args)
    finally:
        ctypes.memset(buf.ctypes.data, 0, buf.size)
    _lib.check(rc, what)
    return pubs.reshape(-1, 64), st


def _derive_keys(fn, what, h, dr, stats=None, allow_partial=False):
    assert dr.parents.dtype == DERIVE_PARENT_DTYPE and dr.reqs.dtype == DERIVE_REQ_DTYPE
    n = dr.n
    secrets, pubs = np.zeros(32 * n, dtype=np.uint8), np.zeros(64 * n, dtype=np.uint8)
    st, tries = np.full(n, 255, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    args = [h, _p(dr.parents), len(dr.parents), _p(dr.reqs), n, _p(dr.arena), dr.arena.size, _p(secrets), _p(pubs),
            _p(st), _p(tries)]
    rc = fn(*args, ctypes.byref(stats)) if stats is not None else fn(*args)
    if rc != 0 and not allow_partial:
        _lib.check(rc, what)
    return secrets.reshape(-1, 32), pubs.reshape(-1, 64), st, tries


def _check_tables(checks, reqs, nodes, key_class, n_keys):
    assert checks.dtype == TX_CHECK_DTYPE and nodes.dtype == REQ_NODE_DTYPE and reqs.dtype == np.uint32
    assert key_class is None or (key_class.dtype == np.uint32 and len(key_class) == n_keys)


def _tx_verdicts(h, sig_table, status, keys, checks, reqs, nodes, key_class):
    assert sig_table.dtype in (TXSIG12_DTYPE, TXSIG_DTYPE) and keys.dtype == KEY_DTYPE
    assert status.dtype == np.uint8 and len(status) == len(sig_table)
    _check_tables(checks, reqs, nodes, key_class, len(keys))
    vd = np.zeros(len(checks), dtype=TX_VERDICT_DTYPE)
    rs = np.full(len(reqs), 255, dtype=np.uint8)
    rc = _lib.lib().cg_tx_verdicts(h, _p(sig_table), sig_table.dtype.itemsize, len(sig_table), _p(status), _p(keys),
                                   len(keys), _p(key_class), _p(checks), len(checks), _p(reqs), len(reqs), _p(nodes),
                                   len(nodes), _p(vd), _p(rs))
    _lib.check(rc, "cg_tx_verdicts")
    return vd, rs


class EnginePool:
    """One process, several devices (cg_pool): ``verify(batch)`` shards the items over the healthy
    slots, re-runs a failed slot's shard elsewhere, and returns one status byte per item (items
    no slot could run stay NOT_RUN and raise ``EngineUnavailable`` unless ``allow_partial``)."""

    def __init__(self, devices, chunk_items=0, host_threads=0, table_bytes_max=0, rsa=False):
        L = _lib.lib()
        cfg = _lib.cg_config(0, _lib.FLAG_RSA if rsa else 0, 0, 0, chunk_items, host_threads, 0, table_bytes_max)
        devs = (ctypes.c_int32 * len(devices))(*devices)
        h = ctypes.c_void_p()
        _lib.check(L.cg_pool_open(ctypes.byref(h), devs, len(devices), ctypes.byref(cfg)), "cg_pool_open")
        self._h = h
        self.devices = list(devices)
        self.rsa = bool(rsa)
        self.last_stats = None

    def close(self):
        if self._h:
            _lib.lib().cg_pool_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def healthy(self):
        L = _lib.lib()
        return [L.cg_pool_slot_healthy(self._h, k) == 1 for k in range(L.cg_pool_slots(self._h))]

    def inject_fault(self, slot, fail=True):
        _lib.check(_lib.lib().cg_pool_inject_fault(self._h, slot, 1 if fail else 0), "cg_pool_inject_fault")

    def verify(self, batch, mode=MODE_DOVERIFY, allow_partial=False):
        st = np.full(batch.n, 255, dtype=np.uint8)
        stats = _lib.cg_pool_stats()
        rc = _lib.lib().cg_pool_verify_batch(self._h, _p(batch.keys), len(batch.keys), _p(batch.items), batch.n,
                                             _p(batch.arena), batch.arena.size, mode, _p(st), ctypes.byref(stats))
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        if rc != 0 and not allow_partial:
            _lib.check(rc, "cg_pool_verify_batch")
        return st

    def verify_tx_signatures(self, tb, mode=MODE_DOVERIFY, allow_partial=False):
        """cg_pool_verify_tx_signatures: the signature table sharded over the healthy slots."""
        st = np.full(len(tb.sigs), 255, dtype=np.uint8)
        stats = _lib.cg_pool_stats()
        rc = _lib.lib().cg_pool_verify_tx_signatures(self._h, _p(tb.keys), len(tb.keys), _p(tb.ids), tb.n_ids,
                                                     _p(tb.sigs), len(tb.sigs), _p(tb.tmpls), len(tb.tmpls),
                                                     _p(tb.arena), tb.arena.size, mode, _p(st), ctypes.byref(stats))
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        if rc != 0 and not allow_partial:
            _lib.check(rc, "cg_pool_verify_tx_signatures")
        return st

    def verify_tx_signatures_packed(self, pb, mode=MODE_DOVERIFY, allow_partial=False):
        """cg_pool_verify_tx_signatures_packed: the 12-byte table sharded over the healthy slots."""
        st = np.full(pb.n, 255, dtype=np.uint8)
        stats = _lib.cg_pool_stats()
        rc = _lib.lib().cg_pool_verify_tx_signatures_packed(self._h, _p(pb.keys), len(pb.keys), _p(pb.ids), pb.n_ids,
                                                            _p(pb.sigs), pb.n, _p(pb.stream), pb.stream.size,
                                                            _p(pb.tmpls), len(pb.tmpls), _p(pb.arena), pb.arena.size,
                                                            mode, _p(st), ctypes.byref(stats))
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        if rc != 0 and not allow_partial:
            _lib.check(rc, "cg_pool_verify_tx_signatures_packed")
        return st

    def verify_required_signatures_packed(self, pb, checks, reqs, nodes, key_class=None, mode=MODE_DOVERIFY,
                                          want_status=False, allow_partial=False):
        """cg_pool_verify_required_signatures_packed: the sharded verify, then the reduction on one healthy
        slot; signatures no slot ran surface as NOT_RUN verdicts."""
        _check_tables(checks, reqs, nodes, key_class, len(pb.keys))
        vd = np.zeros(len(checks), dtype=TX_VERDICT_DTYPE)
        rs = np.full(len(reqs), 255, dtype=np.uint8)
        st = np.full(pb.n, 255, dtype=np.uint8) if want_status else None
        stats = _lib.cg_pool_stats()
        rc = _lib.lib().cg_pool_verify_required_signatures_packed(
            self._h, _p(pb.keys), len(pb.keys), _p(pb.ids), pb.n_ids, _p(pb.sigs), pb.n, _p(pb.stream), pb.stream.size,
            _p(pb.tmpls), len(pb.tmpls), _p(pb.arena), pb.arena.size, mode, _p(key_class), _p(checks), len(checks),
            _p(reqs), len(reqs), _p(nodes), len(nodes), _p(st), _p(vd), _p(rs), ctypes.byref(stats))
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        if rc != 0 and not allow_partial:
            _lib.check(rc, "cg_pool_verify_required_signatures_packed")
        return (vd, rs, st) if want_status else (vd, rs)

    def verify_transactions(self, txs, comps, keys, sigs, tmpls, arena, mode=MODE_DOVERIFY, allow_partial=False):
        """cg_pool_verify_transactions: the whole call on one healthy slot, the next one on a device
        fault. Returns (ids [n_tx, 32], tx_status, sig_status) as Engine.verify_transactions."""
        ids = np.zeros(32 * len(txs), dtype=np.uint8)
        txst = np.zeros(len(txs), dtype=np.uint8)
        sst = np.full(len(sigs), 255, dtype=np.uint8)
        stats = _lib.cg_pool_stats()
        rc = _lib.lib().cg_pool_verify_transactions(self._h, _p(txs), len(txs), _p(comps), len(comps), _p(keys),
                                                    len(keys), _p(sigs), len(sigs), _p(tmpls), len(tmpls), _p(arena),
                                                    arena.size, mode, _p(ids), _p(txst), _p(sst), ctypes.byref(stats))
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        if rc != 0 and not allow_partial:
            _lib.check(rc, "cg_pool_verify_transactions")
        return ids.reshape(-1, 32), txst, sst

    def load_signers(self, seeds):
        """cg_pool_signers_load: the signer set on every slot; returns each key's Abyte."""
        return _load_signers(_lib.lib().cg_pool_signers_load, "cg_pool_signers_load", self._h, seeds)

    def clear_signers(self):
        _lib.check(_lib.lib().cg_pool_signers_clear(self._h), "cg_pool_signers_clear")

    def sign_tx_ids(self, sr, allow_partial=False):
        """cg_pool_sign_tx_ids: the whole call on one healthy slot, the next one on a device fault.
        Returns (signatures uint8 [n, 64], status uint8 [n]) as Engine.sign_tx_ids."""
        assert sr.reqs.dtype == SIGN_REQ_DTYPE and sr.tmpls.dtype == TMPL_DTYPE
        sigs = np.zeros(64 * sr.n, dtype=np.uint8)
        st = np.full(sr.n, 255, dtype=np.uint8)
        stats = _lib.cg_pool_stats()
        rc = _lib.lib().cg_pool_sign_tx_ids(self._h, _p(sr.ids), sr.n_ids, _p(sr.reqs), sr.n, _p(sr.tmpls),
                                            len(sr.tmpls), _p(sr.arena), sr.arena.size, _p(sigs), _p(st),
                                            ctypes.byref(stats))
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        if rc != 0 and not allow_partial:
            _lib.check(rc, "cg_pool_sign_tx_ids")
        return sigs.reshape(-1, 64), st

    def load_ec_signers(self, keys):
        """cg_pool_ec_signers_load: the ECDSA signer set on every slot; returns what Engine.load_ec_signers does."""
        return _load_ec_signers(_lib.lib().cg_pool_ec_signers_load, "cg_pool_ec_signers_load", self._h, keys)

    def clear_ec_signers(self):
        _lib.check(_lib.lib().cg_pool_ec_signers_clear(self._h), "cg_pool_ec_signers_clear")

    def sign_ec_tx_ids(self, sr, nonces, allow_partial=False):
        """cg_pool_ec_sign_tx_ids: the whole call on one healthy slot, the next one on a device fault.
        Returns what Engine.sign_ec_tx_ids returns."""
        assert sr.reqs.dtype == SIGN_REQ_DTYPE and sr.tmpls.dtype == TMPL_DTYPE
        stats = _lib.cg_pool_stats()
        fn = _lib.lib().cg_pool_ec_sign_tx_ids
        out = _sign_ec(lambda k, sigs, ln, st: fn(self._h, _p(sr.ids), sr.n_ids, _p(sr.reqs), sr.n, _p(sr.tmpls),
                                                  len(sr.tmpls), _p(sr.arena), sr.arena.size, k, sigs, ln, st,
                                                  ctypes.byref(stats)),
                       "cg_pool_ec_sign_tx_ids", sr.n, nonces, allow_partial)
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        return out

    def load_rsa_signers(self, keys):
        """cg_pool_rsa_signers_load: the RSA signer set on every slot; returns what Engine.load_rsa_signers does."""
        return _load_rsa_signers(_lib.lib().cg_pool_rsa_signers_load, "cg_pool_rsa_signers_load", self._h, keys)

    def clear_rsa_signers(self):
        _lib.check(_lib.lib().cg_pool_rsa_signers_clear(self._h), "cg_pool_rsa_signers_clear")

    def sign_rsa_tx_ids(self, sr, salts, allow_partial=False):
        """cg_pool_rsa_sign_tx_ids: the whole call on one healthy slot, the next one on a device fault.
        Returns what Engine.sign_rsa_tx_ids returns."""
        assert sr.reqs.dtype == SIGN_REQ_DTYPE and sr.tmpls.dtype == TMPL_DTYPE
        stats = _lib.cg_pool_stats()
        fn = _lib.lib().cg_pool_rsa_sign_tx_ids
        out = _sign_rsa(lambda k, sigs, ln, st: fn(self._h, _p(sr.ids), sr.n_ids, _p(sr.reqs), sr.n, _p(sr.tmpls),
                                                   len(sr.tmpls), _p(sr.arena), sr.arena.size, k, sigs, ln, st,
                                                   ctypes.byref(stats)),
                        "cg_pool_rsa_sign_tx_ids", sr.n, salts, allow_partial)
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        return out

    def derive_keys(self, dr, allow_partial=False):
        """cg_pool_derive_keys: the whole call on one healthy slot, the next one on a device fault.
        Returns what Engine.derive_keys returns."""
        stats = _lib.cg_pool_stats()
        out = _derive_keys(_lib.lib().cg_pool_derive_keys, "cg_pool_derive_keys", self._h, dr, stats, allow_partial)
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        return out

    def public_keys(self, scheme, secrets):
        """cg_pool_public_keys: Engine.public_keys on one healthy slot, the next one on a device fault."""
        stats = _lib.cg_pool_stats()
        out = _public_keys(_lib.lib().cg_pool_public_keys, "cg_pool_public_keys", self._h, scheme, secrets, stats)
        self.last_stats = {k: getattr(stats, k) for k, _ in _lib.cg_pool_stats._fields_ if k != "reserved"}
        return out

    def verify_requeue(self, batch, mode=MODE_DOVERIFY, between=None):
        """The JVM binding's re-queue (CryptoBatch.kt verifyBatch): on CG_ERR_DEVICE only the items left
        NOT_RUN go to the pool once more, as a sub-batch over the same keys and arena; what still stays
        NOT_RUN is returned as NOT_RUN (the binding hands those to Crypto.doVerify one by one).
        ``between()`` runs before the re-queue (tests clear a drill fault there)."""
        st = self.verify(batch, mode, allow_partial=True)
        rc_first = self.last_stats
        todo = np.flatnonzero(st == 255)
        if todo.size:
            if between:
                between()
            sub = batch.subset(todo)
            st2 = self.verify(sub, mode, allow_partial=True)
            st[todo] = st2
        self.first_stats = rc_first
        return st
