"""The Python layer of tear-off building on the CPU: PartialMerkleTree.from_postorder, the
status-to-exception mapping, and build_filtered_batch / build_batch / build_filtered_transactions over a
stand-in engine that answers with the oracle's tables (tests/build_filtered_ref.py), so the packing and
unpacking are checked apart from the device call."""
import hashlib

import numpy as np
import pytest

import build_filtered_ref as R
from build_filtered_ref import notary_filter, wire_transaction
from corda_amd import batch as B
from corda_amd import merkle as M
from corda_amd import transactions as T
from oracle import corda as O


def _tx(n_blobs, tag):
    rng = np.random.default_rng(1000 * tag + n_blobs)
    blobs = [rng.integers(0, 256, int(rng.integers(1, 200)), dtype=np.uint8).tobytes() for _ in range(n_blobs)]
    return blobs, hashlib.sha256(b"salt %d" % tag).digest(), b"salt blob %d" % tag


def test_from_postorder_inverts_postorder():
    for n in (1, 2, 3, 5, 8, 9, 17):
        hs = [hashlib.sha256(b"%d %d" % (n, i)).digest() for i in range(n)]
        for pick in ([], [0], [n - 1], list(range(0, n, 2)), list(range(n))):
            stream = O.partial_tree_postorder(O.partial_tree_build(O.merkle_tree(hs), [hs[i] for i in pick]))
            x = M.PartialMerkleTree.from_postorder(stream)
            assert x.postorder() == stream
            assert M.PartialMerkleTree.from_postorder(x.postorder()).postorder() == x.postorder()
    for bad in ([(B.PMT_NODE, None)], [(B.PMT_LEAF, bytes(32)), (B.PMT_LEAF, bytes(32))], [(7, bytes(32))], []):
        with pytest.raises(ValueError):
            M.PartialMerkleTree.from_postorder(bad)


def test_status_to_exception():
    assert M.build_status_exception(0) is None
    e = M.build_status_exception(1)
    assert type(e) is M.MerkleTreeException and str(e) == "Cannot calculate Merkle root on empty hash list."
    e = M.build_status_exception(4)  # IllegalArgumentException, PartialMerkleTree.kt:67
    assert type(e) is ValueError and str(e) == "Zero hashes shouldn't be included in partial tree."
    e = M.build_status_exception(5)  # PartialMerkleTree.kt:74
    assert type(e) is M.MerkleTreeException and str(e) == "Some of the provided hashes are not in the tree."
    for st in (2, 3, 6):
        assert type(M.build_status_exception(st)) is ValueError
    assert type(M.build_status_exception(255)) is RuntimeError
    assert (B.BUILD_ZERO_HASH, B.BUILD_NOT_IN_TREE, B.BUILD_BAD_VISIBLE) == (4, 5, 6)


def test_build_filtered_batch_packs_and_unpacks():
    txs = [_tx(n, n) for n in (0, 1, 2, 4, 7, 11)]
    masks = [[], [1], [0, 1], [0, 0, 0, 0], [1, 0, 1, 0, 0, 1, 1], [0] * 10 + [1]]
    eng = R.OracleEngine()
    got = M.build_filtered_batch(txs, masks, eng)
    (t, c, arena, vis), = eng.calls
    assert vis.tolist() == [v for m in masks for v in m + [0]]  # the salt leaf, packed last, is hidden
    assert len(vis) == len(c) == sum(len(b) + 1 for b, _, _ in txs)
    for (blobs, salt, salt_blob), mask, f in zip(txs, masks, got):
        assert isinstance(f, M.FilteredTransaction)
        assert f.root_hash == O.tx_id(blobs, salt, salt_blob)
        assert f.component_blobs == [b for b, v in zip(blobs, mask) if v]
        assert f.nonces == [O.compute_nonce(salt, i) for i, v in enumerate(mask) if v]
        hashes = [O.component_hash(b, salt, i) for i, b in enumerate(blobs)] + [O.sha256(salt_blob)]
        want = O.partial_tree_postorder(O.partial_tree_build(O.merkle_tree(hashes),
                                                             [h for h, v in zip(hashes, mask) if v]))
        assert f.partial_merkle_tree.postorder() == want
        # what the notary would do with it
        ptree = O.partial_tree_from_postorder(f.partial_merkle_tree.postorder())
        if any(mask):
            assert O.filtered_tx_verify(f.root_hash, f.component_blobs, f.nonces, ptree)
        else:
            assert want == [(B.PMT_LEAF, f.root_hash)]
            with pytest.raises(O.MerkleTreeException):
                O.filtered_tx_verify(f.root_hash, f.component_blobs, f.nonces, ptree)
    # a mask may name the salt leaf: the status comes back as the exception
    got = M.build_filtered_batch(txs[1:3], [[1, 1], [0, 2, 0]], R.OracleEngine())
    assert [type(x) for x in got] == [ValueError, ValueError]
    with pytest.raises(ValueError):
        M.build_filtered_batch(txs[:1], [[1, 0, 0]], R.OracleEngine())
    with pytest.raises(ValueError):
        M.build_filtered_batch(txs, masks[:-1], R.OracleEngine())
    assert M.build_filtered_batch([], [], R.OracleEngine()) == []


def test_build_batch_maps_every_status():
    a, b, c, d = (hashlib.sha256(bytes([k])).digest() for k in range(4))
    leaf_lists = [[a, b, c], [a, b, c], [a, a, a], [a, b, c], [], [a, a, b], [a, b, c, d, a]]
    include = [[b], [a, a], [a], [bytes(32)], [a], [a, a], [d]]
    got = M.PartialMerkleTree.build_batch(leaf_lists, include, R.OracleEngine())
    assert [type(x) for x in got] == [tuple, M.MerkleTreeException, M.MerkleTreeException, ValueError,
                                      M.MerkleTreeException, tuple, tuple]
    assert str(got[3]) == "Zero hashes shouldn't be included in partial tree."
    assert str(got[1]) == str(got[2]) == "Some of the provided hashes are not in the tree."
    for j in (0, 5, 6):
        root, pmt = got[j]
        assert root == O.merkle_root(leaf_lists[j])
        assert pmt.postorder() == O.partial_tree_postorder(O.partial_tree_build(O.merkle_tree(leaf_lists[j]), include[j]))
        assert O.partial_tree_verify(O.partial_tree_from_postorder(pmt.postorder()), root, include[j])
    assert M.PartialMerkleTree.build_batch([], [], R.OracleEngine()) == []


def test_wire_transaction_build_filtered_transaction():
    wtx = wire_transaction()
    d = wtx.data()
    eng = R.OracleEngine()
    f = wtx.build_filtered_transaction(notary_filter, eng)
    assert eng.calls[0][3].tolist() == [1, 1, 0, 0, 0, 0, 1, 0]
    assert f.root_hash == O.tx_id(d.components, d.salt, d.salt_blob)
    assert f.component_blobs == [d.components[0], d.components[1], d.components[6]]
    assert f.nonces == [O.compute_nonce(d.salt, i) for i in (0, 1, 6)]
    assert O.filtered_tx_verify(f.root_hash, f.component_blobs, f.nonces,
                                O.partial_tree_from_postorder(f.partial_merkle_tree.postorder()))
    both = T.build_filtered_transactions([wtx, wtx], lambda c: False, R.OracleEngine())
    assert [x.partial_merkle_tree.postorder() for x in both] == [[(B.PMT_LEAF, f.root_hash)]] * 2
