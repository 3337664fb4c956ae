// Per-transaction verdicts (include/cordagpu.h, cg_tx_verdicts): the lane logic of txverdict.hip, free
// of HIP so that the CPU compiles exactly what the GPU runs (tests/native/txverdict_test.cpp,
// tests/test_txverdict.py). Two parts per transaction:
//   - the span scan: the first signature whose status is not CG_VALID, whether every record of the span
//     carries the transaction's index, whether a signer's key is a CompositeKey (span_scan), and whether
//     a signer has a given key class (span_has). Both take (lane, stride), so one lane walks a short
//     span alone and a wave strides a long one; partial results combine with span_join;
//   - the requirement walk (req_walk): PublicKey.isFulfilledBy over the flattened CompositeKey nodes,
//     an explicit stack of CG_REQ_MAX_DEPTH frames and a budget of CG_REQ_MAX_VISITS node visits, so
//     that every loop ends for any table contents. Every index is checked before its load.
// tx_requirements puts them together; its `Has` argument answers "does a signer have class c" (one
// lane: a loop over the span; a wave: a strided loop and a wave-wide any).
#pragma once
#include <stdint.h>

#include "../../include/cordagpu.h"

#if defined(__HIPCC__)
#define CG_TXV_HD __host__ __device__ __forceinline__
#else
#define CG_TXV_HD inline
#endif
// a node load of the requirement walk (the CPU test counts them)
#ifndef CG_TXV_VISIT
#define CG_TXV_VISIT() ((void)0)
#endif

namespace cg {

constexpr uint32_t kTxvSmallMax = 32;      // spans up to this long take one lane, longer ones a wave
constexpr uint64_t kTxvNoBad = ~0ull;      // span key: no signature with a status other than CG_VALID
constexpr uint32_t kTxvFrameWords = 3;     // a walk frame: node index, next child, weight sum

// The two record layouts of the signature table.
struct Rec12 {
  const cg_txsig_packed* p;
  CG_TXV_HD uint32_t tx_idx(uint64_t i) const { return p[i].tx_idx; }
  CG_TXV_HD uint32_t key_idx(uint64_t i) const { return p[i].key_idx; }
};
struct Rec24 {
  const cg_txsig* p;
  CG_TXV_HD uint32_t tx_idx(uint64_t i) const { return p[i].tx_idx; }
  CG_TXV_HD uint32_t key_idx(uint64_t i) const { return p[i].key_idx; }
};

struct TxvTables {
  uint64_t n_sigs;
  const uint8_t* status;
  const cg_key* keys;
  uint32_t n_keys;
  const uint32_t* key_class;  // null: the identity
  const uint32_t* reqs;
  uint32_t n_reqs;
  const cg_req_node* nodes;
  uint32_t n_nodes;
};

// What a scan of (part of) a span found. first: (ordinal << 8 | status) of the first signature that
// is not CG_VALID, or kTxvNoBad; flags: CG_TXV_SPAN_BAD / CG_TXV_COMPOSITE_SIGNER.
struct TxvSpan {
  uint64_t first;
  uint32_t flags;
};

CG_TXV_HD TxvSpan span_join(TxvSpan a, TxvSpan b) {
  TxvSpan r;
  r.first = a.first < b.first ? a.first : b.first;
  r.flags = a.flags | b.flags;
  return r;
}

CG_TXV_HD bool span_in_table(const TxvTables& tb, const cg_tx_check& ck) {
  return ck.reserved == 0 && ck.first_sig <= tb.n_sigs && ck.n_sigs <= tb.n_sigs - ck.first_sig;
}

// Ordinals lane, lane + stride, ... of transaction t's span (which lies inside the table: span_in_table).
template <class Acc>
CG_TXV_HD TxvSpan span_scan(const Acc& acc, const TxvTables& tb, const cg_tx_check& ck, uint32_t t, uint32_t lane,
                            uint32_t stride) {
  TxvSpan r;
  r.first = kTxvNoBad;
  r.flags = 0;
  for (uint32_t i = lane; i < ck.n_sigs; i += stride) {
    const uint64_t j = ck.first_sig + i;
    if (acc.tx_idx(j) != t) r.flags |= CG_TXV_SPAN_BAD;
    const uint8_t st = tb.status[j];
    if (st != CG_VALID) {
      const uint64_t key = ((uint64_t)i << 8) | st;
      if (key < r.first) r.first = key;
    }
    const uint32_t k = acc.key_idx(j);
    if (k < tb.n_keys && tb.keys[k].scheme == CG_COMPOSITE_KEY) r.flags |= CG_TXV_COMPOSITE_SIGNER;
    if (stride > ck.n_sigs - i) break;  // i + stride would pass the span (and could wrap)
  }
  return r;
}

// Does one of the ordinals lane, lane + stride, ... sign with a key of class `cls`?
template <class Acc>
CG_TXV_HD bool span_has(const Acc& acc, const TxvTables& tb, const cg_tx_check& ck, uint32_t cls, uint32_t lane,
                        uint32_t stride) {
  for (uint32_t i = lane; i < ck.n_sigs; i += stride) {
    const uint32_t k = acc.key_idx(ck.first_sig + i);
    if (k < tb.n_keys && (tb.key_class ? tb.key_class[k] : k) == cls) return true;
    if (stride > ck.n_sigs - i) break;
  }
  return false;
}

// The walk's frames: word w of frame d at base[(d * kTxvFrameWords + w) * stride] (the kernels keep
// them in LDS, one column per lane; the CPU in a plain array, stride 1).
struct TxvStack {
  uint32_t* base;
  uint32_t stride;
  CG_TXV_HD uint32_t& at(uint32_t d, uint32_t w) const { return base[(d * kTxvFrameWords + w) * stride]; }
};

CG_TXV_HD bool node_children_ok(const cg_req_node& nd, uint32_t idx, uint32_t n_nodes) {
  return nd.a > idx && (uint64_t)nd.a + nd.n_children <= n_nodes;
}

// PublicKey.isFulfilledBy for the requirement rooted at node `root`: CG_REQ_*. has(cls): a signer of
// the span has key class cls. Loop bound: every iteration either visits a node (at most
// CG_REQ_MAX_VISITS of them) or pops a frame (at most one pop per composite visited).
template <class Has>
CG_TXV_HD uint8_t req_walk(const cg_req_node* nodes, uint32_t n_nodes, uint32_t root, Has& has, const TxvStack& st) {
  if (root >= n_nodes) return CG_REQ_BAD;
  CG_TXV_VISIT();
  const cg_req_node rn = nodes[root];
  if (rn.n_children == 0) return has(rn.a) ? CG_REQ_FULFILLED : CG_REQ_MISSING;
  if (!node_children_ok(rn, root, n_nodes)) return CG_REQ_BAD;
  uint32_t visits = 1, depth = 0;
  // the frame on top, in registers: the composite `node`, its next child and its weight sum so far
  uint32_t node = root, a = rn.a, nch = rn.n_children, next = 0, sum = 0;
  int32_t thr = rn.threshold, weight = rn.weight;
  for (;;) {
    if (next == nch) {  // every child seen: this composite's verdict goes into its parent's sum
      const bool ok = (int32_t)sum >= thr;
      if (depth == 0) return ok ? CG_REQ_FULFILLED : CG_REQ_MISSING;
      --depth;
      const int32_t w = weight;
      node = st.at(depth, 0);
      next = st.at(depth, 1);
      sum = st.at(depth, 2) + (ok ? (uint32_t)w : 0u);  // List<Int>.sum() wraps
      const cg_req_node pn = nodes[node];  // node < n_nodes was checked when the frame was made
      if (!node_children_ok(pn, node, n_nodes)) return CG_REQ_BAD;
      a = pn.a;
      nch = pn.n_children;
      thr = pn.threshold;
      weight = pn.weight;
      if (next > nch) return CG_REQ_BAD;
      continue;
    }
    if (visits >= CG_REQ_MAX_VISITS) return CG_REQ_HOST;
    ++visits;
    const uint32_t child = a + next;  // < n_nodes: node_children_ok(a + nch <= n_nodes), next < nch
    ++next;
    CG_TXV_VISIT();
    const cg_req_node cn = nodes[child];
    if (cn.n_children == 0) {
      if (has(cn.a)) sum += (uint32_t)cn.weight;
      continue;
    }
    if (!node_children_ok(cn, child, n_nodes)) return CG_REQ_BAD;
    if (depth + 1 >= CG_REQ_MAX_DEPTH) return CG_REQ_HOST;  // the frame in registers is one of the CG_REQ_MAX_DEPTH
    st.at(depth, 0) = node;
    st.at(depth, 1) = next;
    st.at(depth, 2) = sum;
    ++depth;
    node = child;
    a = cn.a;
    nch = cn.n_children;
    thr = cn.threshold;
    weight = cn.weight;
    next = 0;
    sum = 0;
  }
}

// The verdict of a transaction whose span scan gave `sp` (in_table: span_in_table), and its
// requirements' status bytes (written when `write`: one lane of a wave).
template <class Has>
CG_TXV_HD cg_tx_verdict tx_requirements(const TxvTables& tb, const cg_tx_check& ck, bool in_table, TxvSpan sp, Has& has,
                                        const TxvStack& st, uint8_t* req_status, bool write) {
  cg_tx_verdict v;
  const bool span_bad = !in_table || (sp.flags & CG_TXV_SPAN_BAD);
  uint32_t flags = span_bad ? CG_TXV_SPAN_BAD : (sp.flags & CG_TXV_COMPOSITE_SIGNER);
  if (span_bad) {
    v.first_bad = 0xFFFFFFFFu;
    v.status = CG_NOT_RUN;
  } else if (sp.first == kTxvNoBad) {
    v.first_bad = 0xFFFFFFFFu;
    v.status = CG_VALID;
  } else {
    v.first_bad = (uint32_t)(sp.first >> 8);
    v.status = (uint8_t)(sp.first & 0xFF);
  }
  uint32_t missing = 0;
  const bool reqs_ok = ck.first_req <= tb.n_reqs && ck.n_req <= tb.n_reqs - ck.first_req;
  if (!reqs_ok) {
    flags |= CG_TXV_REQ_HOST;
  } else {
    for (uint32_t r = 0; r < ck.n_req; ++r) {
      uint8_t rs = CG_REQ_HOST;
      if (!span_bad) {
        const uint32_t root = tb.reqs[ck.first_req + r];
        rs = req_walk(tb.nodes, tb.n_nodes, root, has, st);
        // a CompositeKey among the signers fulfils no composite requirement (CompositeKey.kt:186-189)
        if (rs == CG_REQ_FULFILLED && (sp.flags & CG_TXV_COMPOSITE_SIGNER) && tb.nodes[root].n_children != 0)
          rs = CG_REQ_MISSING;
      }
      if (rs == CG_REQ_MISSING) ++missing;
      if (rs == CG_REQ_HOST || rs == CG_REQ_BAD) flags |= CG_TXV_REQ_HOST;
      if (write) req_status[ck.first_req + r] = rs;
    }
  }
  v.flags = (uint8_t)flags;
  v.n_missing = (uint16_t)(missing > 0xFFFFu ? 0xFFFFu : missing);
  return v;
}

// One lane, the whole transaction.
template <class Acc>
struct TxvLaneHas {
  const Acc& acc;
  const TxvTables& tb;
  const cg_tx_check& ck;
  CG_TXV_HD bool operator()(uint32_t cls) const { return span_has(acc, tb, ck, cls, 0, 1); }
};

template <class Acc>
CG_TXV_HD cg_tx_verdict tx_verdict_lane(const Acc& acc, const TxvTables& tb, const cg_tx_check& ck, uint32_t t,
                                        const TxvStack& st, uint8_t* req_status) {
  const bool in_table = span_in_table(tb, ck);
  TxvSpan sp;
  sp.first = kTxvNoBad;
  sp.flags = 0;
  if (in_table) sp = span_scan(acc, tb, ck, t, 0, 1);
  TxvLaneHas<Acc> has{acc, tb, ck};
  return tx_requirements(tb, ck, in_table, sp, has, st, req_status, true);
}

}  // namespace cg
