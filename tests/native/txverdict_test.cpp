// Host build of corda_amd/csrc/txverdict.h (the lane logic of the per-transaction verdict kernels) for
// tests/test_txverdict.py: a shared library for ctypes, and a program with its own main that reads one
// case from a file and writes the results (the same cases again under -fsanitize=address,undefined,
// every table in a heap block of exactly its size).
//   g++ -O1 -std=c++17 -fPIC -shared -o libtxverdicttest.so txverdict_test.cpp
//   g++ -O1 -std=c++17 -o txverdict_test txverdict_test.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t g_visits;  // node loads of the requirement walk since the last reset
#define CG_TXV_VISIT() (++g_visits)
#include "../../corda_amd/csrc/txverdict.h"

namespace {

struct Tables {
  const void* sigs;
  uint32_t stride;
  cg::TxvTables tb;
  const cg_tx_check* checks;
  uint64_t n_tx;
};

// what k_tx_verdicts_wave does with its 64 lanes, one after the other
template <class Acc>
struct WaveHas {
  const Acc& acc;
  const cg::TxvTables& tb;
  const cg_tx_check& ck;
  bool operator()(uint32_t cls) const {
    bool any = false;
    for (uint32_t lane = 0; lane < 64; ++lane) any |= cg::span_has(acc, tb, ck, cls, lane, 64u);
    return any;
  }
};

template <class Acc>
void run(const Acc& acc, const Tables& T, uint32_t lanes, cg_tx_verdict* verdicts, uint8_t* req_status) {
  uint32_t frames[cg::kTxvFrameWords * CG_REQ_MAX_DEPTH];
  const cg::TxvStack st{frames, 1};
  for (uint64_t t = 0; t < T.n_tx; ++t) {
    const cg_tx_check& ck = T.checks[t];
    if (lanes == 1) {
      verdicts[t] = cg::tx_verdict_lane(acc, T.tb, ck, (uint32_t)t, st, req_status);
      continue;
    }
    const bool in_table = cg::span_in_table(T.tb, ck);
    cg::TxvSpan sp{cg::kTxvNoBad, 0};
    if (in_table)
      for (uint32_t lane = 0; lane < 64; ++lane) sp = cg::span_join(sp, cg::span_scan(acc, T.tb, ck, (uint32_t)t, lane, 64u));
    WaveHas<Acc> has{acc, T.tb, ck};
    verdicts[t] = cg::tx_requirements(T.tb, ck, in_table, sp, has, st, req_status, true);
  }
}

struct Never {
  bool operator()(uint32_t) const { return false; }
};

}  // namespace

extern "C" {

uint32_t tv_sizes(uint32_t which) {
  switch (which) {
    case 0: return sizeof(cg_tx_check);
    case 1: return sizeof(cg_req_node);
    case 2: return sizeof(cg_tx_verdict);
    case 3: return CG_REQ_MAX_DEPTH;
    case 4: return CG_REQ_MAX_VISITS;
    case 5: return cg::kTxvSmallMax;
  }
  return 0;
}

// lanes: 1 = one lane per transaction (k_tx_verdicts_small), 64 = the wave form. req_status starts as
// CG_REQ_HOST, as launch_tx_verdicts leaves it. Returns the most nodes one requirement's walk loaded.
uint64_t tv_run(const void* sigs, uint32_t stride, uint64_t n_sigs, const uint8_t* status, const cg_key* keys,
                uint32_t n_keys, const uint32_t* key_class, const cg_tx_check* checks, uint64_t n_tx,
                const uint32_t* reqs, uint32_t n_reqs, const cg_req_node* nodes, uint32_t n_nodes, uint32_t lanes,
                cg_tx_verdict* verdicts, uint8_t* req_status) {
  Tables T;
  T.sigs = sigs;
  T.stride = stride;
  T.tb = cg::TxvTables{n_sigs, status, keys, n_keys, key_class, reqs, n_reqs, nodes, n_nodes};
  T.checks = checks;
  T.n_tx = n_tx;
  if (n_reqs) memset(req_status, CG_REQ_HOST, n_reqs);
  if (stride == sizeof(cg_txsig_packed))
    run(cg::Rec12{(const cg_txsig_packed*)sigs}, T, lanes, verdicts, req_status);
  else
    run(cg::Rec24{(const cg_txsig*)sigs}, T, lanes, verdicts, req_status);
  uint64_t most = 0;
  uint32_t frames[cg::kTxvFrameWords * CG_REQ_MAX_DEPTH];
  const cg::TxvStack st{frames, 1};
  Never never;
  for (uint32_t r = 0; r < n_reqs; ++r) {
    g_visits = 0;
    (void)cg::req_walk(nodes, n_nodes, reqs[r], never, st);
    if (g_visits > most) most = g_visits;
  }
  return most;
}

}  // extern "C"

// txverdict_test <case file> <result file>
// case: uint64 stride, n_sigs, n_keys, has_class, n_tx, n_reqs, n_nodes, lanes; then the signature table,
// status, keys, key_class (if has_class), checks, reqs, nodes. result: verdicts, req_status, uint64 most visits.
int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t h[8];
  if (fread(h, sizeof h, 1, f) != 1) return 2;
  const uint64_t sizes[7] = {h[0] * h[1], h[1], sizeof(cg_key) * h[2], h[3] ? 4 * h[2] : 0, sizeof(cg_tx_check) * h[4],
                             4 * h[5], sizeof(cg_req_node) * h[6]};
  void* buf[7];
  for (int k = 0; k < 7; ++k) {  // exactly its size, so that a read past a table's end is caught
    buf[k] = sizes[k] ? malloc(sizes[k]) : nullptr;
    if (sizes[k] && (!buf[k] || fread(buf[k], sizes[k], 1, f) != 1)) return 2;
  }
  fclose(f);
  cg_tx_verdict* verdicts = h[4] ? (cg_tx_verdict*)malloc(sizeof(cg_tx_verdict) * h[4]) : nullptr;
  uint8_t* req_status = h[5] ? (uint8_t*)malloc(h[5]) : nullptr;
  const uint64_t most =
      tv_run(buf[0], (uint32_t)h[0], h[1], (const uint8_t*)buf[1], (const cg_key*)buf[2], (uint32_t)h[2],
             h[3] ? (const uint32_t*)buf[3] : nullptr, (const cg_tx_check*)buf[4], h[4], (const uint32_t*)buf[5],
             (uint32_t)h[5], (const cg_req_node*)buf[6], (uint32_t)h[6], (uint32_t)h[7], verdicts, req_status);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  if (h[4]) fwrite(verdicts, sizeof(cg_tx_verdict), h[4], o);
  if (h[5]) fwrite(req_status, 1, h[5], o);
  fwrite(&most, sizeof most, 1, o);
  fclose(o);
  for (void* p : buf) free(p);
  free(verdicts);
  free(req_status);
  printf("ok: %llu transactions, %llu requirements, most visits %llu\n", (unsigned long long)h[4],
         (unsigned long long)h[5], (unsigned long long)most);
  return 0;
}
