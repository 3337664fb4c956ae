// Host build of corda_amd/csrc/pmt_build.h: the walk and the by-value inclusion rule that
// build_filtered.hip's lanes run, over cases read from a file (tests/test_pmt_build.py writes them and
// compares the output with oracle/corda.py). A stand-alone program, so that the same cases also run under
// -fsanitize=address,undefined; every case's buffers are heap blocks of exactly their size.
//
// Input:  u32 n_cases, then per case: u32 n, u32 m, n x 32 leaf-hash bytes, then
//           m == 0xffffffff: n mask bytes (inclusion by index, cg_build_filtered's rule)
//           otherwise:       m x 32 include-hash bytes (inclusion by value, cg_build_partial_trees' rule)
// Output: one line per case: "0 <kind>[:<hash hex>] ... root:<hex> counts:<rows>,<hashes>,<hashConcats>"
//         (a status other than 0: the status alone); " MISMATCH" behind it if the count pass disagrees with
//         the stream or the walk did not hash exactly P - 1 nodes.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../corda_amd/csrc/pmt_build.h"
#include "../../corda_amd/csrc/sha2.h"

namespace {

struct Count {
  static constexpr bool kHash = false;
  const uint8_t* vis;
  uint64_t n_nodes = 0, n_hashes = 0;
  bool visible(uint64_t i) const { return vis[i] != 0; }
  void leaf(uint64_t, uint32_t*) const {}
  void concat(uint32_t*, const uint32_t*, const uint32_t*) const {}
  void emit(uint32_t kind, const uint32_t*) {
    ++n_nodes;
    n_hashes += kind != CG_PMT_NODE;
  }
};

struct Emit {
  static constexpr bool kHash = true;
  const uint8_t* vis;
  const uint8_t* leaves;
  FILE* f;
  uint64_t n_nodes = 0, n_hashes = 0, concats = 0;
  bool visible(uint64_t i) const { return vis[i] != 0; }
  void leaf(uint64_t i, uint32_t h[8]) const {
    for (int k = 0; k < 8; ++k) {
      uint32_t w;
      memcpy(&w, leaves + 32 * i + 4 * k, 4);
      h[k] = __builtin_bswap32(w);
    }
  }
  void concat(uint32_t o[8], const uint32_t l[8], const uint32_t r[8]) {
    uint32_t s[8], w[16];
    sha256_init(s);
    for (int k = 0; k < 8; ++k) {
      w[k] = l[k];
      w[8 + k] = r[k];
    }
    sha256_compress(s, w);
    w[0] = 0x80000000u;
    for (int k = 1; k < 15; ++k) w[k] = 0;
    w[15] = 512;
    sha256_compress(s, w);
    for (int k = 0; k < 8; ++k) o[k] = s[k];
    ++concats;
  }
  void emit(uint32_t kind, const uint32_t* h) {
    ++n_nodes;
    fprintf(f, " %u", kind);
    if (kind == CG_PMT_NODE) return;
    ++n_hashes;
    fputc(':', f);
    for (int k = 0; k < 8; ++k) fprintf(f, "%08x", h[k]);
  }
};

struct BytesAt {
  const uint8_t* p;
  void operator()(uint64_t i, uint32_t h[8]) const { memcpy(h, p + 32 * i, 32); }
};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 2;
  uint32_t n_cases = 0;
  if (!rd(in, &n_cases, 4)) return 3;
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint32_t n = 0, m = 0;
    if (!rd(in, &n, 4) || !rd(in, &m, 4)) return 3;
    std::unique_ptr<uint8_t[]> leaves(new uint8_t[32 * (size_t)n]), vis(new uint8_t[n]);
    if (!rd(in, leaves.get(), 32 * (size_t)n)) return 3;
    uint32_t st = 0;
    if (m == 0xffffffffu) {
      if (!rd(in, vis.get(), n)) return 3;
      if (n == 0) st = 1;
    } else {
      std::unique_ptr<uint8_t[]> inc(new uint8_t[32 * (size_t)m]);
      if (!rd(in, inc.get(), 32 * (size_t)m)) return 3;
      st = cg::pmt_mark(n, m, BytesAt{leaves.get()}, BytesAt{inc.get()}, vis.get());
    }
    if (st != 0) {
      fprintf(out, "%u\n", st);
      continue;
    }
    uint32_t root[8];
    Count cnt;
    cnt.vis = vis.get();
    cg::pmt_walk(n, cnt, root);
    Emit em;  // prints the stream as it goes
    em.vis = vis.get();
    em.leaves = leaves.get();
    em.f = out;
    fprintf(out, "0");
    cg::pmt_walk(n, em, root);
    fprintf(out, " root:");
    for (int k = 0; k < 8; ++k) fprintf(out, "%08x", root[k]);
    uint64_t P = 1;
    while (P < n) P <<= 1;
    const bool same = cnt.n_nodes == em.n_nodes && cnt.n_hashes == em.n_hashes && em.concats == P - 1;
    fprintf(out, " counts:%llu,%llu,%llu%s\n", (unsigned long long)cnt.n_nodes, (unsigned long long)cnt.n_hashes,
            (unsigned long long)em.concats, same ? "" : " MISMATCH");
  }
  fclose(in);
  if (fclose(out) != 0) return 4;
  printf("ok: %u cases\n", n_cases);
  return 0;
}
