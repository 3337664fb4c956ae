// Host build of the Ed25519 signer's lane code (corda_amd/csrc: sc_muladd, the 32- and 64-byte-prefix
// SHA-512 forms, ed_fixed_base9, ed_encode, ed_signer_expand) with FE_BOUNDS_CHECK on: the arithmetic
// k_ed_signer_expand / k_ed_sign_* run, checked on the CPU. Built once per -DED_WIDE_BW=26/24/22
// (tests/hostsign.py). With -DSIGN_MAIN it is a stand-alone program over a text file of cases, which
// the tests build with the sanitizers. Test infrastructure only.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <string>
#include <vector>

#include "../../corda_amd/csrc/ed25519_rows.h"

static Ed25519Consts g_C;
static EdBWideTab* g_TB = nullptr;
static std::vector<bool> g_built;
static ge_p3 g_base[EdWideCfg::kBDigits];  // 2^{ED_WIDE_BW u} B

// The constant table is tens of GB at radix 2^26: mapped without backing store, and only the groups of
// 8 multiples a scalar's digits touch are built, with the device lane's code (ed_bwide_group).
static void tb_init() {
  if (g_TB) return;
  ed_consts_init(g_C);
  void* m = mmap(nullptr, sizeof(EdBWideTab), PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (m == MAP_FAILED) abort();
  g_TB = (EdBWideTab*)m;
  ge9_niels_identity_half(g_TB->ident);
  g_built.assign((size_t)EdWideCfg::kBDigits * (EdWideCfg::kBMult / 8), false);
  ge_p3 B;
  fe x, y, two_inv, t;
  fe_sub(x, g_C.Btab[1].ypx, g_C.Btab[1].ymx);
  fe_add(y, g_C.Btab[1].ypx, g_C.Btab[1].ymx);
  fe_0(t);
  t.v[0] = 2;
  fe_invert(two_inv, t);
  fe_mul(B.X, x, two_inv);
  fe_mul(B.Y, y, two_inv);
  fe_1(B.Z);
  fe_mul(B.T, B.X, B.Y);
  ge_p3 P = B;
  for (int u = 0; u < EdWideCfg::kBDigits; ++u) {
    if (u > 0) ed_dbl_n(P, P, ED_WIDE_BW);
    g_base[u] = P;
  }
}
static void tb_touch(const uint32_t* es) {
  for (int u = 0; u < EdWideCfg::kBDigits; ++u) {
    const int d = sc_digit_at<EdWideCfg::kBBits>(es, u), a = d < 0 ? -d : d;
    if (a == 0) continue;
    const int grp = (a - 1) / 8;
    const size_t k = (size_t)u * (EdWideCfg::kBMult / 8) + grp;
    if (g_built[k]) continue;
    ed_bwide_group(&g_TB->t[u][8 * grp], g_base[u], 0, grp, g_C.d2);
    g_built[k] = true;
  }
}

// s B encoded, s < 2^253; digits_out (optional): the kBDigits signed digits the rows were read by
static void fixed_base_enc(uint32_t enc[8], const uint32_t s[8], int32_t* digits_out) {
  tb_init();
  uint32_t es[EdWideCfg::kBPackedWords];
  sc_recode_wb<ED_WIDE_BW, EdWideCfg::kBBits>(es, EdWideCfg::kBPackedWords, s);
  if (digits_out)
    for (int u = 0; u < EdWideCfg::kBDigits; ++u) digits_out[u] = sc_digit_at<EdWideCfg::kBBits>(es, u);
  tb_touch(es);
  ge_p2 q;
  ed_fixed_base9(q, es, *g_TB);
  fe zi;
  fe_invert(zi, q.Z);
  ed_encode(enc, q, zi);
}

static void signer_expand(EdSigner& sg, const uint32_t seed[8]) {
  tb_init();
  uint32_t es[EdWideCfg::kBPackedWords];
  EdSigner tmp;
  ed_signer_scalars(tmp, es, seed);
  tb_touch(es);
  ed_signer_expand(sg, seed, *g_TB);
}

// An arena copy of msg at byte phase `phase` (0..3) of a 4-aligned buffer, readable to its rounded end
struct Arena {
  std::vector<uint32_t> buf;
  uint64_t off, len_rounded;
  Arena(const uint8_t* msg, uint64_t len, uint32_t phase) : buf((len + phase + 3) / 4 + 1, 0xa5a5a5a5u), off(phase) {
    if (len) memcpy((uint8_t*)buf.data() + phase, msg, len);
    len_rounded = (phase + len + 3) & ~(uint64_t)3;
  }
  ArenaLd ld() const { return ArenaLd{(const uint8_t*)buf.data(), len_rounded}; }
};
// A template image prefix || 0^32 || suffix, zero-padded to the 16-aligned slot, and the id's dwords
struct Splice {
  std::vector<uint32_t> img, id;
  uint32_t at, len;
  Splice(const uint8_t* pre, uint32_t plen, const uint8_t* idb, const uint8_t* suf, uint32_t slen)
      : id(8), at(plen), len(plen + 32 + slen) {
    const uint64_t slot = ((uint64_t)len + 15) & ~(uint64_t)15;
    img.assign(slot / 4, 0u);
    if (plen) memcpy((uint8_t*)img.data(), pre, plen);
    if (slen) memcpy((uint8_t*)img.data() + plen + 32, suf, slen);
    memcpy(id.data(), idb, 32);
  }
  SpliceLd ld() const { return SpliceLd{(const uint8_t*)img.data(), (uint64_t)img.size() * 4, id.data(), at}; }
};

// The per-item lane path of k_ed_sign_nonce / _rb / _encode / _s over message source `hash`:
// hash(pw, out16, prefix) = SHA-512(prefix (pw words) || M)
template <class Hash>
static void sign_lane(uint32_t sig[16], const EdSigner& sg, Hash hash) {
  uint32_t hw[16], r[8], k[8], pre[16], S[8], R[8];
  hash(8, hw, sg.prefix);
  sc_reduce512(r, hw);
  fixed_base_enc(R, r, nullptr);
  for (int w = 0; w < 8; ++w) {
    pre[w] = R[w];
    pre[8 + w] = sg.abyte[w];
  }
  hash(16, hw, pre);
  sc_reduce512(k, hw);
  sc_muladd(S, k, sg.a, r);
  for (int w = 0; w < 8; ++w) {
    sig[w] = R[w];
    sig[8 + w] = S[w];
  }
}

extern "C" {
int t_wide_bw() { return ED_WIDE_BW; }
int t_b_digits() { return EdWideCfg::kBDigits; }

void t_sc_muladd(const uint32_t* k, const uint32_t* a, const uint32_t* r, uint32_t* out) { sc_muladd(out, k, a, r); }

void t_fixed_base(const uint32_t* s, uint32_t* enc, int32_t* digits_out) { fixed_base_enc(enc, s, digits_out); }

// SHA-512(prefix (pw = 8 / 16 words) || msg), the arena form, msg at byte phase `phase`
void t_sha512_prefix_arena(int pw, const uint32_t* prefix, const uint8_t* msg, uint64_t len, uint32_t phase,
                           uint32_t* out) {
  const Arena a(msg, len, phase);
  if (pw == 8) sha512_prefix_ld<8>(out, prefix, a.ld(), a.off, len);
  else sha512_prefix64_ld(out, prefix, a.ld(), a.off, len);
}
// the splice form over prefix || id || suffix
void t_sha512_prefix_splice(int pw, const uint32_t* prefix, const uint8_t* pre, uint32_t plen, const uint8_t* id,
                            const uint8_t* suf, uint32_t slen, uint32_t* out) {
  const Splice sp(pre, plen, id, suf, slen);
  if (pw == 8) sha512_prefix_splice<8>(out, prefix, sp.ld(), sp.len, nullptr);
  else sha512_prefix64_splice(out, prefix, sp.ld(), sp.len, nullptr);
}

// out: a, prefix, abyte (24 words)
void t_signer_expand(const uint32_t* seed, uint32_t* out) {
  EdSigner sg;
  signer_expand(sg, seed);
  memcpy(out, &sg, sizeof sg);
}

void t_sign_arena(const uint32_t* seed, const uint8_t* msg, uint64_t len, uint32_t phase, uint32_t* sig) {
  EdSigner sg;
  signer_expand(sg, seed);
  const Arena a(msg, len, phase);
  sign_lane(sig, sg, [&](int pw, uint32_t* out, const uint32_t* prefix) {
    if (pw == 8) sha512_prefix_ld<8>(out, prefix, a.ld(), a.off, len);
    else sha512_prefix64_ld(out, prefix, a.ld(), a.off, len);
  });
}
void t_sign_splice(const uint32_t* seed, const uint8_t* pre, uint32_t plen, const uint8_t* id, const uint8_t* suf,
                   uint32_t slen, uint32_t* sig) {
  EdSigner sg;
  signer_expand(sg, seed);
  const Splice sp(pre, plen, id, suf, slen);
  sign_lane(sig, sg, [&](int pw, uint32_t* out, const uint32_t* prefix) {
    if (pw == 8) sha512_prefix_splice<8>(out, prefix, sp.ld(), sp.len, nullptr);
    else sha512_prefix64_splice(out, prefix, sp.ld(), sp.len, nullptr);
  });
}
}

#ifdef SIGN_MAIN
// Cases, one per line, fields in hex ("-" = empty):
//   M seed pub msg sig            the arena form (at all four byte phases)
//   T seed pub prefix id suffix sig   the splice form
//   B scalar enc                  ed_fixed_base9 + ed_encode of a crafted scalar
// Exit status 0 when every case matches, 1 on a mismatch, 2 on a bad file.
static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> b;
  if (h == "-") return b;
  for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return b;
}
static std::vector<std::string> split(const std::string& l) {
  std::vector<std::string> f;
  size_t i = 0;
  while (i < l.size()) {
    while (i < l.size() && (l[i] == ' ' || l[i] == '\n' || l[i] == '\r')) ++i;
    size_t j = i;
    while (j < l.size() && l[j] != ' ' && l[j] != '\n' && l[j] != '\r') ++j;
    if (j > i) f.push_back(l.substr(i, j - i));
    i = j;
  }
  return f;
}
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fp = fopen(argv[1], "r");
  if (!fp) return 2;
  std::string line;
  int c, bad = 0, n = 0;
  std::vector<std::string> lines;
  while ((c = fgetc(fp)) != EOF) {
    if (c == '\n') {
      lines.push_back(line);
      line.clear();
    } else {
      line.push_back((char)c);
    }
  }
  if (!line.empty()) lines.push_back(line);
  fclose(fp);
  for (const std::string& l : lines) {
    const std::vector<std::string> f = split(l);
    if (f.empty()) continue;
    ++n;
    uint32_t w[8], sig[16];
    if (f[0] == "B" && f.size() == 3) {
      const std::vector<uint8_t> s = unhex(f[1]), e = unhex(f[2]);
      if (s.size() != 32 || e.size() != 32) return 2;
      memcpy(w, s.data(), 32);
      uint32_t enc[8];
      fixed_base_enc(enc, w, nullptr);
      if (memcmp(enc, e.data(), 32)) ++bad;
    } else if (f[0] == "M" && f.size() == 5) {
      const std::vector<uint8_t> seed = unhex(f[1]), pub = unhex(f[2]), msg = unhex(f[3]), want = unhex(f[4]);
      if (seed.size() != 32 || pub.size() != 32 || want.size() != 64 || msg.empty()) return 2;
      memcpy(w, seed.data(), 32);
      uint32_t ex[24];
      t_signer_expand(w, ex);
      if (memcmp(ex + 16, pub.data(), 32)) ++bad;
      for (uint32_t phase = 0; phase < 4; ++phase) {
        t_sign_arena(w, msg.data(), msg.size(), phase, sig);
        if (memcmp(sig, want.data(), 64)) ++bad;
      }
    } else if (f[0] == "T" && f.size() == 7) {
      const std::vector<uint8_t> seed = unhex(f[1]), pub = unhex(f[2]), pre = unhex(f[3]), id = unhex(f[4]),
                                 suf = unhex(f[5]), want = unhex(f[6]);
      if (seed.size() != 32 || id.size() != 32 || want.size() != 64) return 2;
      memcpy(w, seed.data(), 32);
      t_sign_splice(w, pre.data(), (uint32_t)pre.size(), id.data(), suf.data(), (uint32_t)suf.size(), sig);
      if (memcmp(sig, want.data(), 64)) ++bad;
      (void)pub;
    } else {
      return 2;
    }
  }
  printf("%d cases, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}
#endif
