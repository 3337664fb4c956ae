// Host build of the ECDSA signer's lane code (corda_amd/csrc/sign_ec.h: the range checks, e, k G over the
// constant G table through ec_slot_fixed_base, r = x mod n, s = k^-1 (e + r d), the DER encoder; and the
// SHA-256 loaders in their arena and splice-from-midstate forms) with FE_BOUNDS_CHECK on: the arithmetic
// the kernels of sign_ec.hip run, checked on the CPU. Built once per radix (-DED_WIDE_BW=-DEC_WIDE_GW=
// 26 / 24 / 22, tests/hostsignec.py). With -DSIGN_EC_MAIN it is a stand-alone program over a text file of
// cases, which the tests build with the sanitizers. Test infrastructure only.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <string>
#include <vector>

#include "../../corda_amd/csrc/sign_ec.h"

static_assert(ED_WIDE_BW == EC_WIDE_GW, "one fixed-base radix per build");

// The constant G table, mapped without backing store; only the groups a scalar's digits touch are built,
// with the device lanes' code (ec_gwide_group_from)
template <int C>
struct GTab {
  EcConsts K;
  EcGWideTab* T = nullptr;
  std::vector<bool> built;
  Jac base[EC_WIDE_GDIGITS];  // 2^{EC_WIDE_GW u} G
  EcRowScratch* S = nullptr;
  void init() {
    if (T) return;
    ec_consts_init<C>(K);
    void* m = mmap(nullptr, sizeof(EcGWideTab), PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED) abort();
    T = (EcGWideTab*)m;
    S = new EcRowScratch;
    built.assign((size_t)EC_WIDE_GDIGITS * (EC_WIDE_GMULT / EC_MULT), false);
    Jac P = {K.gx, K.gy, K.one_p};
    for (int u = 0; u < EC_WIDE_GDIGITS; ++u) {
      if (u > 0) jac_dbl_n<C>(P, P, EC_WIDE_GW);
      base[u] = P;
    }
  }
  void touch(const u256w& d, int32_t* digits_out) {
    init();
    constexpr int GG = EC_WIDE_GMULT / EC_MULT;
    uint32_t dg[EC_WIDE_GPACKED];
    ec_recode_wide<EC_WIDE_GW, EC_WIDE_GDIGITS, false, EC_WIDE_GBITS>(dg, d);
    for (int u = 0; u < EC_WIDE_GDIGITS; ++u) {
      const int e = ec_digit_at<EC_WIDE_GBITS>(dg, u), a = e < 0 ? -e : e;
      if (digits_out) digits_out[u] = e;
      if (a == 0 || built[(size_t)u * GG + (a - 1) / EC_MULT]) continue;
      const int g = (a - 1) / EC_MULT;
      ec_gwide_group_from<C>(&T->t[u][g * EC_MULT], base[u], g, *S, K);
      built[(size_t)u * GG + g] = true;
    }
  }
};
static GTab<CG_CURVE_K1> g_k1;
static GTab<CG_CURVE_R1> g_r1;

// An arena copy of `data` at byte phase `phase` of a 4-aligned buffer, readable to its rounded end only
struct Arena {
  std::vector<uint32_t> buf;
  uint64_t off, len_rounded;
  Arena(const uint8_t* data, uint64_t len, uint32_t phase) : buf((len + phase + 3) / 4 + 1, 0xa5a5a5a5u), off(phase) {
    if (len) memcpy((uint8_t*)buf.data() + phase, data, len);
    len_rounded = (phase + len + 3) & ~(uint64_t)3;
    buf.resize(len_rounded / 4 ? len_rounded / 4 : 1);  // a load past the rounded end is out of bounds
  }
  ArenaLd ld() const { return ArenaLd{(const uint8_t*)buf.data(), len_rounded}; }
};
// A template image prefix || 0^32 || suffix, zero-padded to the 16-aligned slot, the id's dwords, and the
// SHA-256 state after the prefix's full blocks (what k_tmpl_prep leaves in TmplMid)
struct Splice {
  std::vector<uint32_t> img, id;
  uint32_t at, len, mid[8], blocks;
  Splice(const uint8_t* pre, uint32_t plen, const uint8_t* idb, const uint8_t* suf, uint32_t slen)
      : id(8), at(plen), len(plen + 32 + slen) {
    const uint64_t slot = ((uint64_t)len + 15) & ~(uint64_t)15;
    img.assign(slot / 4, 0u);
    if (plen) memcpy((uint8_t*)img.data(), pre, plen);
    if (slen) memcpy((uint8_t*)img.data() + plen + 32, suf, slen);
    memcpy(id.data(), idb, 32);
    sha256_init(mid);
    blocks = plen / 64;
    for (uint32_t b = 0; b < blocks; ++b) {
      uint32_t w[16];
      for (int j = 0; j < 16; ++j) w[j] = CG_BSWAP32(img[16 * b + j]);
      sha256_compress(mid, w);
    }
  }
  SpliceLd ld() const { return SpliceLd{(const uint8_t*)img.data(), (uint64_t)img.size() * 4, id.data(), at}; }
};

static void from_be(u256w& v, const uint8_t* be) {
  uint32_t w[8];
  memcpy(w, be, 32);
  ec_secret_from_be(v, w);
}
static void to_be(uint8_t* be, const u256w& v) {
  for (int k = 0; k < 8; ++k) {
    const uint32_t w = CG_BSWAP32(v.w[7 - k]);
    memcpy(be + 4 * k, &w, 4);
  }
}

// The lane of one item from the digest on: the checks of k_ec_signer_expand and k_ec_sign_prep, then
// k_ec_sign_mul and one item of k_ec_sign_finish
template <int C>
static uint8_t sign_lane(GTab<C>& G, const u256w& d, const uint32_t h[8], const u256w& k, uint32_t out[CG_EC_SIG_WORDS],
                         uint32_t& len, int32_t* digits_out) {
  G.init();
  for (int i = 0; i < CG_EC_SIG_WORDS; ++i) out[i] = 0;
  len = 0;
  if (!ec_scalar_in_range<C>(d)) return CG_NOT_RUN;  // refused at load
  EcSigner sg;
  ec_signer_init<C>(sg, d, G.K);
  if (!ec_scalar_in_range<C>(k)) return CG_NONCE_REJECTED;
  u256w e;
  ec_sign_e(e, h);
  G.touch(k, digits_out);
  alignas(8) uint8_t slot[sizeof(ge_p2)];
  memset(slot, 0, sizeof slot);
  memcpy(slot, &k, sizeof k);
  if (!ec_slot_fixed_base<C>(slot, *G.T, G.K)) return CG_NONCE_REJECTED;
  Jac P;
  memcpy(&P, slot, sizeof P);
  f29 zi, km, kinv;
  m29_inv<C, 0>(zi, P.Z, G.K.one_p);
  u256w r;
  ec_sign_r<C>(r, P, zi);
  m29_from_plain<C, 1>(km, k, G.K.r2_n);
  m29_inv<C, 1>(kinv, km, G.K.one_n);
  return ec_sign_finish<C>(out, len, r, e, sg.d_m, kinv);
}
static uint8_t sign_digest(int curve, const uint8_t* d_be, const uint32_t h[8], const uint8_t* k_be, uint8_t* out72,
                           uint32_t* len, int32_t* digits_out) {
  u256w d, k;
  from_be(d, d_be);
  from_be(k, k_be);
  uint32_t out[CG_EC_SIG_WORDS];
  const uint8_t st = curve == CG_CURVE_R1 ? sign_lane(g_r1, d, h, k, out, *len, digits_out)
                                          : sign_lane(g_k1, d, h, k, out, *len, digits_out);
  memcpy(out72, out, CG_EC_SIG_SLOT);
  return st;
}

extern "C" {
int t_wide_bw() { return EC_WIDE_GW; }
int t_g_digits() { return EC_WIDE_GDIGITS; }

// r = x mod n for a canonical x < p (32 big-endian bytes each)
void t_x_mod_n(int curve, const uint8_t* x_be, uint8_t* r_be) {
  u256w x, r;
  from_be(x, x_be);
  if (curve == CG_CURVE_R1) ec_x_mod_n<CG_CURVE_R1>(r, x);
  else ec_x_mod_n<CG_CURVE_K1>(r, x);
  to_be(r_be, r);
}

// StdDSAEncoder.encode(r, s) into the 72-byte slot; returns the length
uint32_t t_der(const uint8_t* r_be, const uint8_t* s_be, uint8_t* out72) {
  u256w r, s;
  from_be(r, r_be);
  from_be(s, s_be);
  uint32_t out[CG_EC_SIG_WORDS];
  const uint32_t len = ec_sig_der(out, r, s);
  memcpy(out72, out, CG_EC_SIG_SLOT);
  return len;
}

// k_ec_signer_expand's lane: the load status, X || Y
int t_signer_load(int curve, const uint8_t* d_be, uint8_t* xy64) {
  u256w d;
  from_be(d, d_be);
  memset(xy64, 0, 64);
  if (!ec_scalar_in_range(curve, d)) return CG_KEY_INVALID;
  Jac Q;
  f29 zi;
  if (curve == CG_CURVE_R1) {
    g_r1.touch(d, nullptr);
    if (!ec_fixed_base<CG_CURVE_R1>(Q, d, *g_r1.T, g_r1.K)) return CG_KEY_INVALID;
    m29_inv<CG_CURVE_R1, 0>(zi, Q.Z, g_r1.K.one_p);
    ec_affine_be<CG_CURVE_R1>((uint32_t*)xy64, Q, zi);
  } else {
    g_k1.touch(d, nullptr);
    if (!ec_fixed_base<CG_CURVE_K1>(Q, d, *g_k1.T, g_k1.K)) return CG_KEY_INVALID;
    m29_inv<CG_CURVE_K1, 0>(zi, Q.Z, g_k1.K.one_p);
    ec_affine_be<CG_CURVE_K1>((uint32_t*)xy64, Q, zi);
  }
  return 0;
}

// Crypto.doSign(privateKey, clearData): the arena form, msg at byte phase `phase`
int t_sign_arena(int curve, const uint8_t* d_be, const uint8_t* msg, uint64_t mlen, uint32_t phase, const uint8_t* k_be,
                 uint8_t* out72, uint32_t* len, int32_t* digits_out) {
  memset(out72, 0, CG_EC_SIG_SLOT);
  *len = 0;
  if (mlen == 0) return CG_EMPTY;
  const Arena a(msg, mlen, phase);
  uint32_t h[8];
  sha256_ld_suffix(h, a.ld(), a.off, mlen, (const uint32_t*)nullptr);
  return sign_digest(curve, d_be, h, k_be, out72, len, digits_out);
}
// the splice form over prefix || id || suffix, resumed from the prefix's midstate
int t_sign_splice(int curve, const uint8_t* d_be, const uint8_t* pre, uint32_t plen, const uint8_t* id,
                  const uint8_t* suf, uint32_t slen, const uint8_t* k_be, uint8_t* out72, uint32_t* len) {
  const Splice sp(pre, plen, id, suf, slen);
  uint32_t h[8];
  sha256_ld_suffix(h, sp.ld(), 0, sp.len, (const uint32_t*)nullptr, sp.mid, sp.blocks);
  return sign_digest(curve, d_be, h, k_be, out72, len, nullptr);
}
}

#ifdef SIGN_EC_MAIN
// Cases, one per line, fields in hex ("-" = empty), scheme 2 / 3:
//   M scheme d msg k status sig                 the arena form (at all four byte phases)
//   T scheme d prefix id suffix k status sig    the splice form
//   X scheme x r                                r = x mod n
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
static int curve_of(int scheme) { return scheme == CG_ECDSA_SECP256R1_SHA256 ? CG_CURVE_R1 : CG_CURVE_K1; }
static bool same(int st, uint32_t len, const uint8_t* out72, int want_st, const std::vector<uint8_t>& want) {
  uint8_t slot[CG_EC_SIG_SLOT] = {0};
  if (!want.empty()) memcpy(slot, want.data(), want.size());
  return st == want_st && len == want.size() && !memcmp(out72, slot, CG_EC_SIG_SLOT);
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
    uint8_t out[CG_EC_SIG_SLOT];
    uint32_t len = 0;
    if (f[0] == "X" && f.size() == 4) {
      const std::vector<uint8_t> x = unhex(f[2]), r = unhex(f[3]);
      if (x.size() != 32 || r.size() != 32) return 2;
      uint8_t got[32];
      t_x_mod_n(curve_of(atoi(f[1].c_str())), x.data(), got);
      if (memcmp(got, r.data(), 32)) ++bad;
    } else if (f[0] == "M" && f.size() == 7) {
      const std::vector<uint8_t> d = unhex(f[2]), msg = unhex(f[3]), k = unhex(f[4]), want = unhex(f[6]);
      if (d.size() != 32 || k.size() != 32 || want.size() > CG_EC_SIG_SLOT) return 2;
      const uint8_t none = 0;
      for (uint32_t phase = 0; phase < 4; ++phase) {
        const int st = t_sign_arena(curve_of(atoi(f[1].c_str())), d.data(), msg.empty() ? &none : msg.data(), msg.size(),
                                    phase, k.data(), out, &len, nullptr);
        if (!same(st, len, out, atoi(f[5].c_str()), want)) ++bad;
      }
    } else if (f[0] == "T" && f.size() == 9) {
      const std::vector<uint8_t> d = unhex(f[2]), pre = unhex(f[3]), id = unhex(f[4]), suf = unhex(f[5]), k = unhex(f[6]),
                                 want = unhex(f[8]);
      if (d.size() != 32 || k.size() != 32 || id.size() != 32 || want.size() > CG_EC_SIG_SLOT) return 2;
      const int st = t_sign_splice(curve_of(atoi(f[1].c_str())), d.data(), pre.data(), (uint32_t)pre.size(), id.data(),
                                   suf.data(), (uint32_t)suf.size(), k.data(), out, &len);
      if (!same(st, len, out, atoi(f[7].c_str()), want)) ++bad;
    } else {
      return 2;
    }
  }
  printf("%d cases, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}
#endif
