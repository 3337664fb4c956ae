// Host build of the key-derivation lane code (corda_amd/csrc/derive.h: the HMAC-SHA512 midstates and
// lanes, the ECDSA accept rule, the bounded rehash loop, d G over the constant G table, the affine
// output; and the Ed25519 child key over ed_signer_scalars / ed_fixed_base9 / ed_encode) with
// FE_BOUNDS_CHECK on: the arithmetic the kernels of derive_keys.hip run, checked on the CPU. Built once
// per radix (-DED_WIDE_BW=-DEC_WIDE_GW=26 / 24 / 22, tests/hostderive.py). With -DDERIVE_MAIN it is a
// stand-alone program over a text file of cases, which the tests build with the sanitizers.
// Test infrastructure only.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <string>
#include <vector>

#include "../../corda_amd/csrc/derive.h"

static_assert(ED_WIDE_BW == EC_WIDE_GW, "one fixed-base radix per build");

// ---- the constant tables, mapped without backing store; only the groups a scalar's digits touch are
// built, with the device lanes' code (ed_bwide_group, ec_gwide_group_from)
static void* map_sparse(size_t bytes) {
  void* m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (m == MAP_FAILED) abort();
  return m;
}

static Ed25519Consts g_C;
static EdBWideTab* g_TB = nullptr;
static std::vector<bool> g_built;
static ge_p3 g_base[EdWideCfg::kBDigits];  // 2^{ED_WIDE_BW u} B
static void tb_init() {
  if (g_TB) return;
  ed_consts_init(g_C);
  g_TB = (EdBWideTab*)map_sparse(sizeof(EdBWideTab));
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
    T = (EcGWideTab*)map_sparse(sizeof(EcGWideTab));
    S = new EcRowScratch;
    built.assign((size_t)EC_WIDE_GDIGITS * (EC_WIDE_GMULT / EC_MULT), false);
    Jac P = {K.gx, K.gy, K.one_p};
    for (int u = 0; u < EC_WIDE_GDIGITS; ++u) {
      if (u > 0) jac_dbl_n<C>(P, P, EC_WIDE_GW);
      base[u] = P;
    }
  }
  // digits_out (optional): the EC_WIDE_GDIGITS signed digits the rows are read by
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

static void midstates(HmacMid& m, const uint8_t* key, uint32_t klen, uint32_t phase) {
  const Arena k(key, klen, phase);
  hmac512_midstates(m, k.ld(), k.off, klen);
}

// d G as X || Y big-endian; false at infinity
template <int C>
static bool fixed_base_xy(GTab<C>& G, const u256w& d, uint32_t xy[16], int32_t* digits_out) {
  G.touch(d, digits_out);
  Jac R;
  if (!ec_fixed_base<C>(R, d, *G.T, G.K)) return false;
  f29 zi;
  m29_inv<C, 0>(zi, R.Z, G.K.one_p);
  ec_affine_be<C>(xy, R, zi);
  return true;
}

static void ed_public(uint32_t abyte[8], const uint32_t seed[8]) {
  tb_init();
  EdSigner sg;
  uint32_t es[EdWideCfg::kBPackedWords];
  ed_signer_scalars(sg, es, seed);
  tb_touch(es);
  ge_p2 q;
  ed_fixed_base9(q, es, *g_TB);
  fe zi;
  fe_invert(zi, q.Z);
  ed_encode(abyte, q, zi);
}

extern "C" {
int t_wide_bw() { return ED_WIDE_BW; }
int t_g_digits() { return EC_WIDE_GDIGITS; }

// HMAC-SHA512(key, msg): key and msg each at byte phase `phase` of an arena of their own
void t_hmac512(const uint8_t* key, uint32_t klen, const uint8_t* msg, uint64_t len, uint32_t phase, uint8_t* out64) {
  HmacMid m;
  midstates(m, key, klen, phase);
  const Arena a(msg, len, phase);
  hmac512_ld((uint32_t*)out64, m, a.ld(), a.off, len);
}
// the rehashed form: HMAC-SHA512(key, SHA-256(msg)) through sha256_ld_suffix + hmac512_digest32, and
// once more through sha256_digest32 (out: 2 x 64 bytes)
void t_hmac512_rehashed(const uint8_t* key, uint32_t klen, const uint8_t* msg, uint64_t len, uint32_t phase,
                        uint8_t* out128) {
  HmacMid m;
  midstates(m, key, klen, phase);
  const Arena a(msg, len, phase);
  uint32_t seed[8];
  sha256_ld_suffix(seed, a.ld(), a.off, len, (const uint32_t*)nullptr);
  hmac512_digest32((uint32_t*)out128, m, seed);
  sha256_digest32(seed);
  hmac512_digest32((uint32_t*)(out128 + 64), m, seed);
}

int t_accept(int curve, const uint8_t* d_be) {
  u256w d;
  uint32_t w[8];
  memcpy(w, d_be, 32);
  ec_secret_from_be(d, w);
  return ec_secret_accept(curve, d) ? 1 : 0;
}

// d G for any d < 2^256 (the accept rule is not applied); returns 0 at infinity
int t_ec_fixed_base(int curve, const uint8_t* d_be, uint8_t* xy64, int32_t* digits_out) {
  u256w d;
  uint32_t w[8];
  memcpy(w, d_be, 32);
  ec_secret_from_be(d, w);
  return curve == CG_CURVE_R1 ? fixed_base_xy(g_r1, d, (uint32_t*)xy64, digits_out)
                              : fixed_base_xy(g_k1, d, (uint32_t*)xy64, digits_out);
}

// The lane of an ECDSA item (ec_derive_scalar, then d G): status, secret (d big-endian), X || Y, rehashes
int t_derive_ec(int curve, uint32_t force, const uint8_t* key, uint32_t klen, const uint8_t* seed, uint64_t len,
                uint32_t phase, uint8_t* secret32, uint8_t* xy64, uint32_t* retries) {
  HmacMid m;
  midstates(m, key, klen, phase);
  const Arena a(seed, len, phase);
  u256w d;
  uint32_t mac[16];
  memset(secret32, 0, 32);
  memset(xy64, 0, 64);
  const uint8_t st = ec_derive_scalar(d, mac, *retries, curve, force, m, a.ld(), a.off, len);
  if (st != 0) return st;
  memcpy(secret32, mac, 32);
  const bool ok = curve == CG_CURVE_R1 ? fixed_base_xy(g_r1, d, (uint32_t*)xy64, nullptr)
                                       : fixed_base_xy(g_k1, d, (uint32_t*)xy64, nullptr);
  return ok ? 0 : CG_DERIVE_HOST;
}

// ec_derive_attempts over injected macs (64 bytes per attempt, CG_DERIVE_MAX_RETRIES + 1 of them):
// status, d big-endian, rehashes; *rehash_calls counts the rehashes the lane asked for
int t_derive_attempts(int curve, uint32_t force, const uint8_t* macs, uint8_t* d_be, uint32_t* retries,
                      uint32_t* rehash_calls) {
  u256w d;
  uint32_t mac[16];
  *rehash_calls = 0;
  const uint8_t st = ec_derive_attempts(
      d, mac, *retries, curve, force, [&](uint32_t a, uint32_t* out) { memcpy(out, macs + 64 * a, 64); },
      [&](uint32_t) { ++*rehash_calls; });
  memcpy(d_be, mac, 32);
  return st;
}

// The lane of an Ed25519 item: child seed = mac[0..32), Abyte
void t_derive_ed(const uint8_t* key, uint32_t klen, const uint8_t* seed, uint64_t len, uint32_t phase, uint8_t* secret32,
                 uint8_t* abyte32) {
  uint32_t mac[16];
  t_hmac512(key, klen, seed, len, phase, (uint8_t*)mac);
  memcpy(secret32, mac, 32);
  ed_public((uint32_t*)abyte32, mac);
}
void t_ed_public(const uint8_t* seed32, uint8_t* abyte32) {
  uint32_t s[8];
  memcpy(s, seed32, 32);
  ed_public((uint32_t*)abyte32, s);
}
}

#ifdef DERIVE_MAIN
// Cases, one per line, fields in hex ("-" = empty), scheme 2 / 3 / 4:
//   H key msg mac                       HMAC-SHA512 at all four byte phases
//   A scheme d accept(0/1)              the accept rule
//   G scheme d xy                       d G
//   D scheme force key seed status secret pub retries    one item's lane at all four byte phases
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
  const uint8_t none = 0;
  for (const std::string& l : lines) {
    const std::vector<std::string> f = split(l);
    if (f.empty()) continue;
    ++n;
    if (f[0] == "H" && f.size() == 4) {
      const std::vector<uint8_t> key = unhex(f[1]), msg = unhex(f[2]), want = unhex(f[3]);
      if (key.empty() || key.size() > 128 || want.size() != 64) return 2;
      for (uint32_t phase = 0; phase < 4; ++phase) {
        uint8_t mac[64];
        t_hmac512(key.data(), (uint32_t)key.size(), msg.empty() ? &none : msg.data(), msg.size(), phase, mac);
        if (memcmp(mac, want.data(), 64)) ++bad;
      }
    } else if (f[0] == "A" && f.size() == 4) {
      const std::vector<uint8_t> d = unhex(f[2]);
      if (d.size() != 32) return 2;
      if (t_accept(curve_of(atoi(f[1].c_str())), d.data()) != atoi(f[3].c_str())) ++bad;
    } else if (f[0] == "G" && f.size() == 4) {
      const std::vector<uint8_t> d = unhex(f[2]), want = unhex(f[3]);
      if (d.size() != 32 || want.size() != 64) return 2;
      uint8_t xy[64];
      if (!t_ec_fixed_base(curve_of(atoi(f[1].c_str())), d.data(), xy, nullptr) || memcmp(xy, want.data(), 64)) ++bad;
    } else if (f[0] == "D" && f.size() == 9) {
      const int scheme = atoi(f[1].c_str());
      const uint32_t force = (uint32_t)atoi(f[2].c_str());
      const std::vector<uint8_t> key = unhex(f[3]), seed = unhex(f[4]), sec = unhex(f[6]), pub = unhex(f[7]);
      if (key.empty() || key.size() > 128 || sec.size() != 32 || pub.size() != 64) return 2;
      for (uint32_t phase = 0; phase < 4; ++phase) {
        uint8_t s[32], p[64] = {0};
        uint32_t tries = 0;
        int st = 0;
        const uint8_t* sd = seed.empty() ? &none : seed.data();
        if (scheme == CG_EDDSA_ED25519_SHA512) t_derive_ed(key.data(), (uint32_t)key.size(), sd, seed.size(), phase, s, p);
        else st = t_derive_ec(curve_of(scheme), force, key.data(), (uint32_t)key.size(), sd, seed.size(), phase, s, p, &tries);
        if (st != atoi(f[5].c_str()) || (int)tries != atoi(f[8].c_str()) || memcmp(s, sec.data(), 32) ||
            memcmp(p, pub.data(), 64))
          ++bad;
      }
    } else {
      return 2;
    }
  }
  printf("%d cases, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}
#endif
