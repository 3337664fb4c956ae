// Lane code of Crypto.deriveKeyPair (core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:646-771) for
// the kernels of derive_keys.hip, HIP-free (host + device) so the host tests reach it:
//   deriveHMAC          HMAC-SHA512(keyData, seed): the parent's two midstates (after K xor ipad, after
//                       K xor opad), the inner hash resumed over the seed bytes, one outer block
//   deriveKeyPairEdDSA  child seed = mac[0..32); EdDSAPrivateKeySpec(seed) is ed_signer_scalars
//   deriveKeyPairECDSA  d = BigInteger(1, mac[0..32)), the accept rule of BC's ECKeyPairGenerator plus
//                       d < n, and on a refusal the whole derivation again with seed := SHA-256(seed),
//                       at most CG_DERIVE_MAX_RETRIES times
// Secret: the midstates, every mac, d and the digits (include/cordagpu.h).
#pragma once
#include "../../include/cordagpu.h"
#include "ecdsa_rows.h"
#include "ed25519_rows.h"

// SHA-512 state after the one block K xor ipad / K xor opad of a parent key
struct HmacMid {
  uint64_t in[8], out[8];
};

CG_HD void hmac512_pad_state(uint64_t s[8], const uint32_t kw[32], uint32_t pad) {
  uint64_t w[16];
#pragma unroll
  for (int j = 0; j < 16; ++j)
    w[j] = ((uint64_t)CG_BSWAP32(kw[2 * j] ^ pad) << 32) | CG_BSWAP32(kw[2 * j + 1] ^ pad);
  sha512_init(s);
  sha512_compress(s, w);
}

// key_len in [1, 128] (a longer key would be hashed first: the callers refuse it)
template <class Ld>
CG_HD void hmac512_midstates(HmacMid& m, const Ld& ld, uint64_t key_off, uint32_t key_len) {
  uint32_t kw[32];  // the key, zero-padded to the block, as little-endian words
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const uint32_t pos = 4u * (uint32_t)j;
    uint32_t w = 0;
    if (pos < key_len) {
      w = ld.bytes4(key_off + pos);
      const uint32_t rem = key_len - pos;
      if (rem < 4) w &= 0xffffffffu >> (32u - 8u * rem);
    }
    kw[j] = w;
  }
  hmac512_pad_state(m.in, kw, 0x36363636u);
  hmac512_pad_state(m.out, kw, 0x5c5c5c5cu);
}

// The outer hash: one block (the 64 inner digest bytes, padding, length 128 + 64) from the opad
// midstate. mac: the 64 bytes as 16 little-endian words.
CG_HD void hmac512_outer(uint32_t mac[16], const HmacMid& m, const uint64_t inner[8]) {
  uint64_t s[8], w[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    s[k] = m.out[k];
    w[k] = inner[k];
  }
  w[8] = 0x8000000000000000ULL;
#pragma unroll
  for (int k = 9; k < 15; ++k) w[k] = 0;
  w[15] = (128 + 64) * 8;
  sha512_compress(s, w);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    mac[2 * k] = CG_BSWAP32((uint32_t)(s[k] >> 32));
    mac[2 * k + 1] = CG_BSWAP32((uint32_t)s[k]);
  }
}

// HMAC-SHA512 of the seed bytes at ld[off, off + len) (len 0 is legal)
template <class Ld>
CG_HD void hmac512_ld(uint32_t mac[16], const HmacMid& m, const Ld& ld, uint64_t off, uint64_t len) {
  uint64_t s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = m.in[k];
  sha512_resume128_ld(s, ld, off, len);
  hmac512_outer(mac, m, s);
}

// HMAC-SHA512 of a 32-byte seed held as 8 big-endian words (a SHA-256 digest: the rehashed seed)
CG_HD void hmac512_digest32(uint32_t mac[16], const HmacMid& m, const uint32_t seed_be[8]) {
  uint64_t s[8], w[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = m.in[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = ((uint64_t)seed_be[2 * k] << 32) | seed_be[2 * k + 1];
  w[4] = 0x8000000000000000ULL;
#pragma unroll
  for (int k = 5; k < 15; ++k) w[k] = 0;
  w[15] = (128 + 32) * 8;
  sha512_compress(s, w);
  hmac512_outer(mac, m, s);
}

// SHA-256 of a 32-byte digest held as 8 big-endian words, in place
CG_HD void sha256_digest32(uint32_t d[8]) {
  uint32_t s[8], w[16];
  sha256_init(s);
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = d[k];
  w[8] = 0x80000000u;
#pragma unroll
  for (int k = 9; k < 15; ++k) w[k] = 0;
  w[15] = 256;
  sha256_compress(s, w);
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = s[k];
}

// d = BigInteger(1, b[0..32)) for 32 big-endian bytes held as 8 little-endian words
CG_HD void ec_secret_from_be(u256w& d, const uint32_t b[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) d.w[7 - k] = CG_BSWAP32(b[k]);
}

// The accept rule: d >= 2, d < n, and WNafUtil.getNafWeight(d) = bitCount(3d xor d) >= n.bitLength() >>> 2
// (64 on both curves).
template <int C>
CG_HD bool ec_secret_accept(const u256w& d) {
  uint32_t hi = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i) hi |= d.w[i];
  if (hi == 0 && d.w[0] < 2) return false;
  if (!u256_lt_mod<C, 1>(d)) return false;
  uint32_t carry = 0;
  int weight = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = 3ull * d.w[i] + carry;
    carry = (uint32_t)(t >> 32);
    weight += __builtin_popcount((uint32_t)t ^ d.w[i]);
  }
  weight += __builtin_popcount(carry);
  return weight >= 64;
}
CG_HD bool ec_secret_accept(int curve, const u256w& d) {
  return curve == CG_CURVE_R1 ? ec_secret_accept<CG_CURVE_R1>(d) : ec_secret_accept<CG_CURVE_K1>(d);
}

// The attempts of one ECDSA item. mac_of(a, mac) is attempt a's mac, rehash(a) replaces the seed by its
// SHA-256 behind a refused attempt a. The first `force` attempts are refused whatever their d
// (CG_TEST_DERIVE_FORCE_RETRIES). Returns 0 with d and the count of rehashes made, or CG_DERIVE_HOST
// when attempt CG_DERIVE_MAX_RETRIES is refused too. The loop ends after CG_DERIVE_MAX_RETRIES + 1
// rounds whatever the input.
template <class MacFn, class RehashFn>
CG_HD uint8_t ec_derive_attempts(u256w& d, uint32_t mac[16], uint32_t& retries, int curve, uint32_t force,
                                 MacFn mac_of, RehashFn rehash) {
  for (uint32_t a = 0; a <= CG_DERIVE_MAX_RETRIES; ++a) {
    mac_of(a, mac);
    ec_secret_from_be(d, mac);
    retries = a;
    if (a >= force && ec_secret_accept(curve, d)) return 0;
    if (a < CG_DERIVE_MAX_RETRIES) rehash(a);
  }
  return CG_DERIVE_HOST;
}

// deriveKeyPairECDSA's scalar for the seed at ld[off, off + len) under the parent midstates m
template <class Ld>
CG_HD uint8_t ec_derive_scalar(u256w& d, uint32_t mac[16], uint32_t& retries, int curve, uint32_t force,
                               const HmacMid& m, const Ld& ld, uint64_t off, uint64_t len) {
  uint32_t seed[8];  // from the first rehash on: SHA-256 of the previous seed, big-endian words
  return ec_derive_attempts(
      d, mac, retries, curve, force,
      [&](uint32_t a, uint32_t* out) {
        if (a == 0) hmac512_ld(out, m, ld, off, len);
        else hmac512_digest32(out, m, seed);
      },
      [&](uint32_t a) {
        if (a == 0) sha256_ld_suffix(seed, ld, off, len, (const uint32_t*)nullptr);
        else sha256_digest32(seed);
      });
}

// d G over the constant radix-2^EC_WIDE_GW table. False when the result is infinity (never for
// 2 <= d < n: G has prime order n).
template <int C, class TabG>
CG_HD bool ec_fixed_base(Jac& R, const u256w& d, const TabG& TG, const EcConsts& K) {
  bool inf = true;
  jac_set_inf<C>(R, K);
  ec_add_g_wide<C>(R, inf, d, TG, K);
  return !inf;
}

// The k G of an item slot in place: the slot's scalar (u256w) becomes the Jacobian result. False at
// infinity (the slot keeps the scalar). Shared by k_derive_ec_mul (derive_keys.hip) and k_ec_sign_mul
// (sign_ec.hip).
template <int C, class TabG>
CG_HD bool ec_slot_fixed_base(void* slot, const TabG& TG, const EcConsts& K) {
  const u256w d = *(const u256w*)slot;
  Jac R;
  if (!ec_fixed_base<C>(R, d, TG, K)) return false;
  *(Jac*)slot = R;
  return true;
}

// X || Y big-endian (16 little-endian words of the 64 bytes) of the Jacobian P given zi = 1 / P.Z
template <int C>
CG_HD void ec_affine_be(uint32_t out[16], const Jac& P, const f29& zi) {
  f29 zi2, zi3, x, y;
  m29_sq<C, 0>(zi2, zi);
  m29_mul<C, 0>(zi3, zi2, zi);
  m29_mul<C, 0>(x, P.X, zi2);
  m29_mul<C, 0>(y, P.Y, zi3);
  u256w xp, yp;
  m29_to_plain<C, 0>(xp, x);
  m29_to_plain<C, 0>(yp, y);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out[k] = CG_BSWAP32(xp.w[7 - k]);
    out[8 + k] = CG_BSWAP32(yp.w[7 - k]);
  }
}
