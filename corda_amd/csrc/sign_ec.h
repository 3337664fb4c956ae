// Lane code of ECDSA signing (BC 1.57 SHA256withECDSA behind Crypto.doSign, core/src/main/kotlin/net/
// corda/core/crypto/Crypto.kt:395-402, 415-422; NotaryService.kt:73-80) for the kernels of sign_ec.hip,
// HIP-free (host + device) so the host tests reach it. DSABase.engineSign -> ECDSASigner.generateSignature
// -> StdDSAEncoder.encode with the nonce given: the caller draws RandomDSAKCalculator.nextK's
// BigInteger(256, random) candidate, and one candidate is one attempt of BC's loop.
//   e = BigInteger(1, SHA-256(M))        256-bit n: no shift; used unreduced (e < 2^256 < 2n)
//   k refused unless 0 < k < n
//   r = x(k G) mod n                     one conditional subtraction: x < p < 2n on both curves
//   s = k^-1 (e + d r) mod n             refused when r = 0 or s = 0
//   DERSequence(ASN1Integer(r), ASN1Integer(s)), minimal two's complement: 8 .. 72 bytes
// Secret: d, k, k^-1 (given one k, d = (s k - e) / r).
#pragma once
#include "derive.h"

#define CG_EC_SIG_SLOT 72  // bytes per signature slot: the DER bytes, then zeros
#define CG_EC_SIG_WORDS (CG_EC_SIG_SLOT / 4)

// A loaded signer: d as the finish kernel multiplies with it (Montgomery mod n), and its class:
// 0 refused at load (its requests are CG_NOT_RUN), else 1 + curve.
struct EcSigner {
  f29 d_m;
  uint32_t cls;
};

// The load check: 0 < d < n
template <int C>
CG_HD bool ec_scalar_in_range(const u256w& d) {
  return !u256_iszero(d) && u256_lt_mod<C, 1>(d);
}
CG_HD bool ec_scalar_in_range(int curve, const u256w& d) {
  return curve == CG_CURVE_R1 ? ec_scalar_in_range<CG_CURVE_R1>(d) : ec_scalar_in_range<CG_CURVE_K1>(d);
}

template <int C>
CG_HD void ec_signer_init(EcSigner& sg, const u256w& d, const EcConsts& K) {
  m29_from_plain<C, 1>(sg.d_m, d, K.r2_n);
  sg.cls = 1u + (uint32_t)C;
}

// e = BigInteger(1, digest) for the SHA-256 state h (8 big-endian words)
CG_HD void ec_sign_e(u256w& e, const uint32_t h[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) e.w[i] = h[7 - i];
}

// r = x mod n for a canonical x < p
template <int C>
CG_HD void ec_x_mod_n(u256w& r, const u256w& x) {
  const bool take = !u256_lt_mod<C, 1>(x);
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)x.w[i] - Mod<C, 1>::w(i) - br;
    r.w[i] = take ? (uint32_t)t : x.w[i];
    br = (uint32_t)(t >> 63);
  }
}

// r = x(P) mod n of the finite Jacobian P given zi = 1 / P.Z
template <int C>
CG_HD void ec_sign_r(u256w& r, const Jac& P, const f29& zi) {
  f29 zi2, x;
  m29_sq<C, 0>(zi2, zi);
  m29_mul<C, 0>(x, P.X, zi2);
  u256w xp;
  m29_to_plain<C, 0>(xp, x);
  ec_x_mod_n<C>(r, xp);
}

// s = k^-1 (e + r d) mod n: r < n and e < 2^256 plain, d and k^-1 Montgomery
template <int C>
CG_HD void ec_sign_s(u256w& s, const u256w& r, const u256w& e, const f29& d_m, const f29& kinv_m) {
  f29 t, u;
  f29_from_words(t, r.w);
  m29_mul<C, 1>(u, t, d_m);  // r d (plain, < 2n)
  f29_from_words(t, e.w);    // < 2^256 < 2n
  m29_add_lazy(u, u, t);     // < 4n, limbs < 2^30: a product's operand
  m29_mul<C, 1>(t, u, kinv_m);
  m29_to_words_canon<C, 1>(s.w, t);
}

// ---- StdDSAEncoder.encode in registers. The signature is a 72-byte big-endian string held as 18
// little-endian words (o[17] = bytes 0..3): every position is a byte shift of a multi-word value, so
// nothing is indexed by a per-lane byte position.
// content bytes of ASN1Integer(v), v > 0: (bitLength + 8) / 8
CG_HD uint32_t ec_der_int_len(const u256w& v) {
  uint32_t bl = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (v.w[i]) bl = 32u * (uint32_t)i + 32u - (uint32_t)__builtin_clz(v.w[i]);
  return (bl + 8u) >> 3;
}
// o |= v << (8 sh), sh <= 67 (the shifted value stays inside the 72 bytes)
CG_HD void ec_der_place(uint32_t o[CG_EC_SIG_WORDS], const u256w& v, uint32_t sh) {
  uint32_t x[CG_EC_SIG_WORDS];
  const uint32_t t = 8u * (sh & 3u), q = sh >> 2;
#pragma unroll
  for (int i = 0; i < CG_EC_SIG_WORDS; ++i) {
    const uint64_t lo = i < 8 ? v.w[i] : 0u, prev = i > 0 && i <= 8 ? v.w[i - 1] : 0u;
    x[i] = (uint32_t)(((lo << 32 | prev) << t) >> 32);
  }
#pragma unroll
  for (int b = 1; b <= 16; b <<= 1) {
    const bool on = (q & (uint32_t)b) != 0;
#pragma unroll
    for (int i = CG_EC_SIG_WORDS - 1; i >= 0; --i) {
      const uint32_t from = i >= b ? x[i - b] : 0u;
      x[i] = on ? from : x[i];
    }
  }
#pragma unroll
  for (int i = 0; i < CG_EC_SIG_WORDS; ++i) o[i] |= x[i];
}
CG_HD void ec_der_put(uint32_t o[CG_EC_SIG_WORDS], uint32_t pos, uint32_t byte) {
#pragma unroll
  for (int i = 0; i < CG_EC_SIG_WORDS; ++i) o[i] |= (uint32_t)i == (pos >> 2) ? byte << (8u * (pos & 3u)) : 0u;
}
// The slot's 18 memory words (DER bytes, then zeros) for r, s in [1, n); returns the DER length
CG_HD uint32_t ec_sig_der(uint32_t out[CG_EC_SIG_WORDS], const u256w& r, const u256w& s) {
  const uint32_t lr = ec_der_int_len(r), ls = ec_der_int_len(s), body = lr + ls + 4u;
  uint32_t o[CG_EC_SIG_WORDS];
#pragma unroll
  for (int i = 0; i < CG_EC_SIG_WORDS; ++i) o[i] = 0;
  o[CG_EC_SIG_WORDS - 1] = 0x30000200u | (body << 16) | lr;  // 30 len 02 len(r)
  ec_der_place(o, r, 68u - lr);
  ec_der_put(o, 67u - lr, 0x02u);
  ec_der_put(o, 66u - lr, ls);
  ec_der_place(o, s, 66u - lr - ls);
#pragma unroll
  for (int i = 0; i < CG_EC_SIG_WORDS; ++i) out[i] = CG_BSWAP32(o[CG_EC_SIG_WORDS - 1 - i]);
  return body + 2u;
}

// The finish of one item given k^-1 (Montgomery): s, the refusals, the encoding. Returns the status
// (0 or CG_NONCE_REJECTED); out / len are the slot's words and length byte either way.
template <int C>
CG_HD uint8_t ec_sign_finish(uint32_t out[CG_EC_SIG_WORDS], uint32_t& len, const u256w& r, const u256w& e,
                             const f29& d_m, const f29& kinv_m) {
  u256w s;
  ec_sign_s<C>(s, r, e, d_m, kinv_m);
  if (u256_iszero(r) || u256_iszero(s)) {
#pragma unroll
    for (int i = 0; i < CG_EC_SIG_WORDS; ++i) out[i] = 0;
    len = 0;
    return CG_NONCE_REJECTED;
  }
  len = ec_sig_der(out, r, s);
  return 0;
}
