// RSA_SHA256 (Corda scheme 1, BouncyCastle "SHA256WITHRSAANDMGF1": RSASSA-PSS, SHA-256, MGF1-SHA256,
// 32-byte salt, trailer 0xBC) for host and device: the strict key decode, the per-key Montgomery
// constants and the EMSA-PSS check of BC 1.57 PSSSigner.verifySignature as corda_amd/hostverify.py
// restates it. The lane-cooperative modular exponentiation lives in rsa_wave.h; the scalar one
// here serves the key preparation (one lane per key) and the host tests (tests/native/host_rsa.cpp).
//
// Accepted keys (everything else keeps CG_UNSUPPORTED and goes to the host fallback, which owns the
// reference's exceptions): canonical DER SubjectPublicKeyInfo { AlgorithmIdentifier { rsaEncryption,
// parameters absent or NULL }, BIT STRING (0 unused bits) { RSAPublicKey { n, e } } }, every length
// minimal, no trailing bytes, both INTEGERs minimal and positive, n odd with 1024 <= bitlen(n) <= 4096
// (any bit length), 1 <= e < 2^32.
#pragma once
#include "sha2.h"

#define RSA_MIN_BITS 1024u
#define RSA_MAX_BITS 4096u
#define RSA_MAX_LIMBS 128u
#define RSA_HASH_LEN 32u
#define RSA_SALT_LEN 32u
#define RSA_TRAILER 0xBCu

// Per-key record the key-prep kernel writes and the verify kernel reads (1056 bytes).
struct RsaKeyRec {
  uint32_t ok;         // 1: accepted (the fields below are valid), 0: not accepted
  uint32_t bits;       // bitlen(n)
  uint32_t L;          // ceil(bits / 32) limbs
  uint32_t k;          // ceil(bits / 8): the longest signature
  uint32_t em_bits;    // bits - 1
  uint32_t block_len;  // ceil(em_bits / 8)
  uint32_t e;
  uint32_t n0inv;      // -n^-1 mod 2^32
  uint32_t n[RSA_MAX_LIMBS];   // little-endian limbs, zero above L
  uint32_t rr[RSA_MAX_LIMBS];  // R^2 mod n, R = 2^(32 L)
};

CG_HD uint32_t rsa_byte(const uint8_t* arena, uint64_t lr, uint64_t off) {
  return cg_ld_bytes4(arena, lr, off) & 0xffu;
}

// One DER tag-length header at [pos, end): the tag must be `tag`, the length minimal (short form
// below 128, 0x81 for 128..255, 0x82 for 256..65535) and the content inside [pos, end). On success
// pos is the content's first byte and *clen its length.
CG_HD bool rsa_der_tl(const uint8_t* arena, uint64_t lr, uint64_t& pos, uint64_t end, uint32_t tag, uint32_t* clen) {
  if (end - pos < 2) return false;
  if (rsa_byte(arena, lr, pos) != tag) return false;
  const uint32_t b = rsa_byte(arena, lr, pos + 1);
  uint32_t len;
  pos += 2;
  if (b < 0x80u) {
    len = b;
  } else if (b == 0x81u) {
    if (end - pos < 1) return false;
    len = rsa_byte(arena, lr, pos);
    pos += 1;
    if (len < 0x80u) return false;
  } else if (b == 0x82u) {
    if (end - pos < 2) return false;
    len = (rsa_byte(arena, lr, pos) << 8) | rsa_byte(arena, lr, pos + 1);
    pos += 2;
    if (len < 0x100u) return false;
  } else {
    return false;
  }
  if (len > end - pos) return false;
  *clen = len;
  return true;
}

// A minimal positive INTEGER at pos: on success *mag / *mlen are its magnitude (leading 0x00 sign
// byte dropped; the first magnitude byte is non-zero) and pos is past it.
CG_HD bool rsa_der_uint(const uint8_t* arena, uint64_t lr, uint64_t& pos, uint64_t end, uint64_t* mag, uint32_t* mlen) {
  uint32_t len;
  if (!rsa_der_tl(arena, lr, pos, end, 0x02u, &len) || len == 0) return false;
  const uint32_t b0 = rsa_byte(arena, lr, pos);
  if (b0 & 0x80u) return false;  // negative
  if (b0 == 0) {
    if (len == 1) return false;                                 // zero
    if (!(rsa_byte(arena, lr, pos + 1) & 0x80u)) return false;  // non-minimal
    *mag = pos + 1;
    *mlen = len - 1;
  } else {
    *mag = pos;
    *mlen = len;
  }
  pos += len;
  return true;
}

struct RsaKeyView {
  uint64_t n_off;  // arena offset of n's most significant byte
  uint32_t n_len;  // magnitude bytes
  uint32_t bits;
  uint32_t e;
};

// The accepted-key rule (the file comment). `arena` 4-byte aligned, readable to lr = round4(length).
CG_HD bool rsa_key_decode(RsaKeyView& v, const uint8_t* arena, uint64_t lr, uint64_t off, uint32_t len) {
  uint64_t pos = off;
  const uint64_t end = off + len;
  uint32_t l;
  if (!rsa_der_tl(arena, lr, pos, end, 0x30u, &l) || pos + l != end) return false;  // SPKI, no trailing bytes
  if (!rsa_der_tl(arena, lr, pos, end, 0x30u, &l)) return false;                    // AlgorithmIdentifier
  const uint64_t alg_end = pos + l;
  {
    const uint8_t oid[11] = {0x06, 0x09, 0x2A, 0x86, 0x48, 0x86, 0xF7, 0x0D, 0x01, 0x01, 0x01};
    if (l != 11 && l != 13) return false;
    uint32_t bad = 0;
    for (int i = 0; i < 11; ++i) bad |= rsa_byte(arena, lr, pos + i) ^ oid[i];
    if (l == 13) bad |= (rsa_byte(arena, lr, pos + 11) ^ 0x05u) | rsa_byte(arena, lr, pos + 12);  // NULL
    if (bad) return false;
  }
  pos = alg_end;
  if (!rsa_der_tl(arena, lr, pos, end, 0x03u, &l) || pos + l != end || l < 1) return false;  // BIT STRING
  if (rsa_byte(arena, lr, pos) != 0) return false;                                          // unused bits
  pos += 1;
  if (!rsa_der_tl(arena, lr, pos, end, 0x30u, &l) || pos + l != end) return false;  // RSAPublicKey
  uint64_t e_off;
  uint32_t e_len;
  if (!rsa_der_uint(arena, lr, pos, end, &v.n_off, &v.n_len)) return false;
  if (!rsa_der_uint(arena, lr, pos, end, &e_off, &e_len) || pos != end) return false;
  if (e_len > 4) return false;
  v.e = 0;
  for (uint32_t i = 0; i < e_len; ++i) v.e = (v.e << 8) | rsa_byte(arena, lr, e_off + i);
  if (v.n_len > RSA_MAX_BITS / 8) return false;
  const uint32_t top = rsa_byte(arena, lr, v.n_off);
  uint32_t tb = 0;
  while ((top >> tb) != 0) ++tb;
  v.bits = 8 * (v.n_len - 1) + tb;
  if (v.bits < RSA_MIN_BITS || v.bits > RSA_MAX_BITS) return false;
  if (!(rsa_byte(arena, lr, v.n_off + v.n_len - 1) & 1u)) return false;  // even modulus
  return true;
}

// Limb i (little-endian) of the big-endian integer arena[off, off + len).
CG_HD uint32_t rsa_be_limb(const uint8_t* arena, uint64_t lr, uint64_t off, uint32_t len, uint32_t i) {
  if (4 * i >= len) return 0u;
  const uint32_t rem = len - 4 * i;
  if (rem >= 4) return CG_BSWAP32(cg_ld_bytes4(arena, lr, off + rem - 4));
  return CG_BSWAP32(cg_ld_bytes4(arena, lr, off)) >> (8u * (4u - rem));
}

CG_HD uint32_t rsa_n0inv(uint32_t n0) {  // n0 odd
  uint32_t x = n0;                       // 3 correct bits; each step doubles them
  for (int i = 0; i < 5; ++i) x *= 2u - n0 * x;
  return 0u - x;
}

// x = 2 x mod n over L limbs (x < n).
CG_HD void rsa_double_mod(uint32_t* x, const uint32_t* n, uint32_t L) {
  uint32_t carry = 0, borrow = 0;
  for (uint32_t i = 0; i < L; ++i) {
    const uint32_t xi = x[i];
    const uint32_t y = (xi << 1) | carry;
    carry = xi >> 31;
    x[i] = y;
    const uint64_t d = (uint64_t)y - n[i] - borrow;
    borrow = (uint32_t)(d >> 63);
  }
  if (carry || !borrow) {
    uint32_t b = 0;
    for (uint32_t i = 0; i < L; ++i) {
      const uint64_t d = (uint64_t)x[i] - n[i] - b;
      x[i] = (uint32_t)d;
      b = (uint32_t)(d >> 63);
    }
  }
}

// rr = 2^(64 L) mod n: from 2^(bits - 1) < n by doublings.
CG_HD void rsa_rr(uint32_t* rr, const uint32_t* n, uint32_t L, uint32_t bits) {
  for (uint32_t i = 0; i < RSA_MAX_LIMBS; ++i) rr[i] = 0;
  rr[(bits - 1) >> 5] = 1u << ((bits - 1) & 31u);
  const uint32_t steps = 64u * L - (bits - 1);
  for (uint32_t s = 0; s < steps; ++s) rsa_double_mod(rr, n, L);
}

// Decode + constants for one key; rec->ok says whether it was accepted.
CG_HD void rsa_key_prepare(RsaKeyRec* rec, const uint8_t* arena, uint64_t lr, uint64_t off, uint32_t len) {
  RsaKeyView v;
  rec->ok = 0;
  if (!rsa_key_decode(v, arena, lr, off, len)) return;
  rec->bits = v.bits;
  rec->L = (v.bits + 31) / 32;
  rec->k = (v.bits + 7) / 8;
  rec->em_bits = v.bits - 1;
  rec->block_len = (v.bits - 1 + 7) / 8;
  rec->e = v.e;
  for (uint32_t i = 0; i < RSA_MAX_LIMBS; ++i) rec->n[i] = rsa_be_limb(arena, lr, v.n_off, v.n_len, i);
  rec->n0inv = rsa_n0inv(rec->n[0]);
  rsa_rr(rec->rr, rec->n, rec->L, v.bits);
  rec->ok = 1;
}

// ---- scalar Montgomery arithmetic (one thread; the host tests' cross-check of the constants)
// out = a b R^-1 mod n (a, b < n); t: L + 2 limbs of scratch. out may alias a or b.
CG_HD void rsa_mont_mul_scalar(uint32_t* out, const uint32_t* a, const uint32_t* b, const RsaKeyRec* key, uint32_t* t) {
  const uint32_t L = key->L;
  const uint32_t* n = key->n;
  for (uint32_t i = 0; i < L + 2; ++i) t[i] = 0;
  for (uint32_t i = 0; i < L; ++i) {
    uint64_t c = 0;
    for (uint32_t j = 0; j < L; ++j) {
      c += (uint64_t)a[i] * b[j] + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    c += t[L];
    t[L] = (uint32_t)c;
    t[L + 1] = (uint32_t)(c >> 32);
    const uint32_t m = t[0] * key->n0inv;
    c = ((uint64_t)m * n[0] + t[0]) >> 32;
    for (uint32_t j = 1; j < L; ++j) {
      c += (uint64_t)m * n[j] + t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    c += t[L];
    t[L - 1] = (uint32_t)c;
    t[L] = t[L + 1] + (uint32_t)(c >> 32);
  }
  uint32_t borrow = 0;
  for (uint32_t i = 0; i < L; ++i) borrow = (uint32_t)(((uint64_t)t[i] - n[i] - borrow) >> 63);
  if (t[L] || !borrow) {
    uint32_t b2 = 0;
    for (uint32_t i = 0; i < L; ++i) {
      const uint64_t d = (uint64_t)t[i] - n[i] - b2;
      t[i] = (uint32_t)d;
      b2 = (uint32_t)(d >> 63);
    }
  }
  for (uint32_t i = 0; i < L; ++i) out[i] = t[i];
}

// m = s^e mod n, s < n, left-to-right square-and-multiply (all arrays RSA_MAX_LIMBS limbs).
CG_HD void rsa_modexp_scalar(uint32_t* m, const uint32_t* s, const RsaKeyRec* key) {
  uint32_t x[RSA_MAX_LIMBS], acc[RSA_MAX_LIMBS], t[RSA_MAX_LIMBS + 2];
  const uint32_t L = key->L;
  for (uint32_t i = 0; i < RSA_MAX_LIMBS; ++i) m[i] = 0;
  rsa_mont_mul_scalar(x, s, key->rr, key, t);  // s R
  for (uint32_t i = 0; i < L; ++i) acc[i] = x[i];
  int top = 31;
  while (top > 0 && !((key->e >> top) & 1u)) --top;
  for (int bit = top - 1; bit >= 0; --bit) {
    rsa_mont_mul_scalar(acc, acc, acc, key, t);
    if ((key->e >> bit) & 1u) rsa_mont_mul_scalar(acc, acc, x, key, t);
  }
  uint32_t one[RSA_MAX_LIMBS];
  for (uint32_t i = 0; i < L; ++i) one[i] = i == 0 ? 1u : 0u;
  rsa_mont_mul_scalar(m, acc, one, key, t);
}

// ---- EMSA-PSS verification (RFC 8017 9.1.2 as BC 1.57 PSSSigner.verifySignature does it;
// corda_amd/hostverify.py rsa_verify lines 77-92). `em` is the block_len-byte encoded message
// (s^e mod n, big-endian, left-padded with zeros); the check unmasks DB in place.
CG_HD uint32_t rsa_em_be32(const uint8_t* em, uint32_t pos) {
  return ((uint32_t)em[pos] << 24) | ((uint32_t)em[pos + 1] << 16) | ((uint32_t)em[pos + 2] << 8) | em[pos + 3];
}
// Trailer and minimum length (db_len >= salt + 1).
CG_HD bool rsa_pss_pre(const uint8_t* em, uint32_t block_len) {
  if (block_len < RSA_HASH_LEN + RSA_SALT_LEN + 2u) return false;
  return em[block_len - 1] == RSA_TRAILER;
}
// DB[32 c, 32 c + 32) ^= MGF1-SHA256(H) block c = SHA-256(H || BE32(c)); H = em[db_len, db_len + 32)
// is not touched, so the blocks are independent (one lane each on the device).
CG_HD void rsa_pss_unmask_block(uint8_t* em, uint32_t db_len, uint32_t c) {
  uint32_t w[16], s[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = rsa_em_be32(em, db_len + 4u * i);
  w[8] = c;
  w[9] = 0x80000000u;
#pragma unroll
  for (int i = 10; i < 15; ++i) w[i] = 0;
  w[15] = 36u * 8u;
  sha256_init(s);
  sha256_compress(s, w);
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const uint32_t pos = 32u * c + j;
    if (pos < db_len) em[pos] ^= (uint8_t)(s[j >> 2] >> (24 - 8 * (j & 3)));
  }
}
// After the unmasking: the bits of DB[0] above emBits are masked, not checked (BC 1.57; OpenSSL
// rejects them); PS must be zero, then 0x01, then the salt; SHA-256(0^8 || mhash || salt) == H.
// mhash: SHA-256(message) as 8 big-endian words.
CG_HD bool rsa_pss_post(const uint8_t* em, uint32_t block_len, uint32_t em_bits, const uint32_t mhash[8]) {
  const uint32_t db_len = block_len - RSA_HASH_LEN - 1u;
  const uint32_t ps_len = db_len - RSA_SALT_LEN - 1u;
  const uint32_t top = 0xFFu >> (8u * block_len - em_bits);
  uint32_t bad = 0;
  for (uint32_t pos = 0; pos < ps_len; ++pos) bad |= pos == 0 ? (em[0] & top) : em[pos];
  bad |= (ps_len == 0 ? (em[0] & top) : em[ps_len]) ^ 0x01u;
  if (bad) return false;
  uint32_t w[16], s[8];
  w[0] = w[1] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) w[2 + i] = mhash[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) w[10 + i] = rsa_em_be32(em, ps_len + 1u + 4u * i);
  sha256_init(s);
  sha256_compress(s, w);
  w[0] = rsa_em_be32(em, ps_len + 25u);
  w[1] = rsa_em_be32(em, ps_len + 29u);
  w[2] = 0x80000000u;
#pragma unroll
  for (int i = 3; i < 15; ++i) w[i] = 0;
  w[15] = 72u * 8u;
  sha256_compress(s, w);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= s[i] ^ rsa_em_be32(em, db_len + 4u * i);
  return diff == 0;
}
// The whole check on one thread.
CG_HD bool rsa_pss_check(uint8_t* em, uint32_t block_len, uint32_t em_bits, const uint32_t mhash[8]) {
  if (!rsa_pss_pre(em, block_len)) return false;
  const uint32_t db_len = block_len - RSA_HASH_LEN - 1u;
  for (uint32_t c = 0; 32u * c < db_len; ++c) rsa_pss_unmask_block(em, db_len, c);
  return rsa_pss_post(em, block_len, em_bits, mhash);
}

// ---- EMSA-PSS encoding (RFC 8017 9.1.1 as BC 1.57 PSSSigner.generateSignature does it, with the
// salt given; corda_amd/hostverify.py rsa_pss_sign restates it). mhash, salt and h are 8 big-endian
// words each; they are read through pointers, never indexed in registers.
// H = SHA-256(0^8 || mHash || salt)
CG_HD void rsa_pss_h(uint32_t h[8], const uint32_t* mhash, const uint32_t* salt) {
  uint32_t w[16];
  w[0] = w[1] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) w[2 + i] = mhash[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) w[10 + i] = salt[i];
  sha256_init(h);
  sha256_compress(h, w);
  w[0] = salt[6];
  w[1] = salt[7];
  w[2] = 0x80000000u;
#pragma unroll
  for (int i = 3; i < 15; ++i) w[i] = 0;
  w[15] = 72u * 8u;
  sha256_compress(h, w);
}
// Byte `pos` of PS || 01 || salt || H || BC before the masking (block_len >= 66).
CG_HD uint32_t rsa_pss_plain_byte(uint32_t pos, uint32_t block_len, const uint32_t* salt, const uint32_t* h) {
  const uint32_t db_len = block_len - RSA_HASH_LEN - 1u;
  const uint32_t ps_len = db_len - RSA_SALT_LEN - 1u;
  if (pos < ps_len) return 0u;
  if (pos == ps_len) return 1u;
  if (pos < db_len) {
    const uint32_t j = pos - ps_len - 1u;
    return (salt[j >> 2] >> (24u - 8u * (j & 3u))) & 0xffu;
  }
  if (pos < db_len + RSA_HASH_LEN) {
    const uint32_t j = pos - db_len;
    return (h[j >> 2] >> (24u - 8u * (j & 3u))) & 0xffu;
  }
  return RSA_TRAILER;
}
// The bits of EM above emBits (BC: block[0] &= 0xff >> (8 block_len - emBits))
CG_HD void rsa_pss_clear_top(uint8_t* em, uint32_t block_len, uint32_t em_bits) {
  em[0] &= (uint8_t)(0xFFu >> (8u * block_len - em_bits));
}
// The whole encoding on one thread: em[0, block_len).
CG_HD void rsa_pss_encode(uint8_t* em, uint32_t block_len, uint32_t em_bits, const uint32_t* mhash, const uint32_t* salt) {
  uint32_t h[8];
  rsa_pss_h(h, mhash, salt);
  for (uint32_t pos = 0; pos < block_len; ++pos) em[pos] = (uint8_t)rsa_pss_plain_byte(pos, block_len, salt, h);
  const uint32_t db_len = block_len - RSA_HASH_LEN - 1u;
  for (uint32_t c = 0; 32u * c < db_len; ++c) rsa_pss_unmask_block(em, db_len, c);  // its own inverse
  rsa_pss_clear_top(em, block_len, em_bits);
}
