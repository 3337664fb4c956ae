// Host build of corda_amd/csrc/rsa.h for tests/test_rsa_host.py: the key decode and Montgomery
// constants, the scalar modular exponentiation and the EMSA-PSS check, callable through ctypes; and,
// with -DHOST_RSA_MAIN, a stand-alone program that runs hr_verify over a file of vectors (so that it
// can be built with -fsanitize=address,undefined and run directly).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../corda_amd/csrc/rsa.h"

namespace {
// an aligned, padded copy: the decode reads aligned dwords up to round4(len)
struct Padded {
  std::vector<uint32_t> w;
  uint64_t lr;
  Padded(const uint8_t* p, uint32_t len) : w((len + 3) / 4 + 1, 0u), lr(((uint64_t)len + 3) & ~(uint64_t)3) {
    if (len) memcpy(w.data(), p, len);
  }
  const uint8_t* bytes() const { return (const uint8_t*)w.data(); }
};
}  // namespace

extern "C" {

uint32_t hr_rec_bytes() { return (uint32_t)sizeof(RsaKeyRec); }

// rec->ok after rsa_key_prepare (the key-prep kernel's per-key work)
int hr_key_prepare(const uint8_t* spki, uint32_t len, RsaKeyRec* rec) {
  const Padded k(spki, len);
  memset(rec, 0, sizeof *rec);
  rsa_key_prepare(rec, k.bytes(), k.lr, 0, len);
  return (int)rec->ok;
}

// bit length the decode accepts, or 0 (what cg_rsa_key_bits returns)
uint32_t hr_key_bits(const uint8_t* spki, uint32_t len) {
  const Padded k(spki, len);
  RsaKeyView v;
  return rsa_key_decode(v, k.bytes(), k.lr, 0, len) ? v.bits : 0u;
}

// m = s^e mod n as 4 L big-endian bytes; returns 0, or -1 when s >= n or sig_len > k
int hr_modexp(const RsaKeyRec* rec, const uint8_t* sig, uint32_t sig_len, uint8_t* out) {
  if (sig_len > rec->k) return -1;
  const Padded s(sig, sig_len);
  uint32_t x[RSA_MAX_LIMBS], m[RSA_MAX_LIMBS];
  for (uint32_t i = 0; i < RSA_MAX_LIMBS; ++i) x[i] = rsa_be_limb(s.bytes(), s.lr, 0, sig_len, i);
  uint32_t borrow = 0;
  for (uint32_t i = 0; i < RSA_MAX_LIMBS; ++i) borrow = (uint32_t)(((uint64_t)x[i] - rec->n[i] - borrow) >> 63);
  if (!borrow) return -1;
  rsa_modexp_scalar(m, x, rec);
  for (uint32_t i = 0; i < rec->L; ++i)
    for (int b = 0; b < 4; ++b) out[4 * rec->L - 1 - (4 * i + b)] = (uint8_t)(m[i] >> (8 * b));
  return 0;
}

// rsa_pss_check over a copy of em; mhash: the 32 digest bytes
int hr_pss_check(const uint8_t* em, uint32_t block_len, uint32_t em_bits, const uint8_t* mhash) {
  std::vector<uint8_t> e(em, em + block_len);
  uint32_t mh[8];
  for (int i = 0; i < 8; ++i) mh[i] = rsa_em_be32(mhash, 4u * i);
  return rsa_pss_check(e.data(), block_len, em_bits, mh) ? 1 : 0;
}

// The whole verification as the kernels do it, on one thread: -1 key not accepted, 1 valid, 0 invalid.
int hr_verify(const uint8_t* spki, uint32_t klen, const uint8_t* sig, uint32_t sig_len, const uint8_t* msg,
              uint32_t msg_len) {
  static RsaKeyRec rec;
  if (!hr_key_prepare(spki, klen, &rec)) return -1;
  std::vector<uint8_t> m(4 * rec.L);
  if (hr_modexp(&rec, sig, sig_len, m.data()) != 0) return 0;
  const uint32_t extra = 4 * rec.L - rec.block_len;
  for (uint32_t i = 0; i < extra; ++i)
    if (m[i]) return 0;  // does not fit the emBits block
  const Padded p(msg, msg_len);
  uint32_t mh[8];
  sha256_arena_suffix(mh, p.bytes(), p.lr, 0, msg_len, nullptr);
  return rsa_pss_check(m.data() + extra, rec.block_len, rec.em_bits, mh) ? 1 : 0;
}

}  // extern "C"

#ifdef HOST_RSA_MAIN
// vectors: [u32 klen][u32 slen][u32 mlen][i32 want][key][sig][msg] ...; exit status 0 when all agree
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t h[4];
  int n = 0, bad = 0;
  while (fread(h, 4, 4, f) == 4) {
    std::vector<uint8_t> k(h[0]), s(h[1]), m(h[2]);
    if ((h[0] && fread(k.data(), 1, h[0], f) != h[0]) || (h[1] && fread(s.data(), 1, h[1], f) != h[1]) ||
        (h[2] && fread(m.data(), 1, h[2], f) != h[2]))
      return 2;
    const int got = hr_verify(k.data(), h[0], s.data(), h[1], m.data(), h[2]);
    if (got != (int)h[3]) {
      printf("vector %d: got %d want %d\n", n, got, (int)h[3]);
      ++bad;
    }
    ++n;
  }
  fclose(f);
  printf("%d vectors, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}
#endif
