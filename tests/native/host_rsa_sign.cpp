// Stand-alone host program over the HIP-free EMSA-PSS encode of corda_amd/csrc/rsa.h (rsa_pss_h,
// rsa_pss_plain_byte, rsa_pss_unmask_block, rsa_pss_clear_top: the code k_rsa_sign_prep and k_rsa_sign run)
// for tests/test_rsa_sign_host.py. It reads vectors from the file named on its command line, each
//   u32 bits | 32 bytes SHA-256(message) | 32 bytes salt | block_len bytes of the expected EM
// (little-endian u32; block_len = ceil((bits - 1) / 8)), encodes each one into a heap buffer of exactly
// block_len bytes (so a sanitizer build sees any byte written or read outside it), checks that the
// verifier's rsa_pss_check accepts the result, and prints "<n> vectors, <m> mismatches". Exit status 0
// only when m is 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../corda_amd/csrc/rsa.h"

static uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s vectors.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  unsigned n = 0, bad = 0;
  for (;;) {
    uint32_t bits;
    uint8_t mh[32], salt[32];
    if (fread(&bits, 4, 1, f) != 1) break;
    if (bits < RSA_MIN_BITS || bits > RSA_MAX_BITS || fread(mh, 32, 1, f) != 1 || fread(salt, 32, 1, f) != 1) {
      fprintf(stderr, "malformed vector %u\n", n);
      return 2;
    }
    const uint32_t em_bits = bits - 1, block_len = (em_bits + 7) / 8;
    std::vector<uint8_t> want(block_len);
    if (fread(want.data(), 1, block_len, f) != block_len) {
      fprintf(stderr, "truncated vector %u\n", n);
      return 2;
    }
    uint32_t mhw[8], sw[8];
    for (int i = 0; i < 8; ++i) {
      mhw[i] = be32(mh + 4 * i);
      sw[i] = be32(salt + 4 * i);
    }
    uint8_t* em = (uint8_t*)malloc(block_len);  // exactly block_len bytes
    memset(em, 0xA5, block_len);
    rsa_pss_encode(em, block_len, em_bits, mhw, sw);
    bool ok = memcmp(em, want.data(), block_len) == 0;
    if (ok) ok = rsa_pss_check(em, block_len, em_bits, mhw);  // unmasks in place
    free(em);
    if (!ok) {
      ++bad;
      printf("vector %u (%u bits): mismatch\n", n, bits);
    }
    ++n;
  }
  fclose(f);
  printf("%u vectors, %u mismatches\n", n, bad);
  return bad == 0 && n > 0 ? 0 : 1;
}
