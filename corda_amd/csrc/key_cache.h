// The per-context cache of wide tables: which wide-pool slot holds the tables of which public key.
//
// A wide table (keyws.h EdWideSlot / EcWideSlot) depends only on the key's bytes and the context's
// radix, and a hot key of one call is overwhelmingly a hot key of the next (a notary's identity key),
// so a context keeps the slots' contents between calls and a call builds only the tables of the keys
// it does not find. This header is the bookkeeping, as functions over plain arrays that run on the
// device (verify.hip: k_kc_begin, k_key_classify, k_kc_claim, the k_*_kc_commit kernels) and on the
// CPU (tests/native/key_cache_test.cpp drives the same functions against a dictionary):
//   owners   per slot: whose tables it holds (scheme, format, length, bytes) and a state
//   index    open addressing (linear probing) over the VALID owners, rebuilt at the start of a call;
//            an entry is a slot + 1, 0 is free. A probe ends at a free entry. A hit is a full
//            compare of tag and bytes against the owner: the hash only picks where to look
//   live     per slot: some key of this call hit it (the claim pass must leave it alone)
// One call: kc_begin_slot for every slot, kc_index_insert for every VALID one; kc_probe per
// wide-eligible key (a hit marks the slot live); kc_free_count / kc_free_fill list the slots that are
// not live, EMPTY ones first; kc_claim hands the r-th of them to the r-th miss (owner PENDING);
// the builds run; kc_commit turns PENDING into VALID (or EMPTY: the key did not decode).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KC_HD __host__ __device__ inline
#else
#define KC_HD static inline
#endif

#define KC_KEY_WORDS 24u  // 96 bytes: the longest key any decode accepts is 91 (an EC SubjectPublicKeyInfo)
#define KC_EMPTY 0u
#define KC_PENDING 1u  // claimed by this call, tables not built yet: never a hit
#define KC_VALID 2u
#define KC_NONE 0xffffffffu

struct KcKey {
  uint32_t tag;   // scheme | fmt << 8 | len << 16; 0: not cacheable (longer than KC_KEY_WORDS words)
  uint32_t hash;
  uint32_t bytes[KC_KEY_WORDS];  // the key's len bytes, zero-filled
};
struct KcOwner {
  uint32_t state;
  uint32_t pad;
  KcKey key;
};

// 4 little-endian bytes at arena[off, off + 4) by aligned loads; bytes at or past len_rounded (the
// arena length rounded up to 4) read as 0 (sha2.h cg_ld_bytes4: what the decode kernels read)
KC_HD uint32_t kc_ld4(const uint8_t* arena, uint64_t len_rounded, uint64_t off) {
  const uint64_t a0 = off & ~(uint64_t)3;
  const uint32_t sh = (uint32_t)(off & 3) * 8u;
  const uint32_t w0 = a0 < len_rounded ? *(const uint32_t*)(arena + a0) : 0u;
  if (sh == 0) return w0;
  const uint32_t w1 = (a0 + 4) < len_rounded ? *(const uint32_t*)(arena + a0 + 4) : 0u;
  return (w0 >> sh) | (w1 << (32u - sh));
}

// The identity of key (scheme, fmt, len, arena[off, off + len)): exactly what the decode kernels
// consume. A key outside the arena or longer than the owner record is not cacheable (tag 0): no
// decode accepts it, and it never produces a hit.
KC_HD void kc_key_load(KcKey& k, uint32_t scheme, uint32_t fmt, uint32_t len, const uint8_t* arena, uint64_t arena_len,
                       uint64_t off) {
  const bool ok = len != 0 && len <= 4u * KC_KEY_WORDS && off <= arena_len && len <= arena_len - off;
  k.tag = ok ? (scheme & 0xffu) | (fmt & 0xffu) << 8 | len << 16 : 0u;
  const uint64_t lr = (arena_len + 3) & ~(uint64_t)3;
  uint32_t h = 0x811c9dc5u ^ k.tag;
  for (uint32_t w = 0; w < KC_KEY_WORDS; ++w) {
    uint32_t v = 0;
    if (ok && 4u * w < len) {
      v = kc_ld4(arena, lr, off + 4u * w);
      if (len - 4u * w < 4u) v &= (1u << (8u * (len - 4u * w))) - 1u;
    }
    k.bytes[w] = v;
    h = (h ^ v) * 0x01000193u;
    h ^= h >> 15;
  }
  k.hash = h;
}

KC_HD bool kc_key_equal(const KcKey& a, const KcKey& b) {
  if (a.tag != b.tag || a.tag == 0u) return false;
  uint32_t d = 0;
  for (uint32_t w = 0; w < KC_KEY_WORDS; ++w) d |= a.bytes[w] ^ b.bytes[w];
  return d == 0;
}

// Entries of the index for `slots` slots: a power of two, at least twice the slots, so a probe
// always meets a free entry.
KC_HD uint32_t kc_index_size(uint32_t slots) {
  uint32_t t = 16;
  while (t < 2u * slots) t <<= 1;
  return t;
}
// Home entry of a hash: its low `bits` bits (the whole index unless a test narrows it, so that
// keys collide; bits 0 = one home for every key).
KC_HD uint32_t kc_home(uint32_t hash, uint32_t bits, uint32_t size) {
  const uint32_t m = bits >= 32u ? 0xffffffffu : (1u << bits) - 1u;
  return hash & m & (size - 1u);
}

// Start of a call. A slot whose tables are not known to be complete is EMPTY again: a PENDING
// owner (the call that claimed it ended before its commit), and every slot after `dirty` (a call
// failed between claim and commit, or the pool moved). Returns whether the slot is VALID.
KC_HD bool kc_begin_slot(KcOwner* owners, uint32_t* live, uint32_t s, bool dirty) {
  if (dirty || owners[s].state != KC_VALID) owners[s].state = KC_EMPTY;
  live[s] = 0;
  return owners[s].state == KC_VALID;
}

// compare-and-swap of one index entry: atomic on the device (every VALID slot inserts at once)
KC_HD uint32_t kc_cas(uint32_t* p, uint32_t expect, uint32_t val) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expect, val);
#else
  const uint32_t old = *p;
  if (old == expect) *p = val;
  return old;
#endif
}

// Enter VALID slot s (the index was cleared before). False only if the index is full, which
// kc_index_size rules out.
KC_HD bool kc_index_insert(uint32_t* index, uint32_t size, uint32_t bits, const KcOwner* owners, uint32_t s) {
  uint32_t b = kc_home(owners[s].key.hash, bits, size);
  for (uint32_t n = 0; n < size; ++n, b = (b + 1u) & (size - 1u))
    if (kc_cas(&index[b], 0u, s + 1u) == 0u) return true;
  return false;
}

// The slot that holds `k`'s tables, or KC_NONE. Only a VALID owner with equal tag and bytes is a hit.
KC_HD uint32_t kc_probe(const uint32_t* index, uint32_t size, uint32_t bits, const KcOwner* owners, const KcKey& k) {
  if (k.tag == 0u) return KC_NONE;
  uint32_t b = kc_home(k.hash, bits, size);
  for (uint32_t n = 0; n < size; ++n, b = (b + 1u) & (size - 1u)) {
    const uint32_t e = index[b];
    if (e == 0u) return KC_NONE;
    const KcOwner& o = owners[e - 1u];
    if (o.state == KC_VALID && o.key.hash == k.hash && kc_key_equal(o.key, k)) return e - 1u;
  }
  return KC_NONE;
}

// The claimable slots, listed by `parts` workers that each take a contiguous share of the slots:
// kc_free_count gives part t's number of EMPTY (cnt[0]) and of VALID (cnt[1]) slots that are not
// live; with base0 / base1 = the exclusive sums of those over the parts before t, base1 offset by the
// total of cnt[0], kc_free_fill writes part t's slots: EMPTY ones first overall, so a call evicts a
// key's tables only when no empty slot is left.
KC_HD void kc_part(uint32_t slots, uint32_t t, uint32_t parts, uint32_t& lo, uint32_t& hi) {
  const uint32_t per = (slots + parts - 1u) / parts;
  lo = t * per < slots ? t * per : slots;
  hi = lo + per < slots ? lo + per : slots;
}
KC_HD void kc_free_count(const KcOwner* owners, const uint32_t* live, uint32_t slots, uint32_t t, uint32_t parts,
                         uint32_t cnt[2]) {
  uint32_t lo, hi;
  kc_part(slots, t, parts, lo, hi);
  cnt[0] = cnt[1] = 0;
  for (uint32_t s = lo; s < hi; ++s)
    if (!live[s]) ++cnt[owners[s].state == KC_VALID ? 1 : 0];
}
KC_HD void kc_free_fill(const KcOwner* owners, const uint32_t* live, uint32_t slots, uint32_t t, uint32_t parts,
                        uint32_t base0, uint32_t base1, uint32_t* freelist) {
  uint32_t lo, hi;
  kc_part(slots, t, parts, lo, hi);
  for (uint32_t s = lo; s < hi; ++s)
    if (!live[s]) freelist[owners[s].state == KC_VALID ? base1++ : base0++] = s;
}

// The r-th miss of a call takes the r-th claimable slot: its owner becomes `k`, PENDING. Returns
// the slot, or KC_NONE when the call has more misses than claimable slots (the key then takes full
// tables); *evicted = the slot held another key's complete tables.
KC_HD uint32_t kc_claim(KcOwner* owners, const uint32_t* freelist, uint32_t nfree, uint32_t r, const KcKey& k,
                        bool* evicted) {
  *evicted = false;
  if (r >= nfree) return KC_NONE;
  const uint32_t s = freelist[r];
  *evicted = owners[s].state == KC_VALID;
  owners[s].state = KC_PENDING;
  owners[s].key = k;
  return s;
}

// After the slot's tables are built: `decoded` = the key decoded (its tables exist). A key that
// did not decode, or is not cacheable, leaves the slot EMPTY. Returns whether the slot became VALID.
KC_HD bool kc_commit(KcOwner* owners, uint32_t s, bool decoded) {
  if (owners[s].state != KC_PENDING) return false;
  const bool ok = decoded && owners[s].key.tag != 0u;
  owners[s].state = ok ? KC_VALID : KC_EMPTY;
  return ok;
}
