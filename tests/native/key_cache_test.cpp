// CPU test of corda_amd/csrc/key_cache.h: the wide-table cache's index, probe, claim and commit
// functions, the same code the device kernels call (verify.hip k_kc_begin, k_key_classify,
// k_kc_claim, k_kc_commit), driven through random call sequences against a plain dictionary.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -o key_cache_test key_cache_test.cpp && ./key_cache_test
// Prints "ok" and exits 0, or the first broken invariant and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../corda_amd/csrc/key_cache.h"

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
      exit(1);                                             \
    }                                                      \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // [0, n)
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((g_rng >> 33) % (n ? n : 1));
}

// A key of the test: where it lies in the arena, and its identity as the dictionary sees it
// (scheme, format and bytes, spelled out: nothing of the header's hashing or packing).
struct TKey {
  uint32_t scheme, fmt, len;
  uint64_t off;
  bool decodes;
  std::string id;
};

struct Arena {
  std::vector<uint8_t> bytes;
  uint64_t len = 0;  // the logical length; the buffer is rounded up to 4 like every arena
  uint64_t put(const std::vector<uint8_t>& b, uint32_t misalign) {
    while (bytes.size() % 4 != misalign % 4) bytes.push_back(0xEE);
    const uint64_t off = bytes.size();
    bytes.insert(bytes.end(), b.begin(), b.end());
    return off;
  }
  void seal() {
    len = bytes.size();
    while (bytes.size() % 4) bytes.push_back(0x77);  // past the arena's end: must read as 0
  }
};

static TKey make_key(Arena& a, uint32_t scheme, uint32_t fmt, const std::vector<uint8_t>& b, bool decodes) {
  TKey k;
  k.scheme = scheme;
  k.fmt = fmt;
  k.len = (uint32_t)b.size();
  k.off = a.put(b, rnd(4));
  k.decodes = decodes;
  k.id = std::string(1, (char)scheme) + std::string(1, (char)fmt) + std::string(b.begin(), b.end());
  return k;
}

struct Cache {
  uint32_t slots, size, bits;
  std::vector<KcOwner> owners;
  std::vector<uint32_t> live, freel, index;
  Cache(uint32_t s, uint32_t b) : slots(s), size(kc_index_size(s)), bits(b), owners(s), live(s, 7), freel(s, 0xdead), index(size, 0xdead) {
    for (KcOwner& o : owners) memset(&o, 0xAB, sizeof o);  // fresh device memory holds anything
  }
};

struct CallResult {
  std::vector<uint32_t> slot;  // per key of the call: its slot or KC_NONE (full tables)
  uint32_t hits = 0, claimed = 0, built = 0, evicted = 0, fell_back = 0;
};

// One call, in the kernels' order. model: identity -> the slots that hold its complete tables.
static CallResult run_call(Cache& c, std::map<std::string, std::set<uint32_t>>& model, const Arena& a,
                           const std::vector<TKey>& keys, uint32_t cap, uint32_t parts, bool dirty, bool commit) {
  CallResult r;
  r.slot.assign(keys.size(), KC_NONE);
  // k_kc_begin
  if (dirty) model.clear();
  for (uint32_t b = 0; b < c.size; ++b) c.index[b] = 0;
  for (uint32_t s = 0; s < c.slots; ++s) {
    const bool valid = kc_begin_slot(c.owners.data(), c.live.data(), s, dirty);
    CHECK(!dirty || !valid, "slot %u valid after dirty", s);
    CHECK(c.owners[s].state == KC_VALID || c.owners[s].state == KC_EMPTY, "slot %u state %u after begin", s, c.owners[s].state);
  }
  for (uint32_t s = 0; s < c.slots; ++s)
    if (c.owners[s].state == KC_VALID) CHECK(kc_index_insert(c.index.data(), c.size, c.bits, c.owners.data(), s), "index full");
  // the model and the owners agree on what is valid
  uint32_t n_valid = 0, n_model = 0;
  for (uint32_t s = 0; s < c.slots; ++s) n_valid += c.owners[s].state == KC_VALID;
  for (auto& kv : model) n_model += (uint32_t)kv.second.size();
  CHECK(n_valid == n_model, "%u valid owners, the model holds %u", n_valid, n_model);
  // k_key_classify: the first `cap` keys may be wide
  std::vector<uint32_t> miss;
  std::vector<KcKey> kk(keys.size());
  for (uint32_t i = 0; i < keys.size(); ++i) {
    kc_key_load(kk[i], keys[i].scheme, keys[i].fmt, keys[i].len, a.bytes.data(), a.len, keys[i].off);
    if (i >= cap) {
      ++r.fell_back;
      continue;
    }
    const uint32_t hit = kc_probe(c.index.data(), c.size, c.bits, c.owners.data(), kk[i]);
    const auto m = model.find(keys[i].id);
    if (hit == KC_NONE) {
      CHECK(m == model.end(), "key %u is cached but missed", i);
      miss.push_back(i);
      continue;
    }
    CHECK(hit < c.slots, "hit slot %u out of range", hit);
    CHECK(m != model.end() && m->second.count(hit), "key %u hit slot %u, which the model does not give it", i, hit);
    const KcOwner& o = c.owners[hit];
    CHECK(o.state == KC_VALID, "hit on a slot in state %u", o.state);
    CHECK((o.key.tag & 0xff) == keys[i].scheme && ((o.key.tag >> 8) & 0xff) == keys[i].fmt && (o.key.tag >> 16) == keys[i].len,
          "hit owner's tag differs");
    CHECK(memcmp(o.key.bytes, a.bytes.data() + keys[i].off, keys[i].len) == 0, "hit owner's bytes differ from the key's");
    c.live[hit] = 1;
    r.slot[i] = hit;
    ++r.hits;
  }
  // k_kc_claim: the free list by `parts` workers, then the r-th miss takes the r-th entry
  std::vector<uint32_t> cnt(2 * parts);
  for (uint32_t t = 0; t < parts; ++t) kc_free_count(c.owners.data(), c.live.data(), c.slots, t, parts, &cnt[2 * t]);
  uint32_t tot0 = 0, tot1 = 0;
  for (uint32_t t = 0; t < parts; ++t) tot0 += cnt[2 * t], tot1 += cnt[2 * t + 1];
  uint32_t b0 = 0, b1 = tot0;
  for (uint32_t t = 0; t < parts; ++t) {
    kc_free_fill(c.owners.data(), c.live.data(), c.slots, t, parts, b0, b1, c.freel.data());
    b0 += cnt[2 * t];
    b1 += cnt[2 * t + 1];
  }
  const uint32_t nfree = tot0 + tot1;
  uint32_t n_live = 0;
  for (uint32_t s = 0; s < c.slots; ++s) n_live += c.live[s] != 0;
  CHECK(nfree == c.slots - n_live, "%u claimable of %u slots with %u live", nfree, c.slots, n_live);
  for (uint32_t q = 0; q + 1 < nfree; ++q)  // empty slots before valid ones
    CHECK(!(c.owners[c.freel[q]].state == KC_VALID && c.owners[c.freel[q + 1]].state != KC_VALID), "a valid slot listed before an empty one");
  std::set<uint32_t> taken;
  for (uint32_t q = 0; q < miss.size(); ++q) {
    const uint32_t i = miss[q];
    bool ev;
    const uint32_t s = kc_claim(c.owners.data(), c.freel.data(), nfree, q, kk[i], &ev);
    if (s == KC_NONE) {
      CHECK(q >= nfree, "miss %u of %u claimable got no slot", q, nfree);
      ++r.fell_back;
      continue;
    }
    CHECK(s < c.slots && !c.live[s], "claimed slot %u was hit in this call", s);
    CHECK(taken.insert(s).second, "slot %u claimed twice", s);
    CHECK(c.owners[s].state == KC_PENDING, "claimed slot not pending");
    for (auto it = model.begin(); it != model.end();) {  // whoever held it is gone
      const bool had = it->second.erase(s) != 0;
      CHECK(had == false || ev, "eviction not reported");
      it = it->second.empty() ? model.erase(it) : ++it;
    }
    r.evicted += ev;
    r.slot[i] = s;
    ++r.claimed;
  }
  // with the hot keys within the capacity, every one of them has a slot
  if (keys.size() <= cap && cap <= c.slots)
    for (uint32_t i = 0; i < keys.size(); ++i) CHECK(r.slot[i] != KC_NONE, "key %u of %zu hot keys got no slot (cap %u)", i, keys.size(), cap);
  // two keys share a slot only if scheme and bytes are equal
  for (uint32_t i = 0; i < keys.size(); ++i)
    for (uint32_t j = 0; j < i; ++j)
      if (r.slot[i] != KC_NONE && r.slot[i] == r.slot[j]) CHECK(keys[i].id == keys[j].id, "keys %u and %u share slot %u", j, i, r.slot[i]);
  // a pending owner is no hit, even for its own key and even if something entered it in the index
  for (uint32_t q = 0; q < miss.size(); ++q)
    if (r.slot[miss[q]] != KC_NONE && kk[miss[q]].tag) {
      const uint32_t s = r.slot[miss[q]];
      std::vector<uint32_t> idx2(c.index);
      uint32_t b = kc_home(kk[miss[q]].hash, c.bits, c.size);
      while (idx2[b]) b = (b + 1) & (c.size - 1);
      idx2[b] = s + 1;
      const uint32_t hit = kc_probe(idx2.data(), c.size, c.bits, c.owners.data(), kk[miss[q]]);
      CHECK(hit == KC_NONE || (hit != s && c.owners[hit].state == KC_VALID), "a pending owner produced a hit");
    }
  // the builds, then k_kc_commit (a failed call never gets here)
  if (commit)
    for (uint32_t q = 0; q < miss.size(); ++q) {
      const uint32_t i = miss[q], s = r.slot[i];
      if (s == KC_NONE) continue;
      const bool ok = kc_commit(c.owners.data(), s, keys[i].decodes);
      CHECK(ok == (keys[i].decodes && kk[i].tag != 0), "commit of key %u", i);
      CHECK(c.owners[s].state == (ok ? KC_VALID : KC_EMPTY), "state after commit");
      if (ok) model[keys[i].id].insert(s), ++r.built;
      CHECK(!kc_commit(c.owners.data(), s, true), "a second commit changed a slot");
    }
  return r;
}

int main() {
  // identities: equal bytes under another scheme, format or length are other keys; one key does not
  // decode; one is longer than an owner record (never cached); offsets of every alignment; the last
  // key ends at the arena's end, so its tail word runs past it
  Arena a;
  std::vector<TKey> pool;
  std::vector<uint8_t> base(32);
  for (int n = 0; n < 40; ++n) {
    for (auto& b : base) b = (uint8_t)rnd(256);
    pool.push_back(make_key(a, 4, 0, base, n % 7 != 3));
    if (n % 5 == 0) pool.push_back(make_key(a, 3, 0, base, true));  // same bytes, another scheme
    if (n % 5 == 1) pool.push_back(make_key(a, 4, 1, base, true));  // same bytes, another format
    if (n % 5 == 2) {  // a prefix of the same bytes: another length
      std::vector<uint8_t> sh(base.begin(), base.begin() + 31);
      pool.push_back(make_key(a, 4, 0, sh, true));
    }
    if (n % 9 == 0) {  // 91-byte keys that differ in the last byte only
      std::vector<uint8_t> spki(91, (uint8_t)n);
      pool.push_back(make_key(a, 3, 1, spki, true));
      spki[90] ^= 1;
      pool.push_back(make_key(a, 3, 1, spki, true));
    }
  }
  pool.push_back(make_key(a, 2, 1, std::vector<uint8_t>(97, 0x42), true));  // too long: not cacheable
  pool.push_back(make_key(a, 2, 2, std::vector<uint8_t>(33, 0x99), true));  // ends with the arena
  a.seal();
  {
    KcKey k;
    const TKey& last = pool.back();
    kc_key_load(k, last.scheme, last.fmt, last.len, a.bytes.data(), a.len, last.off);
    CHECK(k.tag != 0 && k.bytes[8] == 0x99u, "the tail word past the key's and the arena's end reads as 0, got %08x", k.bytes[8]);
    kc_key_load(k, 2, 2, 33, a.bytes.data(), a.len, a.len - 32);  // runs past the arena: not cacheable
    CHECK(k.tag == 0, "a key outside the arena got a tag");
    kc_key_load(k, 2, 1, 97, a.bytes.data(), a.len, pool[pool.size() - 2].off);
    CHECK(k.tag == 0, "a key longer than an owner record got a tag");
  }

  {
    // a hash match alone is never a hit: one valid owner, probed with keys that were given its hash
    // but differ in scheme, in format, in length, or in one byte
    Cache c(4, 32);
    std::map<std::string, std::set<uint32_t>> model;
    std::vector<TKey> one(1, pool[0]);
    run_call(c, model, a, one, 4, 1, true, true);
    run_call(c, model, a, one, 4, 1, false, true);  // index rebuilt over the valid owner
    KcKey own;
    kc_key_load(own, pool[0].scheme, pool[0].fmt, pool[0].len, a.bytes.data(), a.len, pool[0].off);
    CHECK(kc_probe(c.index.data(), c.size, c.bits, c.owners.data(), own) != KC_NONE, "the owner's own key missed");
    for (int v = 0; v < 4; ++v) {
      KcKey k = own;
      if (v == 0) k.tag = (k.tag & ~0xffu) | 3u;
      if (v == 1) k.tag ^= 1u << 8;
      if (v == 2) k.tag -= 1u << 16;
      if (v == 3) k.bytes[7] ^= 0x01000000u;
      CHECK(!kc_key_equal(k, own) && !kc_key_equal(own, k), "variant %d compares equal", v);
      CHECK(kc_probe(c.index.data(), c.size, c.bits, c.owners.data(), k) == KC_NONE, "variant %d hit on the hash alone", v);
    }
  }

  const uint32_t slot_counts[] = {1, 3, 8, 13, 64};
  uint64_t calls = 0, hits = 0, evictions = 0, fallbacks = 0;
  for (uint32_t slots : slot_counts)
    for (uint32_t bits : {32u, 1u, 0u}) {  // the whole index, two home entries, one
      Cache c(slots, bits);
      std::map<std::string, std::set<uint32_t>> model;
      std::vector<TKey> prev;
      bool dirty = true, open = false;  // the host's flags (cordagpu.cpp kc_dirty / kc_open)
      for (int step = 0; step < 400; ++step) {
        // the next call's hot keys: the last call's again, a shrunk or overlapping set, a fresh one,
        // more than the slots hold, with duplicate rows
        std::vector<TKey> keys;
        const uint32_t kind = rnd(6);
        if (kind == 0 || prev.empty()) {
          const uint32_t n = 1 + rnd(2 * slots + 2);
          for (uint32_t i = 0; i < n; ++i) keys.push_back(pool[rnd((uint32_t)pool.size())]);
        } else if (kind == 1) {
          keys = prev;
        } else if (kind == 2) {  // shrinks
          for (const TKey& k : prev)
            if (rnd(2)) keys.push_back(k);
          if (keys.empty()) keys.push_back(prev[0]);
        } else if (kind == 3) {  // overlaps
          for (const TKey& k : prev) keys.push_back(rnd(3) ? k : pool[rnd((uint32_t)pool.size())]);
        } else if (kind == 4) {  // permuted, with a duplicate row
          keys = prev;
          for (size_t i = keys.size(); i > 1; --i) std::swap(keys[i - 1], keys[rnd((uint32_t)i)]);
          keys.push_back(keys[rnd((uint32_t)keys.size())]);
        } else {  // exceeds the capacity
          for (uint32_t i = 0; i < slots + 1 + rnd(4); ++i) keys.push_back(pool[(i * 7 + step) % pool.size()]);
        }
        const uint32_t cap = rnd(4) ? slots : 1 + rnd(slots);  // the call's cap: at most the slots
        const uint32_t parts = rnd(3) == 0 ? 1 : rnd(2) ? 1024 : 1 + rnd(2 * slots);
        const bool fail = rnd(10) == 0;  // the call ends between claim and commit
        if (open) dirty = true;
        open = true;
        const bool was_dirty = dirty;
        const CallResult r = run_call(c, model, a, keys, cap, parts, dirty, !fail);
        dirty = false;
        if (!fail) open = false;
        if (was_dirty) {
          CHECK(r.hits == 0 && r.evicted == 0, "hits %u / evictions %u in a call on an emptied cache", r.hits, r.evicted);
        }
        ++calls, hits += r.hits, evictions += r.evicted, fallbacks += r.fell_back;
        prev = keys;
      }
      // the same keys twice in a row, nothing failing: the second call builds nothing
      std::vector<TKey> keys;
      for (uint32_t i = 0; i < slots; ++i) keys.push_back(pool[i]);
      run_call(c, model, a, keys, slots, 4, open, true);
      const CallResult r1 = run_call(c, model, a, keys, slots, 4, false, true);
      CHECK(r1.built == 0 && r1.evicted == 0, "a repeated call built %u and evicted %u", r1.built, r1.evicted);
      uint32_t cacheable = 0;
      for (const TKey& k : keys) cacheable += k.decodes && k.len <= 4 * KC_KEY_WORDS;
      CHECK(r1.hits == cacheable, "a repeated call hit %u of %u keys", r1.hits, cacheable);
      // and after "dirty" the cache is empty
      const CallResult r2 = run_call(c, model, a, keys, slots, 4, true, true);
      CHECK(r2.hits == 0 && r2.claimed == slots && r2.evicted == 0, "after dirty: hits %u, claimed %u, evicted %u", r2.hits, r2.claimed, r2.evicted);
    }
  CHECK(hits > 1000 && evictions > 100 && fallbacks > 100, "the sequences reached too little: %llu hits, %llu evictions, %llu fallbacks",
        (unsigned long long)hits, (unsigned long long)evictions, (unsigned long long)fallbacks);
  printf("ok: %llu calls, %llu hits, %llu evictions, %llu fallbacks\n", (unsigned long long)calls, (unsigned long long)hits,
         (unsigned long long)evictions, (unsigned long long)fallbacks);
  return 0;
}
