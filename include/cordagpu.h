/* cordagpu.h — C ABI of the MI355X batch signature-verification engine for Corda.
 *
 * This is the drop-in boundary. Every entry point is plain C: pointers,
 * sizes and status bytes; no torch, HIP or C++ types. A JVM binds it with JNI / Panama
 * (INTEGRATION.md), Python with ctypes (corda_amd/_lib.py).
 *
 * What each entry point replaces in the reference (paths relative to the Corda tree):
 *
 *   cg_verify_batch      N x Crypto.isValid / Crypto.doVerify(scheme, publicKey, sig, clear)
 *                        core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:474-484 (doVerify)
 *                        and :553-559 (isValid -> JCA Signature.initVerify/update/verify into
 *                        i2p EdDSAEngine / BouncyCastle SHA256withECDSA). Serial callers:
 *                        TransactionWithSignatures.checkSignaturesAreValid
 *                        (core/.../transactions/TransactionWithSignatures.kt:58-62).
 *   cg_verify_batch_device  the same, with every buffer already resident in HBM (verifier
 *                        process / bench: no PCIe in the timed region).
 *   cg_sha256_batch      N x SecureHash.sha256(bytes)   core/.../crypto/SecureHash.kt:37
 *   cg_sha512_batch      N x SHA-512 (the EdDSA challenge digest, i2p engine)
 *   cg_tx_ids            N x WireTransaction.id = MerkleTree.getMerkleTree(
 *                        availableComponentHashes).hash  core/.../transactions/WireTransaction.kt:39,104,
 *                        MerkleTransaction.kt:16-33,74-93, core/.../crypto/MerkleTree.kt:27-66
 *   cg_merkle_roots      N x MerkleTree.getMerkleTree(leaves).hash  MerkleTree.kt:27-66
 *
 * Status bytes never collapse to "valid": an item the engine did not run is CG_NOT_RUN.
 * Ownership: the caller owns every buffer; the library copies what it needs and keeps no
 * pointer after a call returns. Threading: a cg_ctx serialises its own calls internally;
 * distinct contexts (one per GPU) run concurrently.
 */
#ifndef CORDAGPU_H
#define CORDAGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CG_ABI_VERSION 2

/* Corda SignatureScheme.schemeNumberID (Crypto.kt:78-184). Others => CG_UNSUPPORTED.
 * CG_RSA_SHA256 (BouncyCastle SHA256WITHRSAANDMGF1: RSASSA-PSS, SHA-256, MGF1-SHA256, 32-byte salt,
 * trailer 0xBC) is CG_UNSUPPORTED too unless the context was opened with CG_FLAG_RSA. With the flag
 * an item gets a verdict when its key is CG_KEY_SPKI and the device decode accepts it: canonical DER
 * SubjectPublicKeyInfo { AlgorithmIdentifier { rsaEncryption 1.2.840.113549.1.1.1, parameters absent
 * or NULL }, BIT STRING with 0 unused bits { RSAPublicKey { n, e } } }, every length minimal, no
 * trailing bytes, all inside cg_key.len, both INTEGERs minimal and positive, n odd with
 * 1024 <= bitlen(n) <= 4096 (any bit length), 1 <= e < 2^32. Every other RSA key (BER forms, other
 * sizes, even n, larger e, another fmt) stays CG_UNSUPPORTED, so the caller's host fallback decides
 * it with the reference's own exception: the engine gives a verdict only for keys it has parsed fully
 * and strictly. cg_rsa_key_bits tells which keys those are. */
enum {
  CG_RSA_SHA256 = 1,
  CG_ECDSA_SECP256K1_SHA256 = 2,
  CG_ECDSA_SECP256R1_SHA256 = 3,
  CG_EDDSA_ED25519_SHA512 = 4,
  CG_SPHINCS256_SHA256 = 5,
  CG_COMPOSITE_KEY = 6
};

/* Public-key byte formats. */
enum {
  CG_KEY_RAW = 0,  /* Ed25519: 32-byte A (what Kryo writes, Kryo.kt:333); ECDSA: 64-byte X||Y big-endian */
  CG_KEY_SPKI = 1, /* X.509 SubjectPublicKeyInfo DER == PublicKey.getEncoded() (44 / 91 / 88 bytes);
                      also the other forms Crypto.decodePublicKey (Crypto.kt:321-325) accepts:
                      Ed25519 with NULL parameters (46), EC around a compressed point (59 / 56)
                      or a hybrid one (06/07 tag, 91 / 88). Anything else: CG_KEY_INVALID. */
  CG_KEY_SEC1 = 2  /* ECDSA only: 04||X||Y, 06/07||X||Y (hybrid) or 02/03||X */
};

/* Per-item verdicts. */
enum {
  CG_VALID = 0,         /* isValid == true */
  CG_INVALID = 1,       /* isValid == false; doVerify => SignatureException("Signature Verification failed!") */
  CG_SIG_MALFORMED = 2, /* engine SignatureException: Ed25519 length != 64, ECDSA DER decode failure */
  CG_KEY_INVALID = 3,   /* key decode IllegalArgumentException / InvalidKeyException */
  CG_UNSUPPORTED = 4,   /* IllegalArgumentException("Unsupported key/algorithm ...") */
  CG_EMPTY = 5,         /* doVerify: IllegalArgumentException("Signature data is empty!" / "Clear data is empty...") */
  CG_NOT_RUN = 255
};

/* Verification semantics. */
enum {
  CG_MODE_DOVERIFY = 0, /* Crypto.doVerify: empty sig / clear => CG_EMPTY */
  CG_MODE_ISVALID = 1   /* Crypto.isValid: no empty checks (empty sig => CG_SIG_MALFORMED) */
};

/* Infrastructure return codes (per-item outcomes are always in status_out). */
enum {
  CG_OK = 0,
  CG_ERR_ARG = -1,
  CG_ERR_DEVICE = -2,
  CG_ERR_NOMEM = -3,
  CG_ERR_RANGE = -4 /* an offset/length points outside the arena */
};

/* One public key, referenced by index from items (the JVM's PublicKey object). */
typedef struct cg_key {
  uint64_t off;      /* key bytes at arena[off .. off+len) */
  uint16_t len;
  uint8_t scheme;    /* CG_* scheme id */
  uint8_t fmt;       /* CG_KEY_* */
  uint32_t reserved; /* must be 0 */
} cg_key;            /* 16 bytes */

/* One signature to verify: (keys[key_idx], sig, clear). */
typedef struct cg_item {
  uint64_t sig_off;  /* signature bytes at arena[sig_off .. sig_off+sig_len) */
  uint64_t msg_off;  /* clear data at arena[msg_off .. msg_off+msg_len) */
  uint32_t msg_len;
  uint32_t key_idx;  /* index into the cg_key table */
  uint16_t sig_len;
  uint16_t reserved0;
  uint32_t reserved1;
} cg_item;           /* 32 bytes */

/* One variable-length message for the hashing entry points. */
typedef struct cg_span {
  uint64_t off;
  uint64_t len;
} cg_span;

/* Transaction component (Kryo-serialised bytes produced on the host). */
typedef struct cg_component {
  uint64_t off;
  uint32_t len;
  uint32_t flags;    /* bit 0: privacy-salt leaf (hashed without nonce, MerkleTransaction.kt:23-30) */
} cg_component;      /* 16 bytes */

/* One WireTransaction: components comps[first .. first+n) in availableComponents order
 * (inputs, attachments, outputs, commands, notary?, timeWindow?, privacySalt). */
typedef struct cg_tx {
  uint64_t first;
  uint32_t n;
  uint32_t reserved;
  uint64_t salt_off; /* 32-byte PrivacySalt value at arena[salt_off] (nonce = SHA256(salt||BE32(i))) */
} cg_tx;             /* 24 bytes */

/* Items per verify chunk when cg_config.chunk_items is 0. A call with more items is verified in
 * ceil(n / chunk) equal chunks against key tables built once for the whole call (so the per-item
 * workspace is bounded by the chunk, not the batch: BASELINE configs[4] streams 12.5M items per
 * GPU through one call). */
#define CG_DEFAULT_CHUNK_ITEMS (8u << 20)
/* Host-buffer calls (cg_verify_batch) pipeline H2D of chunk k+1 against the verify of chunk k
 * in chunks of at most this many items. */
#define CG_PIPELINE_CHUNK_ITEMS (2u << 20)

/* cg_config.flags */
#define CG_FLAG_STAGE_TIMING 1u /* time every item stage with HIP events on the stream it runs on (cg_stage_times) */
#define CG_FLAG_RSA 2u          /* verify CG_RSA_SHA256 items on the device (off: they stay CG_UNSUPPORTED, no RSA
                                   kernel runs and no RSA workspace is allocated) */
#define CG_FLAG_NO_KEY_CACHE 8u /* every call builds the wide tables of its hot keys (cg_key_cache_stats); bit 4u is
                                   unassigned and rejected like every unknown bit */

/* Item stages reported by cg_stage_times (one launch per verify chunk each). */
enum {
  CG_STAGE_PLAN = 0,           /* k_misc_status + plan sort */
  CG_STAGE_ED_HASH = 1,        /* k_ed_hash: SHA-512 challenges, scalar recoding */
  CG_STAGE_ED_LADDER = 2,      /* k_ed_ladder_pf: full-table keys */
  CG_STAGE_ED_LADDER_ROW0 = 3, /* k_ed_ladder<false>: keys with few items (side stream) */
  CG_STAGE_ED_FINISH = 4,      /* k_ed_finish: batched inversion, encode, compare */
  CG_STAGE_R1_FRONT = 5,       /* k_ec_prep + k_ec_inv, secp256r1 */
  CG_STAGE_R1_LADDER = 6,
  CG_STAGE_R1_LADDER_ROW0 = 7,
  CG_STAGE_K1_FRONT = 8,       /* k_ec_prep + k_ec_inv, secp256k1 */
  CG_STAGE_K1_LADDER = 9,
  CG_STAGE_K1_LADDER_ROW0 = 10,
  CG_STAGE_ED_LADDER_WIDE = 11, /* k_ed_ladder_wide: keys with wide tables (many items in the call) */
  CG_STAGE_R1_LADDER_WIDE = 12,
  CG_STAGE_K1_LADDER_WIDE = 13,
  CG_STAGES = 14
};

typedef struct cg_config {
  int32_t device;        /* HIP device ordinal (cg_open; cg_pool_open takes a device list) */
  uint32_t flags;        /* CG_FLAG_* (other bits: CG_ERR_ARG) */
  uint64_t max_items;    /* workspace sizing hint (0 = grow on demand) */
  uint64_t max_arena;    /* workspace sizing hint (0 = grow on demand) */
  uint64_t chunk_items;  /* items per verify chunk (0 = CG_DEFAULT_CHUNK_ITEMS) */
  uint32_t host_threads; /* host threads of this context's scans (key-use counts, chunk extents).
                            0 = CG_HOST_THREADS from the environment if set, else the process's CPU
                            quota (cgroup cpu.max, affinity) divided by the contexts open in the
                            process; at most 64. One process per GPU: pass quota / GPUs per node. */
  uint32_t reserved0;    /* must be 0 */
  uint64_t table_bytes_max; /* HBM the constant fixed-base tables (Ed25519 B, secp256r1 / secp256k1 G) may
                            take. They are built once per device per process at radix 2^26 (~91 GB), 2^24
                            (~25 GB) or 2^22 (~6.9 GB): fewer additions per item the larger (42 / 43 / 44),
                            same verdicts. > 0: the largest set within this many bytes (below the smallest:
                            CG_ERR_ARG). 0: CG_TABLE_BYTES_MAX from the environment if set (bytes, K/M/G
                            suffix), else automatic: a set this process already holds on the device, else
                            the largest that leaves CG_TABLE_HEADROOM of the device's free memory, else the
                            smallest; if its allocation fails (another process took the memory first), the
                            next smaller. cg_context_info reports the choice. */
  uint64_t reserved1;    /* must be 0: cg_open rejects anything else with CG_ERR_ARG */
} cg_config;             /* 56 bytes (static_assert in cordagpu.cpp) */

/* Device memory the automatic table choice leaves free for the calls' workspaces (16 GiB). */
#define CG_TABLE_HEADROOM (16ull << 30)

typedef struct cg_stats {
  uint64_t n_items;
  uint64_t n_keys;
  double ms_h2d;         /* host->device copy (host-buffer entry points only) */
  double ms_key_prep;    /* key decode + table build kernels */
  double ms_verify;      /* verify kernels */
  double ms_d2h;
  double ms_total;
} cg_stats;

typedef struct cg_ctx cg_ctx;

/* What a context was opened with (cg_context_info). */
typedef struct cg_info {
  int32_t device;
  uint32_t fixed_base_bits; /* radix 2^bits of the constant fixed-base tables this context reads: 26, 24 or 22 */
  uint64_t table_bytes;     /* their HBM (shared by every context of the process on the device) */
  uint32_t host_threads;    /* the host budget of this context's scans now (host_budget.h) */
  uint32_t reserved;
  uint64_t chunk_items;     /* items per verify chunk */
} cg_info;                  /* 32 bytes */

/* Library / device info. */
int cg_abi_version(void);
const char* cg_build_info(void);
int cg_device_count(void);
const char* cg_last_error(void); /* thread-local message for the last non-OK return */

int cg_open(cg_ctx** out, const cg_config* cfg);
void cg_close(cg_ctx* ctx);
int cg_context_info(const cg_ctx* ctx, cg_info* out);
/* The constant tables' budget arithmetic, HIP-free (no device needed): the HBM of the set at radix
 * 2^fixed_base_bits (0: no such build), and the radix cg_open would pick for a table_bytes_max on a
 * device with device_free bytes free and no set built yet in the process (0: the budget is below
 * every set, cg_open returns CG_ERR_ARG). */
uint64_t cg_table_bytes(uint32_t fixed_base_bits);
uint32_t cg_table_choice(uint64_t table_bytes_max, uint64_t device_free);
/* The modulus bit length if a CG_FLAG_RSA context would verify under this CG_KEY_SPKI key (the
 * accepted-key rule at the scheme enum; the same decode function the key-prep kernel runs), else 0:
 * such a key's items keep CG_UNSUPPORTED. HIP-free: a binding can pre-route with it. */
uint32_t cg_rsa_key_bits(const uint8_t* spki, uint32_t len);

/* Host memory registration (zero-copy ingestion). A caller that keeps its buffers across calls (a
 * JVM direct ByteBuffer arena, the out-of-process verifier's request buffers) registers them once:
 * the pages are pinned (hipHostRegister, every device) and the host entry points' copies out of
 * them go by DMA straight from those pages instead of through the runtime's CPU staging copy
 * (pageable memory: the calling thread memcpys every byte into a pinned bounce buffer first).
 * Process-wide; ranges may not overlap. The caller must unregister a range before it frees or
 * reuses that memory for anything else. Returns CG_OK, CG_ERR_ARG (NULL, zero length, overlap,
 * unknown pointer) or CG_ERR_DEVICE (the runtime refused). cg_host_registered: 1 if [p, p + len)
 * lies inside one registered range, else 0. */
int cg_host_register(const void* p, uint64_t len);
int cg_host_unregister(const void* p);
int cg_host_registered(const void* p, uint64_t len);
/* 1 when a caller whose node runs `contexts_per_node` contexts (one process per GPU: the GPUs per node;
 * a cg_pool: its slots) should register its buffers, else 0 (pageable is faster). Round 6 measured on
 * one MI355X: alone pageable wins by 10%; beside 7 other ranks' host copies registered wins by 5%
 * (profiles/r06/host8/summary.json). Advised from 4 contexts per node. HIP-free. */
int cg_host_register_advised(uint32_t contexts_per_node);

/* Host buffers in, host status bytes out (what a JNI caller hands over). The key table, the key
 * bytes and the item table go first; then the items are verified in consecutive chunks of at most
 * CG_PIPELINE_CHUNK_ITEMS, the arena bytes chunk k+1 needs (the extent of its items' signatures and
 * messages) copying on a copy stream while chunk k verifies. Only the arena window the keys and
 * items reference is copied. Best throughput when the caller appends (sig, clear) per item in item
 * order after the keys (the layout corda_amd/batch.py and INTEGRATION.md use); any layout is
 * correct: no offset (key, signature, message, and in the calls below component, salt, nonce, hash,
 * root, template) needs any alignment, fields may touch, and the arena may end at the last byte of
 * the last field with arena_len no multiple of 4. Lengths: sig_len and cg_key.len are 16-bit; a JVM signature longer than 65 535 bytes is
 * packed as a surrogate with the same verdict. stats: ms_h2d = until the
 * first chunk is resident, ms_verify = the rest. On CG_ERR_DEVICE every status byte is
 * CG_NOT_RUN.
 * CG_RSA_SHA256 items under a CG_FLAG_RSA context (this and every other verify entry point, the
 * device, transaction, tx-signature and pool forms included): with an accepted key (scheme enum) the
 * status is CG_VALID, CG_INVALID, CG_EMPTY (CG_MODE_DOVERIFY: sig_len == 0 or msg_len == 0) or
 * CG_NOT_RUN (signature or message outside the arena), with the ECDSA path's precedence; never
 * CG_SIG_MALFORMED or CG_KEY_INVALID: every failure inside BC's PSSSigner.verifySignature is `false`
 * (a signature longer than the modulus, s >= n, a PKCS#1 v1.5 block), and under CG_MODE_ISVALID an
 * empty signature is CG_INVALID. A shorter signature is the same integer with leading zeros. The bits
 * of the encoded message above emBits are masked, not checked (BC 1.57; OpenSSL rejects them). Any
 * other RSA key: CG_UNSUPPORTED, as without the flag. The RSA items are verified in one pass after
 * the call's other items; a call without RSA keys pays a few small launches. */
int cg_verify_batch(cg_ctx* ctx, const cg_key* keys, uint32_t n_keys, const cg_item* items, uint64_t n_items,
                    const uint8_t* arena, uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                    cg_stats* stats_opt);

/* Device-resident buffers (HBM pointers) on the caller's HIP stream (hipStream_t as void*; NULL =
 * the context's own stream, not the legacy default stream). Asynchronous: returns after
 * enqueueing; status is valid once the stream has reached that point. Workspace comes from the
 * ctx (reserve with cg_reserve); consecutive calls on one ctx are ordered on the device (each call
 * waits for the previous call's work, whatever stream either was enqueued on), because they share
 * that workspace. A caller's stream is bridged: the kernels run on the context's own stream (a
 * hardware queue of its own), which waits for the work already on the caller's stream, and the
 * caller's stream waits for the call's end, so the call is ordered on the caller's stream as if it
 * ran there (a stream created elsewhere can share an in-order hardware queue with the context's
 * side streams: round 6, corda_amd/csrc/call_scope.h). A call that fails after it began to enqueue
 * still makes the caller's stream wait for what it left in flight.
 * The arena of every *_device form (this one and cg_prepare_keys_device, cg_verify_items_device,
 * cg_sha256_batch_device, cg_tx_ids_device, cg_verify_transactions_device,
 * cg_verify_tx_signatures_device, cg_verify_tx_signatures_packed_device, cg_verify_filtered_device):
 * d_arena itself must be 4-byte aligned and readable up to arena_len rounded up to a multiple of 4
 * (the kernels read aligned dwords; what the up to 3 bytes past arena_len hold never matters). The
 * offsets inside it need no alignment, as in the host forms, which provide both themselves. */
int cg_reserve(cg_ctx* ctx, uint32_t max_keys, uint64_t max_items);
int cg_verify_batch_device(cg_ctx* ctx, const cg_key* d_keys, uint32_t n_keys, const cg_item* d_items,
                           uint64_t n_items, const uint8_t* d_arena, uint64_t arena_len, uint32_t mode,
                           uint8_t* d_status, void* hip_stream);
/* The two halves of cg_verify_batch_device: decode + precompute every key of the table into
 * the ctx workspace (the JVM's PublicKey construction), then verify items against it. A
 * verify call must follow a prepare call for the same key table on the same stream. */
int cg_prepare_keys_device(cg_ctx* ctx, const cg_key* d_keys, uint32_t n_keys, const uint8_t* d_arena,
                           uint64_t arena_len, void* hip_stream);
int cg_verify_items_device(cg_ctx* ctx, const cg_key* d_keys, uint32_t n_keys, const cg_item* d_items,
                           uint64_t n_items, const uint8_t* d_arena, uint64_t arena_len, uint32_t mode,
                           uint8_t* d_status, void* hip_stream);

/* Per-stage device time since the last call (ctx opened with CG_FLAG_STAGE_TIMING): waits for the
 * recorded work, then ms_out[stage] = summed event time of that stage's launches and
 * launches_out[stage] = their number, for stage < min(n, CG_STAGES); resets the record. Returns
 * the number of stages written. */
int cg_stage_times(cg_ctx* ctx, double* ms_out, uint32_t* launches_out, uint32_t n);

/* The context's wide-table cache. A key with many signatures in a call (>= 1,536 Ed25519, >= 512
 * ECDSA) gets "wide" tables, and a context keeps them between calls, keyed by the scheme and the
 * exact key bytes: a call builds them only for the hot keys it does not find (a full byte compare
 * decides, never a hash alone). Verdicts do not depend on it. On by default; off for a context with
 * CG_FLAG_NO_KEY_CACHE, for a process with CG_KEY_CACHE=0 in the environment at cg_open.
 * cg_key_cache_stats waits for the context's stream and reports the last call's counts per pool
 * ([0] Ed25519, [1] ECDSA, both curves). */
typedef struct cg_key_cache_info {
  uint32_t enabled;      /* 1: the cache is on for this context */
  uint32_t slots;        /* wide-table slots per pool the context holds (0: no pool allocated yet) */
  uint32_t hits[2];      /* hot keys whose tables were found */
  uint32_t built[2];     /* tables built and kept (a key that does not decode is never kept) */
  uint32_t evicted[2];   /* slots taken from another key's tables */
  uint32_t fell_back[2]; /* hot keys that took full tables instead (more hot keys than slots) */
} cg_key_cache_info;     /* 40 bytes */
int cg_key_cache_stats(cg_ctx* ctx, cg_key_cache_info* out);

/* Hashing. digests_out: 32*n (sha256) / 64*n (sha512) bytes. */
int cg_sha256_batch(cg_ctx* ctx, const cg_span* spans, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                    uint8_t* digests_out);
int cg_sha512_batch(cg_ctx* ctx, const cg_span* spans, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                    uint8_t* digests_out);
int cg_sha256_batch_device(cg_ctx* ctx, const cg_span* d_spans, uint64_t n, const uint8_t* d_arena,
                           uint64_t arena_len, uint8_t* d_digests, void* hip_stream);

/* Merkle roots of n independent leaf lists: leaf list j = leaves[32*first[j] .. 32*(first[j]+count[j])).
 * A list with count 0 gets status 1 (MerkleTreeException) and a zero root. */
int cg_merkle_roots(cg_ctx* ctx, const uint8_t* leaves, const uint64_t* first, const uint32_t* count,
                    uint64_t n, uint8_t* roots_out, uint8_t* status_out);

/* WireTransaction ids: ids_out 32*n_tx bytes; status_out 0 ok / 1 no leaves (MerkleTreeException) or
 * component range / salt outside the tables / 2 a component outside the arena / 3 a component
 * claimed by more than one transaction (each component belongs to at most one tx). */
int cg_tx_ids(cg_ctx* ctx, const cg_tx* txs, uint64_t n_tx, const cg_component* comps, uint64_t n_comps,
              const uint8_t* arena, uint64_t arena_len, uint8_t* ids_out, uint8_t* status_out);
int cg_tx_ids_device(cg_ctx* ctx, const cg_tx* d_txs, uint64_t n_tx, const cg_component* d_comps,
                     uint64_t n_comps, const uint8_t* d_arena, uint64_t arena_len, uint8_t* d_ids,
                     uint8_t* d_status, void* hip_stream);

/* ---- Transaction pipeline: WireTransaction ids -> SignableData -> every signature.
 * Replaces, for a batch of SignedTransactions, the serial
 *   id = WireTransaction.id (MerkleTransaction.kt:74-93, WireTransaction.kt:39)
 *   for (sig in sigs) Crypto.doVerify(id, sig)        (TransactionWithSignatures.kt:58-61,
 *                                                      Crypto.kt:499-502)
 * The clear data of signature s is SignableData(id, s.metadata).serialize(): for a fixed
 * metadata value that is prefix || id || suffix, so the caller passes one template per metadata
 * value (template bytes inside the arena) and the engine splices the device-computed ids in.
 * Signatures of a transaction whose id cannot be computed (status != 0), or that reference a
 * transaction / template out of range, get CG_NOT_RUN. */
typedef struct cg_signable_tmpl {
  uint64_t prefix_off; /* prefix bytes at arena[prefix_off .. +prefix_len) */
  uint64_t suffix_off; /* suffix bytes at arena[suffix_off .. +suffix_len) */
  uint32_t prefix_len;
  uint32_t suffix_len;
} cg_signable_tmpl;    /* 24 bytes */

typedef struct cg_txsig {
  uint64_t sig_off;    /* signature bytes at arena[sig_off .. +sig_len) */
  uint32_t tx_idx;     /* transaction whose id is signed */
  uint32_t key_idx;    /* TransactionSignature.by, index into the cg_key table */
  uint16_t sig_len;
  uint16_t tmpl;       /* SignatureMetadata template index */
  uint32_t reserved;   /* must be 0 */
} cg_txsig;            /* 24 bytes */

/* Device buffers in HBM except `tmpls` (a small host array). ids: 32*n_tx, tx_status: n_tx
 * (as cg_tx_ids), sig_status: n_sigs. */
int cg_verify_transactions_device(cg_ctx* ctx, const cg_tx* d_txs, uint64_t n_tx, const cg_component* d_comps,
                                  uint64_t n_comps, const cg_key* d_keys, uint32_t n_keys, const cg_txsig* d_sigs,
                                  uint64_t n_sigs, const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                                  const uint8_t* d_arena, uint64_t arena_len, uint32_t mode, uint8_t* d_ids,
                                  uint8_t* d_tx_status, uint8_t* d_sig_status, void* hip_stream);
/* Host buffers in and out (copies through the ctx). */
int cg_verify_transactions(cg_ctx* ctx, const cg_tx* txs, uint64_t n_tx, const cg_component* comps, uint64_t n_comps,
                           const cg_key* keys, uint32_t n_keys, const cg_txsig* sigs, uint64_t n_sigs,
                           const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                           uint64_t arena_len, uint32_t mode, uint8_t* ids_out, uint8_t* tx_status_out,
                           uint8_t* sig_status_out);

/* ---- Signatures over known transaction ids: the batch form of
 *   Crypto.doVerify(txId, transactionSignature)   core/.../crypto/Crypto.kt:499-502
 *     = doVerify(sig.by, sig.bytes, SignableData(txId, sig.signatureMetadata).serialize().bytes)
 *   (TransactionSignature.kt:27 carries `by` + `signatureMetadata`), called per signature by
 *   TransactionWithSignatures.checkSignaturesAreValid (TransactionWithSignatures.kt:58-61) and by
 *   the out-of-process verifier for each received transaction.
 * Such a caller holds the tx id and the signature's metadata, not message bytes: per signature it
 * passes a cg_txsig (24 B) and the signature bytes, per transaction its 32-byte id, and one
 * cg_signable_tmpl per SignatureMetadata value; the engine splices prefix || id || suffix on the
 * device. cg_txsig.tx_idx indexes `ids` (32 * n_ids bytes), tmpl indexes `tmpls`. A signature
 * whose id or template index is out of range, or whose template lies outside the arena, gets
 * CG_NOT_RUN; every other status as cg_verify_batch.
 * Host form: the key table, key and template bytes and the sampled key-use counts are copied
 * first (the key tables build from them), then each verify chunk's slice of the signature table,
 * the ids it references that are not resident yet, and its signature bytes, just before the
 * chunk runs, overlapping the key-table builds and the previous chunk's kernels. stats: ms_h2d =
 * until the first chunk's bytes are resident, ms_verify = the rest, ms_key_prep = the host-side
 * planning before the first copy (the key-use counts that pick each key's table mode: when the
 * keys average 256+ uses, a block sample of the signature table, 8 consecutive records per group,
 * 1 group in 32, each sampled key's count estimated upward and an unsampled key counted as row-0;
 * otherwise every record counted, exact). The counts change only speed, never a verdict. */
int cg_verify_tx_signatures(cg_ctx* ctx, const cg_key* keys, uint32_t n_keys, const uint8_t* ids, uint64_t n_ids,
                            const cg_txsig* sigs, uint64_t n_sigs, const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                            const uint8_t* arena, uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                            cg_stats* stats_opt);
/* Device buffers in HBM except `tmpls` (a small host array); asynchronous on hip_stream. */
int cg_verify_tx_signatures_device(cg_ctx* ctx, const cg_key* d_keys, uint32_t n_keys, const uint8_t* d_ids,
                                   uint64_t n_ids, const cg_txsig* d_sigs, uint64_t n_sigs,
                                   const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena,
                                   uint64_t arena_len, uint32_t mode, uint8_t* d_status, void* hip_stream);

/* ---- The same call with a 12-byte signature table (round 6, VERDICT r5 item 4: the 24-byte cg_txsig
 * was 300 MB of the 1.21 GB a BASELINE configs[4] shard ships over PCIe per call). A signature's bytes
 * are not addressed by an offset: the caller writes the signatures back to back in table order into
 * their own buffer, each starting at a 4-byte boundary (what a JVM writer appending to a direct
 * ByteBuffer does):
 *   signature i = sig_bytes[o_i .. o_i + sig_len_i),  o_0 = 0,  o_{i+1} = o_i + round_up(sig_len_i, 4)
 * The engine recovers the o_i with a prefix scan on the device. A signature whose bytes run past
 * sig_bytes_len gets CG_NOT_RUN; every other rule (ids, templates, the 16-bit surrogate for longer
 * JVM signatures, statuses, stats) is cg_verify_tx_signatures'. `arena` holds the key and template
 * bytes only. */
typedef struct cg_txsig_packed {
  uint32_t tx_idx;     /* transaction whose id is signed (index into ids) */
  uint32_t key_idx;    /* TransactionSignature.by, index into the cg_key table */
  uint16_t sig_len;
  uint16_t tmpl;       /* SignatureMetadata template index */
} cg_txsig_packed;     /* 12 bytes */

int cg_verify_tx_signatures_packed(cg_ctx* ctx, const cg_key* keys, uint32_t n_keys, const uint8_t* ids,
                                   uint64_t n_ids, const cg_txsig_packed* sigs, uint64_t n_sigs,
                                   const uint8_t* sig_bytes, uint64_t sig_bytes_len, const cg_signable_tmpl* tmpls,
                                   uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len, uint32_t mode,
                                   uint8_t* status_out, cg_stats* stats_opt);
/* Device buffers in HBM except `tmpls`; asynchronous on hip_stream. The signature stream lies inside
 * the arena: d_arena[sig_bytes_off .. sig_bytes_off + sig_bytes_len) (one HBM buffer holding the key
 * and template bytes and the stream: nothing is copied). */
int cg_verify_tx_signatures_packed_device(cg_ctx* ctx, const cg_key* d_keys, uint32_t n_keys, const uint8_t* d_ids,
                                          uint64_t n_ids, const cg_txsig_packed* d_sigs, uint64_t n_sigs,
                                          uint64_t sig_bytes_off, uint64_t sig_bytes_len,
                                          const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena,
                                          uint64_t arena_len, uint32_t mode, uint8_t* d_status, void* hip_stream);

/* ---- Per-transaction verdicts: TransactionWithSignatures.verifySignaturesExcept as one call
 *   (core/.../transactions/TransactionWithSignatures.kt:41-47, 58-62, 72-78):
 *   1. the first signature, in list order, that does not verify (its exception is what escapes);
 *   2. otherwise the required keys the signers do not fulfil; isFulfilledBy is composite-aware
 *      (CompositeKey.kt:186-209, CryptoUtils.kt:88-92).
 * The per-signature status bytes are reduced on the device, right behind the kernels that wrote them.
 *
 * Fulfilment is computed from the keys of ALL signatures of the span, whatever their statuses
 * (sigs.map { it.by }.toSet()). A composite node is fulfilled when the wrapping int32 sum of its
 * fulfilled children's weights is >= its threshold (a signed compare, List<Int>.sum()). With a signer
 * whose key entry has scheme CG_COMPOSITE_KEY every composite requirement is unfulfilled
 * (CompositeKey.kt:186-189); leaf requirements still compare classes. The first non-VALID status
 * includes CG_UNSUPPORTED and CG_NOT_RUN: the caller resolves those on the host for that transaction,
 * or re-queues it. Keys allowed to be missing are left out of `reqs` by the caller; CompositeKey
 * constraint and cycle validation (checkValidity) stays on the host, where it throws.
 *
 * Key classes: the key table's identity is (scheme, fmt, bytes), PublicKey.equals is not (the raw and
 * the SPKI form of one key are equal), so key_class[k] (uint32_t[n_keys]; NULL: the identity) gives key
 * entry k its equality class, assigned by the packer from its own equals. A leaf requirement names a
 * class; a required key that never signed is a class no signer has and needs no key-table entry.
 *
 * The device treats every table as untrusted data: each index is bounds-checked before the load
 * that uses it. A composite node's children must lie at indices greater than its own (else
 * CG_REQ_BAD); the walk is an explicit stack of at most CG_REQ_MAX_DEPTH composite nodes (a composite
 * nested deeper: CG_REQ_HOST), and one requirement visits at most CG_REQ_MAX_VISITS nodes (counting
 * a shared subtree once per path that reaches it; then CG_REQ_HOST). These two bounds make every loop
 * of the kernels finite for any input. */
#define CG_REQ_MAX_DEPTH 8
#define CG_REQ_MAX_VISITS 4096

typedef struct cg_tx_check {   /* one per transaction t (t indexes ids / cg_tx) */
  uint64_t first_sig;          /* its signatures are records [first_sig, first_sig + n_sigs) of the signature table, */
  uint32_t n_sigs;             /* in sigs-list order; each must carry tx_idx == t */
  uint32_t first_req;          /* its required keys are reqs[first_req .. first_req + n_req) */
  uint32_t n_req;
  uint32_t reserved;           /* must be 0 */
} cg_tx_check;                 /* 24 bytes */

typedef struct cg_req_node {   /* a required key: leaf or CompositeKey node */
  uint32_t a;                  /* leaf: key class; composite: index of its first child node */
  uint32_t n_children;         /* 0 = leaf; else children are nodes[a .. a + n_children) */
  int32_t  weight;             /* weight inside the parent (ignored for a root) */
  int32_t  threshold;          /* composite only */
} cg_req_node;                 /* 16 bytes */

typedef struct cg_tx_verdict {
  uint32_t first_bad;          /* ordinal inside the span of the first signature whose status != CG_VALID; 0xFFFFFFFF: none */
  uint8_t  status;             /* that signature's status (CG_VALID when none) */
  uint8_t  flags;              /* CG_TXV_* */
  uint16_t n_missing;          /* required keys not fulfilled, saturating */
} cg_tx_verdict;               /* 8 bytes */

/* req_status: one byte per `reqs` entry (an array of root node indices; node tables are shared between
 * transactions, requirement ranges are not: two transactions must not claim the same reqs entry).
 * Entries no transaction claims are CG_REQ_HOST. */
enum {
  CG_REQ_FULFILLED = 0,
  CG_REQ_MISSING = 1,
  CG_REQ_HOST = 2,   /* not evaluated, the caller walks it itself (deeper than CG_REQ_MAX_DEPTH, over the
                        visit budget, or its transaction's span is bad) */
  CG_REQ_BAD = 255   /* malformed table: a root or child range outside the node table, or children at
                        indices not greater than their parent's */
};
/* cg_tx_verdict.flags */
#define CG_TXV_SPAN_BAD 1u         /* the span leaves the signature table, a record in it has another tx_idx, or (device
                                      tables) cg_tx_check.reserved != 0: status = CG_NOT_RUN, first_bad = 0xFFFFFFFF,
                                      requirements not evaluated (CG_REQ_HOST) */
#define CG_TXV_REQ_HOST 2u         /* some requirement came back CG_REQ_HOST or CG_REQ_BAD, or the requirement range
                                      leaves `reqs` (then no req_status byte is written for it) */
#define CG_TXV_COMPOSITE_SIGNER 4u /* a signer's key entry has scheme CG_COMPOSITE_KEY */

/* The reduction alone, over any status array the engine produced (d_status[i] belongs to record i of the
 * signature table: the 12-byte cg_txsig_packed or the 24-byte cg_txsig, sig_stride says which; it
 * serves cg_verify_tx_signatures(_device) and cg_verify_transactions too). A signature whose key_idx
 * is outside the key table signs for no class. n_tx < 2^32. Device buffers in HBM, asynchronous on
 * hip_stream (bridged like every device call). Two kernels: one lane per transaction of up to 32
 * signatures, one wave per longer one. Errors: CG_ERR_ARG for a stride other than 12 / 24 or a NULL
 * table with a non-zero count (key_class may be NULL). */
int cg_tx_verdicts_device(cg_ctx* ctx, const void* d_sig_table, uint32_t sig_stride, uint64_t n_sigs,
                          const uint8_t* d_status, const cg_key* d_keys, uint32_t n_keys, const uint32_t* d_key_class,
                          const cg_tx_check* d_checks, uint64_t n_tx, const uint32_t* d_reqs, uint32_t n_reqs,
                          const cg_req_node* d_nodes, uint32_t n_nodes, cg_tx_verdict* d_verdicts,
                          uint8_t* d_req_status, void* hip_stream);
/* The same over host buffers (copies through the ctx); also CG_ERR_ARG for a non-zero
 * cg_tx_check.reserved. */
int cg_tx_verdicts(cg_ctx* ctx, const void* sig_table, uint32_t sig_stride, uint64_t n_sigs, const uint8_t* status,
                   const cg_key* keys, uint32_t n_keys, const uint32_t* key_class, const cg_tx_check* checks,
                   uint64_t n_tx, const uint32_t* reqs, uint32_t n_reqs, const cg_req_node* nodes, uint32_t n_nodes,
                   cg_tx_verdict* verdicts_out, uint8_t* req_status_out);

/* cg_verify_tx_signatures_packed(_device) followed by the verdict kernels on the same stream, after the
 * last verify chunk, with no host round trip: SignedTransaction.verifyRequiredSignatures for a batch.
 * Host form: status_out may be NULL, then the per-signature statuses are not copied back; the verdicts
 * and req_status always are. On an error every verdict is {0xFFFFFFFF, CG_NOT_RUN, CG_TXV_SPAN_BAD, 0}. */
int cg_verify_required_signatures_packed(cg_ctx* ctx, const cg_key* keys, uint32_t n_keys, const uint8_t* ids,
                                         uint64_t n_ids, const cg_txsig_packed* sigs, uint64_t n_sigs,
                                         const uint8_t* sig_bytes, uint64_t sig_bytes_len,
                                         const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                         uint64_t arena_len, uint32_t mode, const uint32_t* key_class,
                                         const cg_tx_check* checks, uint64_t n_tx, const uint32_t* reqs,
                                         uint32_t n_reqs, const cg_req_node* nodes, uint32_t n_nodes,
                                         uint8_t* status_out, cg_tx_verdict* verdicts_out, uint8_t* req_status_out,
                                         cg_stats* stats_opt);
int cg_verify_required_signatures_packed_device(cg_ctx* ctx, const cg_key* d_keys, uint32_t n_keys,
                                                const uint8_t* d_ids, uint64_t n_ids, const cg_txsig_packed* d_sigs,
                                                uint64_t n_sigs, uint64_t sig_bytes_off, uint64_t sig_bytes_len,
                                                const cg_signable_tmpl* tmpls, uint32_t n_tmpls,
                                                const uint8_t* d_arena, uint64_t arena_len, uint32_t mode,
                                                const uint32_t* d_key_class, const cg_tx_check* d_checks,
                                                uint64_t n_tx, const uint32_t* d_reqs, uint32_t n_reqs,
                                                const cg_req_node* d_nodes, uint32_t n_nodes, uint8_t* d_status,
                                                cg_tx_verdict* d_verdicts, uint8_t* d_req_status, void* hip_stream);

/* ---- Tear-offs: FilteredTransaction.verify / PartialMerkleTree.verify.
 * Replaces, for a batch of filtered transactions (the non-validating notary's input,
 * NonValidatingNotaryFlow.kt:22-27), the serial
 *   hashes = filteredLeaves.availableComponentHashes   serializedHash(x, nonce) = SHA256(kryo(x) || nonce)
 *                                                       (MerkleTransaction.kt:23-28,137)
 *   if (hashes.isEmpty()) throw MerkleTreeException      (MerkleTransaction.kt:173-178)
 *   partialMerkleTree.verify(rootHash, hashes)          (PartialMerkleTree.kt:130-156)
 * PartialMerkleTree.verify alone is the same call with precomputed leaf hashes
 * (CG_FLEAF_HASH) and without the empty check (no CG_FTX_FILTERED flag).
 *
 * The PartialTree is passed flattened in post-order (children before their parent):
 * CG_PMT_LEAF / CG_PMT_INCLUDED push the 32-byte hash at arena[hash_off] (INCLUDED also records
 * it as a used hash); CG_PMT_NODE pops right then left and pushes hashConcat(left, right). */
enum { CG_PMT_NODE = 0, CG_PMT_LEAF = 1, CG_PMT_INCLUDED = 2 };
typedef struct cg_pmt_node {
  uint64_t hash_off;   /* LEAF / INCLUDED: 32-byte SecureHash at arena[hash_off]; NODE: ignored */
  uint32_t kind;       /* CG_PMT_* */
  uint32_t reserved;   /* must be 0 */
} cg_pmt_node;         /* 16 bytes */

enum { CG_FLEAF_SALT = 1u, /* PrivacySalt component: SHA256(blob), no nonce (MerkleTransaction.kt:23-28) */
       CG_FLEAF_HASH = 2u  /* the 32 bytes at off are the leaf hash itself (len must be 32) */ };
typedef struct cg_filtered_leaf {
  uint64_t off;        /* serialised component bytes at arena[off .. off+len) */
  uint64_t nonce_off;  /* its 32-byte nonce (FilteredLeaves.nonces[i]) at arena[nonce_off] */
  uint32_t len;
  uint32_t flags;      /* CG_FLEAF_* */
} cg_filtered_leaf;    /* 24 bytes */

enum { CG_FTX_FILTERED = 1u /* FilteredTransaction.verify: no leaves => status 2 */ };
typedef struct cg_filtered_tx {
  uint64_t first_node; /* partial tree nodes[first_node .. +n_nodes), post-order */
  uint64_t first_leaf; /* hashesToCheck: leaves[first_leaf .. +n_leaves), availableComponents order */
  uint64_t root_off;   /* rootHash (32 bytes) at arena[root_off] */
  uint32_t n_nodes;
  uint32_t n_leaves;
  uint32_t flags;      /* CG_FTX_* */
  uint32_t reserved;   /* must be 0 */
} cg_filtered_tx;      /* 40 bytes */

/* status_out per transaction: 0 verify() == true; 1 verify() == false (root differs, or the
 * used-hash multiset differs from the leaf hashes); 2 MerkleTreeException("Transaction without
 * included leaves."); 3 malformed input the JVM object cannot express: a node / leaf range or
 * hash outside the tables / arena, an unknown node kind, a post-order stream that does not
 * reduce to one root, or a stack deeper than CG_PMT_MAX_DEPTH. */
#define CG_PMT_MAX_DEPTH 64
int cg_verify_filtered(cg_ctx* ctx, const cg_filtered_tx* ftxs, uint64_t n_ftx, const cg_pmt_node* nodes,
                       uint64_t n_nodes, const cg_filtered_leaf* leaves, uint64_t n_leaves, const uint8_t* arena,
                       uint64_t arena_len, uint8_t* status_out);
int cg_verify_filtered_device(cg_ctx* ctx, const cg_filtered_tx* d_ftxs, uint64_t n_ftx, const cg_pmt_node* d_nodes,
                              uint64_t n_nodes, const cg_filtered_leaf* d_leaves, uint64_t n_leaves,
                              const uint8_t* d_arena, uint64_t arena_len, uint8_t* d_status, void* hip_stream);

/* ---- Building tear-offs: WireTransaction.buildFilteredTransaction / PartialMerkleTree.build, the other
 * side of cg_verify_filtered. Replaces, for a batch of transactions (NotaryFlow.Client before a
 * non-validating notary, an oracle flow before Oracle.sign(ftx)), the serial
 *   filteredLeaves = filterWithFun(pred)                 visible component i keeps computeNonce(privacySalt, i)
 *                                                        = SHA256(salt32 || BE32(i)); the privacy salt is never
 *                                                        part of FilteredLeaves (WireTransaction.kt:97-167)
 *   rootHash = wtx.merkleTree.hash                       (MerkleTransaction.kt:159-166)
 *   pmt = PartialMerkleTree.build(merkleTree, filteredLeaves.availableComponentHashes)
 *                                                        (PartialMerkleTree.kt:66-123: a subtree without an
 *                                                        included leaf is cut to Leaf(its hash); the zeroHash
 *                                                        padding leaves are ordinary leaves of the full tree)
 * A filter that matches nothing still builds (one Leaf(root)); the later verify() is what throws.
 *
 * cg_build_filtered takes the cg_tx / cg_component tables and the arena as cg_tx_ids does, plus
 * visible[n_comps]: one byte per component, 0 hidden / 1 visible. It writes the tables cg_verify_filtered
 * reads, dense and in transaction order:
 *   ftxs_out[n_tx]   flags = CG_FTX_FILTERED, first_node / n_nodes / first_leaf / n_leaves, root_off
 *   nodes_out[]      the partial tree in cg_pmt_node post-order (NODE: hash_off 0)
 *   leaves_out[]     one record per visible component: off / len copied from the component (they still
 *                    point into the input arena), nonce_off into the output region, flags 0
 *   out[]            32-byte slots, per transaction: the root (the transaction id), the nonce of each
 *                    visible component in order, the hash of each LEAF / INCLUDED node in stream order
 * Every offset written into the tables that points into out[] is out_base + its byte position in out[]:
 * a caller that places out[] at arena[out_base ...) of one allocation passes everything to
 * cg_verify_filtered unchanged. out must be 16-byte aligned (the device form's d_out; out_base itself is
 * only a number).
 * Inclusion is by component index, the JVM's is by hash value; here they are the same rule: every
 * non-salt leaf of one transaction is hashed with the nonce of its own index, so two leaves of a tree
 * have equal hashes only by a SHA-256 collision, the salt leaf cannot be visible and no leaf is zeroHash.
 * Capacities (rows of nodes_out / leaves_out, bytes of out) come from the caller. Always enough, for a
 * transaction of n components padded to P = 2^k leaves: nodes <= 2P - 1 < 4n, LEAF + INCLUDED nodes
 * <= P < 2n, so node_cap = 4 n_comps, leaf_cap = n_comps, out_cap = 32 (n_tx + 3 n_comps).
 * totals_out: what the call needed. A capacity below it: the host form fails with CG_ERR_ARG, the needed
 * totals in cg_last_error and in totals_out, and writes no table; the device form (nothing syncs with the
 * host) sets totals.over = 1 and writes no row or slot at or past a capacity (ftxs and status are
 * complete, the other tables are not).
 * status_out per transaction: 0 built; 1 / 2 / 3 as cg_tx_ids (1 also: more than 2^30 components);
 * 6 a visible byte other than 0 or 1, or a visible privacy-salt component (FilteredLeaves cannot hold
 * one). A transaction that failed gets one zeroed root slot, n_nodes = 0 and n_leaves = 0.
 *
 * cg_build_partial_trees is bare PartialMerkleTree.build(tree, includeHashes): leaf-hash lists as
 * cg_merkle_roots takes them, plus one include list per tree, include[32 * inc_first[j] ..
 * 32 * (inc_first[j] + inc_count[j])). Inclusion is by value, as in the JVM. Same output tables; the leaf
 * records are CG_FLEAF_HASH and point at copies of the include hashes in out[] (slot order per
 * tree: root, include hashes, node hashes); ftx flags = 0, so the result is the input of bare
 * PartialMerkleTree.verify. Lists may share leaves. status per tree: 0 built; 1 an empty leaf list, more
 * than 2^30 leaves, or (device form) a list outside its table; 4 zeroHash in the include list
 * (IllegalArgumentException "Zero hashes shouldn't be included in partial tree."); 5 the number of
 * included leaves differs from inc_count (MerkleTreeException "Some of the provided hashes are not in
 * the tree.": a duplicate in the list, a hash the tree lacks, or an included hash that also sits at
 * another leaf). The device form's tables are 4-byte aligned; leaf_total is the sum of count[] (or any
 * upper bound of it: the size of the per-leaf scratch). */
typedef struct cg_build_totals {
  uint64_t n_nodes;    /* cg_pmt_node rows */
  uint64_t n_leaves;   /* cg_filtered_leaf rows */
  uint64_t out_bytes;  /* bytes of out[] */
  uint32_t over;       /* 1: a capacity is below what the call needed */
  uint32_t reserved;
} cg_build_totals;     /* 32 bytes */

int cg_build_filtered(cg_ctx* ctx, const cg_tx* txs, uint64_t n_tx, const cg_component* comps, uint64_t n_comps,
                      const uint8_t* arena, uint64_t arena_len, const uint8_t* visible, uint64_t out_base,
                      cg_filtered_tx* ftxs_out, cg_pmt_node* nodes_out, uint64_t node_cap,
                      cg_filtered_leaf* leaves_out, uint64_t leaf_cap, uint8_t* out, uint64_t out_cap,
                      uint8_t* status_out, cg_build_totals* totals_out);
int cg_build_filtered_device(cg_ctx* ctx, const cg_tx* d_txs, uint64_t n_tx, const cg_component* d_comps,
                             uint64_t n_comps, const uint8_t* d_arena, uint64_t arena_len, const uint8_t* d_visible,
                             uint64_t out_base, cg_filtered_tx* d_ftxs, cg_pmt_node* d_nodes, uint64_t node_cap,
                             cg_filtered_leaf* d_leaves, uint64_t leaf_cap, uint8_t* d_out, uint64_t out_cap,
                             uint8_t* d_status, cg_build_totals* d_totals, void* hip_stream);
int cg_build_partial_trees(cg_ctx* ctx, const uint8_t* leaves, const uint64_t* first, const uint32_t* count,
                           uint64_t n, const uint8_t* include, const uint64_t* inc_first, const uint32_t* inc_count,
                           uint64_t out_base, cg_filtered_tx* ftxs_out, cg_pmt_node* nodes_out, uint64_t node_cap,
                           cg_filtered_leaf* leaves_out, uint64_t leaf_cap, uint8_t* out, uint64_t out_cap,
                           uint8_t* status_out, cg_build_totals* totals_out);
int cg_build_partial_trees_device(cg_ctx* ctx, const uint8_t* d_leaves, uint64_t n_leaf_hashes,
                                  const uint64_t* d_first, const uint32_t* d_count, uint64_t n,
                                  uint64_t leaf_total, const uint8_t* d_include, uint64_t n_inc_hashes,
                                  const uint64_t* d_inc_first, const uint32_t* d_inc_count, uint64_t out_base,
                                  cg_filtered_tx* d_ftxs, cg_pmt_node* d_nodes, uint64_t node_cap,
                                  cg_filtered_leaf* d_leaves_out, uint64_t leaf_cap, uint8_t* d_out,
                                  uint64_t out_cap, uint8_t* d_status, cg_build_totals* d_totals, void* hip_stream);

/* ---- Ed25519 signing: the batch form of Crypto.doSign for EDDSA_ED25519_SHA512, the notary's own
 * step after it has checked a transaction's signatures:
 *   NotaryService.sign(txId)   core/.../node/services/NotaryService.kt:77-80
 *     = keyManagementService.sign(SignableData(txId, SignatureMetadata(platformVersion, schemeNumberID)), key)
 *     -> Crypto.doSign(keyPair, signableData)            core/.../crypto/Crypto.kt:415-422
 *     -> Crypto.doSign(privateKey, clearData)            Crypto.kt:395-402
 *     -> i2p 0.2.0 EdDSAEngine.engineSign: RFC 8032's deterministic signature
 *          r = SHA-512(h[32..64) || M) mod L, R = r B, S = (r + SHA-512(R || A || M) a) mod L
 *   (the BFT notary signs the same way, BFTSMaRt.kt:249-255). The output is byte for byte what the JVM
 *   writes. ECDSA and RSA-PSS signing have blocks of their own below (the host draws k, and the salt).
 * A context holds a signer set: private keys the node keeps in its own process
 * (PersistentKeyManagementService.kt:84-95), loaded once and named by index in every request. The seeds,
 * the expanded keys and every nonce r are secret: the signer store is a device allocation of its own,
 * zeroed before it is freed (cg_signers_clear, a reload, cg_close); a sign call zeroes the nonces and
 * their table digits on the stream before it returns. The fixed-base table is read at addresses that
 * depend on r, so the access pattern is not constant-time: this signer is for keys the node already holds
 * in memory, not a stand-in for an HSM.
 * Statuses: 0 signature written; CG_EMPTY msg_len == 0 (Crypto.kt:398 "Signing of an empty array is not
 * permitted!"); CG_NOT_RUN a signer, id or template index out of range, or bytes outside the arena. An
 * item that is not signed gets 64 zero bytes. With no signers loaded a sign call is CG_ERR_ARG and
 * writes nothing; n == 0 is a no-op. */
#define CG_SIGNERS_MAX 65535
/* EdDSAPrivateKeySpec(seed): replaces the context's signer set with the n keys of `seeds` (32 * n bytes).
 * pubkeys_out (32 * n bytes) receives each key's Abyte, which the caller compares with keyPair.public
 * (Crypto.kt:416-419 refuses a key pair whose halves do not belong together). */
int cg_signers_load(cg_ctx* ctx, const uint8_t* seeds, uint32_t n, uint8_t* pubkeys_out); /* no host copy is kept */
/* Zeroes and frees the signer set (a no-op when none is loaded). */
int cg_signers_clear(cg_ctx* ctx);
typedef struct cg_sign_req {
  uint32_t tx_idx;  /* the id to sign, index into ids */
  uint16_t signer;  /* index into the loaded signer set */
  uint16_t tmpl;    /* SignatureMetadata template index */
} cg_sign_req;      /* 8 bytes */
/* Crypto.doSign(keyPair, SignableData(ids[tx_idx], tmpl)) (Crypto.kt:415-422; NotaryService.kt:77-80) for
 * every request: the clear data is the template's prefix || id || suffix, spliced on the device as in
 * cg_verify_tx_signatures. sigs_out: 64 * n bytes (R || S), status_out: n bytes. */
int cg_sign_tx_ids(cg_ctx* ctx, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                   const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                   uint8_t* sigs_out, uint8_t* status_out);
/* Device buffers in HBM except `tmpls` (a small host array); asynchronous on hip_stream. d_ids, d_reqs,
 * d_arena and d_sigs must be 4-byte aligned. */
int cg_sign_tx_ids_device(cg_ctx* ctx, const uint8_t* d_ids, uint64_t n_ids, const cg_sign_req* d_reqs, uint64_t n,
                          const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena,
                          uint64_t arena_len, uint8_t* d_sigs, uint8_t* d_status, void* hip_stream);
typedef struct cg_sign_item {
  uint64_t msg_off;  /* clear data at arena[msg_off .. +msg_len) */
  uint32_t msg_len;
  uint32_t signer;   /* index into the loaded signer set */
} cg_sign_item;      /* 16 bytes */
/* Crypto.doSign(privateKey, clearData) (Crypto.kt:395-402; NotaryService.kt:73-75) over arena bytes. */
int cg_sign_batch(cg_ctx* ctx, const cg_sign_item* items, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                  uint8_t* sigs_out, uint8_t* status_out);

/* ---- ECDSA signing: the batch form of Crypto.doSign for ECDSA_SECP256K1_SHA256 (2) and
 * ECDSA_SECP256R1_SHA256 (3), with the nonce drawn by the caller:
 *   Crypto.doSign(privateKey, clearData)            core/.../crypto/Crypto.kt:395-402
 *   Crypto.doSign(keyPair, signableData)            Crypto.kt:415-422; NotaryService.kt:73-80
 *     -> BC 1.57 DSABase.engineSign -> ECDSASigner.generateSignature -> StdDSAEncoder.encode
 *          e = BigInteger(1, SHA-256(M)); k = BigInteger(256, random), redrawn while k = 0 or k >= n;
 *          r = x(k G) mod n, redrawn while 0; s = k^-1 (e + d r) mod n, the attempt repeated while 0;
 *          DERSequence(ASN1Integer(r), ASN1Integer(s)), 8 .. 72 bytes
 *   Every attempt of BC's loop consumes one 32-byte draw. A request carries one candidate k (32 bytes,
 *   big-endian: what RandomDSAKCalculator.nextK would have drawn); the device applies BC's refusals and
 *   answers CG_NONCE_REJECTED, and the caller redraws and resubmits that item alone: BC's loop for that
 *   item, and given the draws the output is byte for byte what the JVM writes. The device never draws
 *   randomness.
 * The ECDSA signer set is separate from the Ed25519 one: loading or clearing either leaves the other
 * untouched. Secret: d, every k and k^-1 and the table digits of k (given one k, d = (s k - e) / r). The
 * signer store is a device allocation of its own; the staged d bytes are zeroed on the stream right
 * behind the expansion, the store before every free (cg_ec_signers_clear, a reload, cg_close), and no
 * host copy is kept. A sign call zeroes its workspace on the stream behind the last chunk's last kernel,
 * also after a failed launch; the host forms zero their staged copy of the nonces too. Not cleared:
 * scratch memory and LDS. The fixed-base table is read at addresses that depend on digits of k, so the
 * access pattern is not constant-time, as for the Ed25519 signer above.
 * Statuses: 0 signed; CG_EMPTY msg_len == 0, checked before anything else (Crypto.kt:398); CG_NOT_RUN a
 * signer, id or template index out of range, bytes outside the arena, or a signer refused at load;
 * CG_NONCE_REJECTED the candidate is 0 or >= n, or gave r = 0 or s = 0. An item that is not signed gets 72
 * zero bytes and length 0. With no ECDSA signers loaded a sign call is CG_ERR_ARG and writes nothing;
 * n == 0 is a no-op. */
#define CG_NONCE_REJECTED 9 /* redraw this item's k and resubmit it */
#define CG_EC_SIG_MAX 72    /* bytes per signature slot */
/* Replaces the context's ECDSA signer set with n keys: schemes[i] (2 or 3) and 32 bytes of d, big-endian,
 * at secrets[32 i]; mixed curves are allowed, n <= CG_SIGNERS_MAX. pubs_out (64 * n bytes) receives X || Y
 * of d G, which the caller compares with keyPair.public (Crypto.kt:416-419). status_out (n bytes): 0
 * loaded; CG_KEY_INVALID d = 0 or d >= n; CG_UNSUPPORTED another scheme. A refused signer gets zero public
 * bytes and its requests later get CG_NOT_RUN (Crypto never makes such a key). */
int cg_ec_signers_load(cg_ctx* ctx, const uint8_t* schemes, const uint8_t* secrets, uint32_t n, uint8_t* pubs_out,
                       uint8_t* status_out); /* no host copy is kept */
/* Zeroes and frees the ECDSA signer set (a no-op when none is loaded). */
int cg_ec_signers_clear(cg_ctx* ctx);
/* Crypto.doSign(keyPair, SignableData(ids[tx_idx], tmpl)) for every request, as cg_sign_tx_ids; nonces:
 * 32 * n bytes, request i's candidate k. sigs_out: 72 * n bytes (the DER bytes, then zeros), sig_len_out
 * and status_out: n bytes each. */
int cg_ec_sign_tx_ids(cg_ctx* ctx, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                      const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                      const uint8_t* nonces, uint8_t* sigs_out, uint8_t* sig_len_out, uint8_t* status_out);
/* Device buffers in HBM except `tmpls` (a small host array); asynchronous on hip_stream. d_ids, d_reqs,
 * d_arena, d_nonces and d_sigs must be 4-byte aligned. The caller owns (and zeroes) d_nonces. */
int cg_ec_sign_tx_ids_device(cg_ctx* ctx, const uint8_t* d_ids, uint64_t n_ids, const cg_sign_req* d_reqs, uint64_t n,
                             const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena,
                             uint64_t arena_len, const uint8_t* d_nonces, uint8_t* d_sigs, uint8_t* d_sig_len,
                             uint8_t* d_status, void* hip_stream);
/* Crypto.doSign(privateKey, clearData) (Crypto.kt:395-402) over arena bytes. */
int cg_ec_sign_batch(cg_ctx* ctx, const cg_sign_item* items, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                     const uint8_t* nonces, uint8_t* sigs_out, uint8_t* sig_len_out, uint8_t* status_out);

/* ---- RSA-PSS signing: the batch form of Crypto.doSign for RSA_SHA256 (1), with the salt drawn by the caller:
 *   Crypto.doSign(privateKey, clearData)            core/.../crypto/Crypto.kt:395-402
 *   Crypto.doSign(keyPair, signableData)            Crypto.kt:415-422
 *     -> BC 1.57 "SHA256WITHRSAANDMGF1": PSSSignatureSpi.engineSign -> PSSSigner.generateSignature
 *        -> RSABlindedEngine.processBlock                                           [recalled]
 *          mHash = SHA-256(M); random.nextBytes(salt), 32 bytes; H = SHA-256(0^8 || mHash || salt);
 *          DB = PS || 01 || salt, masked with MGF1-SHA256(H); the bits above emBits = bits(n) - 1 cleared;
 *          EM = DB || H || BC; s = EM^d mod n through the CRT parts of a BCRSAPrivateCrtKey; the output
 *          block padded to k = ceil(bits(n) / 8) bytes                                [recalled]
 *   A request carries its salt (32 bytes: what random.nextBytes would have produced). Given the salt the
 *   signature is a pure function of (key, message, salt); BC never refuses or redraws a salt, so there is
 *   no status to resubmit. RSABlindedEngine's blinding changes no output byte and is not built. The device
 *   never draws randomness.
 * The RSA signer set is a third one: loading or clearing any of the three leaves the other two untouched.
 * Secret: p, q, dP, dQ, qInv and everything derived from them, every salt and H, the 16 powers of EM per
 * prime. The signer store is a device allocation of its own; the staged secret bytes are zeroed on the
 * stream right behind the expansion, the store before every free (cg_rsa_signers_clear, a reload,
 * cg_close), and no host copy is kept. A sign call zeroes its workspace on the stream behind the last
 * chunk's last kernel, also after a failed launch; the kernels zero their LDS tables; the host forms zero
 * their staged copy of the salts too. Not constant-time: the LDS address of a table read depends on a
 * window digit of dP / dQ, and the conditional subtraction of every modular product branches on the
 * operands. As for the other two signers: for keys the node already holds in memory, not a stand-in for an
 * HSM.
 * Every signature is checked before it leaves the device: s^e mod n is recomputed and compared with EM. A
 * CRT signature that is wrong modulo one prime gives away the factorisation of n; such an item gets
 * CG_SIGN_CHECK_FAILED and zero bytes.
 * Statuses: 0 signed; CG_EMPTY msg_len == 0, checked before anything else (Crypto.kt:398); CG_NOT_RUN a
 * signer, id or template index out of range, bytes outside the arena, or a signer refused at load;
 * CG_SIGN_CHECK_FAILED see above. An item that is not signed gets 512 zero bytes and length 0. With no RSA
 * signers loaded a sign call is CG_ERR_ARG and writes nothing; n == 0 is a no-op. */
#define CG_SIGN_CHECK_FAILED 10 /* the device recomputed s^e mod n and it did not equal EM: nothing written */
#define CG_RSA_SIG_MAX 512      /* bytes per signature slot */
/* One CRT private key (the fields of a BCRSAPrivateCrtKey; PKCS#1 RSAPrivateKey: qInv = q^-1 mod p): each
 * number a big-endian unsigned byte string at secrets[off .. off + len), at most one leading zero byte. */
typedef struct cg_rsa_signer {
  uint32_t n_off, n_len;
  uint32_t p_off, p_len;
  uint32_t q_off, q_len;
  uint32_t dp_off, dp_len;
  uint32_t dq_off, dq_len;
  uint32_t qinv_off, qinv_len;
  uint32_t e;        /* the public exponent, 1 .. 2^32 - 1 */
} cg_rsa_signer;     /* 52 bytes */
/* Replaces the context's RSA signer set with n keys, n <= CG_SIGNERS_MAX, secrets_len < 2^32. status_out
 * (n bytes): 0 loaded; CG_UNSUPPORTED bits(n) outside 1024 .. 4096 or a prime longer than 2048 bits;
 * CG_KEY_INVALID bytes outside `secrets`, n, p or q even, e = 0, dP >= p, dQ >= q, qInv >= p, or a failed
 * self-test (a fixed value signed through the CRT path must come back under e: catches p q != n and wrong
 * CRT parts). A refused signer does not disturb the others of the load; its requests later get CG_NOT_RUN. */
int cg_rsa_signers_load(cg_ctx* ctx, const cg_rsa_signer* signers, uint32_t n, const uint8_t* secrets,
                        uint64_t secrets_len, uint8_t* status_out); /* no host copy is kept */
/* Zeroes and frees the RSA signer set (a no-op when none is loaded). */
int cg_rsa_signers_clear(cg_ctx* ctx);
/* Crypto.doSign(keyPair, SignableData(ids[tx_idx], tmpl)) for every request, as cg_sign_tx_ids; salts:
 * 32 * n bytes, request i's salt. sigs_out: 512 * n bytes (k = ceil(bits(n) / 8) signature bytes, then
 * zeros), sig_len_out: n uint16_t (k, or 0), status_out: n bytes. */
int cg_rsa_sign_tx_ids(cg_ctx* ctx, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                       const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                       const uint8_t* salts, uint8_t* sigs_out, uint16_t* sig_len_out, uint8_t* status_out);
/* Device buffers in HBM except `tmpls` (a small host array); asynchronous on hip_stream. d_ids, d_reqs,
 * d_arena, d_salts and d_sigs must be 4-byte aligned. The caller owns (and zeroes) d_salts. */
int cg_rsa_sign_tx_ids_device(cg_ctx* ctx, const uint8_t* d_ids, uint64_t n_ids, const cg_sign_req* d_reqs, uint64_t n,
                              const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* d_arena,
                              uint64_t arena_len, const uint8_t* d_salts, uint8_t* d_sigs, uint16_t* d_sig_len,
                              uint8_t* d_status, void* hip_stream);
/* Crypto.doSign(privateKey, clearData) (Crypto.kt:395-402) over arena bytes. */
int cg_rsa_sign_batch(cg_ctx* ctx, const cg_sign_item* items, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                      const uint8_t* salts, uint8_t* sigs_out, uint16_t* sig_len_out, uint8_t* status_out);

/* ---- Key derivation: the batch form of Crypto.deriveKeyPair (core/.../crypto/Crypto.kt:646-771), the
 * call the reference points at for a unique key per transaction (Crypto.kt:631-637). Deterministic for
 * all three curves, so the output is byte for byte what the JVM returns:
 *   mac = HMAC-SHA512(key = keyData, msg = seed)                                   (deriveHMAC)
 *   keyData: a BC EC private key's d.toByteArray() (minimal two's complement, big-endian, 1..33 bytes),
 *            an EdDSA key's geta() (the 32 clamped bytes h[0..32) of SHA-512(seed)). The caller (the
 *            packers of the Python and Kotlin mirrors) forms keyData; the library does not reinterpret it.
 *   EDDSA_ED25519_SHA512: child seed = mac[0..32), EdDSAPrivateKeySpec(seed), public Abyte = encode(a B).
 *   ECDSA_SECP256R1/K1_SHA256: d = BigInteger(1, mac[0..32)); d is refused when d < 2, or
 *            bitCount(3d xor d) < 64 (WNafUtil.getNafWeight against n.bitLength() >>> 2), or d >= n, or
 *            d G is infinity (never, for 2 <= d < n). A refused d repeats the derivation with
 *            seed := SHA-256(seed). The device makes at most CG_DERIVE_MAX_RETRIES rehashes (each
 *            happens with probability about 2^-32 on secp256r1, far less on secp256k1); an item that
 *            still has no d gets CG_DERIVE_HOST and is finished by the caller's host restatement.
 * A seed of length 0 is legal. Statuses: 0 derived; CG_DERIVE_HOST; CG_DERIVE_BAD_PARENT the parent's
 * key_len is 0 (SecretKeySpec throws) or above 128 (would need a pre-hash of the key; never occurs);
 * CG_UNSUPPORTED the parent's scheme is none of the three (deriveKeyPair throws for RSA and SPHINCS);
 * CG_NOT_RUN the parent index, the parent's key bytes or the seed lie out of range. An item with a
 * status other than 0 gets zero secret and public bytes.
 * The parent key bytes on the device, the HMAC midstates, the macs, d and the table digits are secret:
 * the call's workspace is zeroed on the stream behind its last kernel (also after a failed launch) and
 * the library keeps no host copy. Not cleared: scratch memory and LDS. The table gathers are indexed by
 * digits of the child scalar: not constant-time, as for the signer above. The host always draws
 * randomness (generateKeyPair), never the device. */
#define CG_DERIVE_MAX_RETRIES 4
enum {
  CG_DERIVE_HOST = 6,       /* more than CG_DERIVE_MAX_RETRIES rehashes: finish this item on the host */
  CG_DERIVE_BAD_PARENT = 7, /* parent key_len == 0 or > 128 */
  CG_KEY_REJECTED = 8       /* cg_public_keys: the ECDSA candidate d fails the accept rule; redraw it */
};
typedef struct cg_derive_parent {
  uint64_t key_off;  /* keyData at arena[key_off .. key_off+key_len) */
  uint16_t key_len;  /* 1 .. 128 */
  uint8_t scheme;    /* CG_ECDSA_SECP256K1_SHA256, CG_ECDSA_SECP256R1_SHA256 or CG_EDDSA_ED25519_SHA512 */
  uint8_t pad[5];    /* must be 0 */
} cg_derive_parent;  /* 16 bytes */
typedef struct cg_derive_req {
  uint64_t seed_off;  /* seed at arena[seed_off .. seed_off+seed_len) */
  uint32_t seed_len;
  uint32_t parent;    /* index into the parent table */
} cg_derive_req;      /* 16 bytes */
/* Per request: secrets_out 32 bytes (Ed25519: the child seed; ECDSA: d big-endian), pubs_out 64 bytes
 * (Ed25519: Abyte, then 32 zero bytes; ECDSA: X || Y big-endian), status_out 1 byte, and when
 * retries_out_opt is not NULL the number of rehashes made (0 for Ed25519). */
int cg_derive_keys(cg_ctx* ctx, const cg_derive_parent* parents, uint32_t n_parents, const cg_derive_req* reqs,
                   uint64_t n, const uint8_t* arena, uint64_t arena_len, uint8_t* secrets_out, uint8_t* pubs_out,
                   uint8_t* status_out, uint8_t* retries_out_opt);
/* Device buffers in HBM (d_arena, d_secrets and d_pubs 4-byte aligned: the kernels move them as 32-bit
 * words; d_arena readable up to arena_len rounded up to 4); asynchronous on hip_stream. */
int cg_derive_keys_device(cg_ctx* ctx, const cg_derive_parent* d_parents, uint32_t n_parents,
                          const cg_derive_req* d_reqs, uint64_t n, const uint8_t* d_arena, uint64_t arena_len,
                          uint8_t* d_secrets, uint8_t* d_pubs, uint8_t* d_status, uint8_t* d_retries_opt,
                          void* hip_stream);
/* The second half alone: private key -> public key for n secrets of one scheme (32 * n bytes).
 * Ed25519: seed -> Abyte (deriveKeyPairFromEntropy; generateKeyPair with host-drawn SecureRandom bytes).
 * ECDSA: a candidate d (big-endian) goes through the accept rule, then Q = d G; a refused candidate
 * gets CG_KEY_REJECTED and zero bytes, and the host redraws it. pubs_out: 64 * n bytes as above. */
int cg_public_keys(cg_ctx* ctx, uint32_t scheme, const uint8_t* secrets, uint64_t n, uint8_t* pubs_out,
                   uint8_t* status_out);
/* d_secrets and d_pubs 4-byte aligned, as above. */
int cg_public_keys_device(cg_ctx* ctx, uint32_t scheme, const uint8_t* d_secrets, uint64_t n, uint8_t* d_pubs,
                          uint8_t* d_status, void* hip_stream);

/* ---- Several devices in one process (the JVM process drives every GPU of the node).
 * A pool holds one cg_ctx per slot (a slot is a device ordinal; a device may appear twice).
 * cg_pool_verify_batch cuts the items into contiguous, equal shards, one per healthy slot, runs
 * each shard as a cg_verify_batch on its own host thread, and each shard's D2H copy lands in its
 * slice of status_out (that copy is the gather). A shard whose device fails marks its slot
 * unhealthy and is re-run on a healthy slot; items that could not run anywhere stay CG_NOT_RUN
 * and the call returns CG_ERR_DEVICE, so the caller re-queues exactly those (the analogue of the
 * verifier's Artemis redelivery, OutOfProcessTransactionVerifierService.kt:65-72). */
typedef struct cg_pool cg_pool;
typedef struct cg_pool_stats {
  uint32_t shards;        /* shards of the first pass (= healthy slots at the call) */
  uint32_t reruns;        /* shard re-runs after a failure */
  uint32_t failed_slots;  /* slots that failed during this call (now unhealthy) */
  uint32_t reserved;
  uint64_t not_run;       /* items left CG_NOT_RUN */
  double ms_total;
} cg_pool_stats;
int cg_pool_open(cg_pool** out, const int32_t* devices, uint32_t n_slots, const cg_config* cfg);
void cg_pool_close(cg_pool* pool);
uint32_t cg_pool_slots(const cg_pool* pool);
int cg_pool_slot_healthy(const cg_pool* pool, uint32_t slot);  /* 1 healthy, 0 failed, -1 bad slot */
int cg_pool_verify_batch(cg_pool* pool, const cg_key* keys, uint32_t n_keys, const cg_item* items, uint64_t n_items,
                         const uint8_t* arena, uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                         cg_pool_stats* stats_opt);
/* cg_verify_tx_signatures sharded the same way: contiguous, equal shards of the signature table,
 * one per healthy slot, each shard a cg_verify_tx_signatures on its device (ids, keys and templates
 * go to every device; each shard copies only its own signature bytes). */
int cg_pool_verify_tx_signatures(cg_pool* pool, const cg_key* keys, uint32_t n_keys, const uint8_t* ids,
                                 uint64_t n_ids, const cg_txsig* sigs, uint64_t n_sigs,
                                 const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                 uint64_t arena_len, uint32_t mode, uint8_t* status_out, cg_pool_stats* stats_opt);
/* cg_verify_transactions on a pool. A signature may reference any transaction's id, so the call is not
 * sharded: it runs whole on the first healthy slot and, if that slot's device fails (the slot is then
 * marked unhealthy), on the next one. When no slot could run it, every sig status stays CG_NOT_RUN and
 * the call returns CG_ERR_DEVICE (re-queue the request). stats_opt->not_run counts the signatures. */
int cg_pool_verify_transactions(cg_pool* pool, const cg_tx* txs, uint64_t n_tx, const cg_component* comps,
                                uint64_t n_comps, const cg_key* keys, uint32_t n_keys, const cg_txsig* sigs,
                                uint64_t n_sigs, const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                uint64_t arena_len, uint32_t mode, uint8_t* ids_out, uint8_t* tx_status_out,
                                uint8_t* sig_status_out, cg_pool_stats* stats_opt);
/* cg_verify_tx_signatures_packed sharded the same way (each shard's signature bytes start where the
 * previous shard's end: the library sums the lengths at the shard bounds). */
int cg_pool_verify_tx_signatures_packed(cg_pool* pool, const cg_key* keys, uint32_t n_keys, const uint8_t* ids,
                                        uint64_t n_ids, const cg_txsig_packed* sigs, uint64_t n_sigs,
                                        const uint8_t* sig_bytes, uint64_t sig_bytes_len,
                                        const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                        uint64_t arena_len, uint32_t mode, uint8_t* status_out,
                                        cg_pool_stats* stats_opt);
/* cg_verify_required_signatures_packed on a pool: cg_pool_verify_tx_signatures_packed (shards, re-run
 * on a fault), then cg_tx_verdicts on a healthy slot over the gathered statuses. Signatures no slot
 * could run stay CG_NOT_RUN and surface as status = CG_NOT_RUN verdicts (the call then returns
 * CG_ERR_DEVICE like the pool call, with the verdicts written). status_out may be NULL. */
int cg_pool_verify_required_signatures_packed(cg_pool* pool, const cg_key* keys, uint32_t n_keys, const uint8_t* ids,
                                              uint64_t n_ids, const cg_txsig_packed* sigs, uint64_t n_sigs,
                                              const uint8_t* sig_bytes, uint64_t sig_bytes_len,
                                              const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena,
                                              uint64_t arena_len, uint32_t mode, const uint32_t* key_class,
                                              const cg_tx_check* checks, uint64_t n_tx, const uint32_t* reqs,
                                              uint32_t n_reqs, const cg_req_node* nodes, uint32_t n_nodes,
                                              uint8_t* status_out, cg_tx_verdict* verdicts_out,
                                              uint8_t* req_status_out, cg_pool_stats* stats_opt);
/* The signer set on every slot (cg_signers_load per slot; pubkeys_out from the first). A slot whose
 * device fails is marked unhealthy; the call fails only when no slot could load the set. A slot that
 * stayed healthy but could not load the set is passed over by cg_pool_sign_tx_ids. The library keeps no
 * host copy of the seeds: they are copied from the caller's buffer to each device. */
int cg_pool_signers_load(cg_pool* pool, const uint8_t* seeds, uint32_t n, uint8_t* pubkeys_out);
int cg_pool_signers_clear(cg_pool* pool);
/* cg_sign_tx_ids on a pool: not sharded, the whole call runs on the first healthy slot and, if that
 * slot's device fails, on the next one (the cg_pool_verify_transactions pattern). When no slot could run
 * it the status bytes are CG_NOT_RUN, the signatures zero, and the call returns CG_ERR_DEVICE. */
int cg_pool_sign_tx_ids(cg_pool* pool, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                        const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                        uint8_t* sigs_out, uint8_t* status_out, cg_pool_stats* stats_opt);
/* The ECDSA signer set on every slot and cg_ec_sign_tx_ids on a pool, by the rules of the three calls
 * above (pubs_out and status_out of the load from the first slot that loaded). When no slot could run the
 * sign call the status bytes are CG_NOT_RUN, the signatures and lengths zero, and it returns CG_ERR_DEVICE. */
int cg_pool_ec_signers_load(cg_pool* pool, const uint8_t* schemes, const uint8_t* secrets, uint32_t n,
                            uint8_t* pubs_out, uint8_t* status_out);
int cg_pool_ec_signers_clear(cg_pool* pool);
int cg_pool_ec_sign_tx_ids(cg_pool* pool, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                           const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                           const uint8_t* nonces, uint8_t* sigs_out, uint8_t* sig_len_out, uint8_t* status_out,
                           cg_pool_stats* stats_opt);
/* The RSA signer set on every slot and cg_rsa_sign_tx_ids on a pool, by the same rules (status_out of the
 * load from the first slot that loaded). */
int cg_pool_rsa_signers_load(cg_pool* pool, const cg_rsa_signer* signers, uint32_t n, const uint8_t* secrets,
                             uint64_t secrets_len, uint8_t* status_out);
int cg_pool_rsa_signers_clear(cg_pool* pool);
int cg_pool_rsa_sign_tx_ids(cg_pool* pool, const uint8_t* ids, uint64_t n_ids, const cg_sign_req* reqs, uint64_t n,
                            const cg_signable_tmpl* tmpls, uint32_t n_tmpls, const uint8_t* arena, uint64_t arena_len,
                            const uint8_t* salts, uint8_t* sigs_out, uint16_t* sig_len_out, uint8_t* status_out,
                            cg_pool_stats* stats_opt);
/* cg_derive_keys on a pool: not sharded, the whole call runs on the first healthy slot and, if that
 * slot's device fails, on the next one (as cg_pool_sign_tx_ids). When no slot could run it the status
 * bytes are CG_NOT_RUN, the outputs zero, and the call returns CG_ERR_DEVICE. */
int cg_pool_derive_keys(cg_pool* pool, const cg_derive_parent* parents, uint32_t n_parents,
                        const cg_derive_req* reqs, uint64_t n, const uint8_t* arena, uint64_t arena_len,
                        uint8_t* secrets_out, uint8_t* pubs_out, uint8_t* status_out, uint8_t* retries_out_opt,
                        cg_pool_stats* stats_opt);
/* cg_public_keys on a pool, the same way. */
int cg_pool_public_keys(cg_pool* pool, uint32_t scheme, const uint8_t* secrets, uint64_t n, uint8_t* pubs_out,
                        uint8_t* status_out, cg_pool_stats* stats_opt);
/* Failure drill: make every later call on `slot` fail as a device fault would (fail = 1), or
 * clear it and mark the slot healthy again (fail = 0). For tests and operational drills. */
int cg_pool_inject_fault(cg_pool* pool, uint32_t slot, int fail);

#ifdef __cplusplus
}
#endif
#endif /* CORDAGPU_H */
