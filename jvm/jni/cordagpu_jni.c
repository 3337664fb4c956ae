/* cordagpu_jni.c -- JNI shim between net.corda.core.crypto.CryptoBatch (jvm/src/main/kotlin) and
 * libcordagpu.so (include/cordagpu.h). Plain C, direct ByteBuffers only: the JVM hands over the
 * addresses of its off-heap buffers, the engine copies what it needs and keeps no pointer after a
 * call returns (a buffer passed to cg_host_register stays pinned until cg_host_unregister).
 *
 * Build (on a node with a JDK; this repository's image has none, so it is not compiled here):
 *   gcc -O2 -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude \
 *       jvm/jni/cordagpu_jni.c -Lcorda_amd -lcordagpu -o libcordagpu_jni.so
 */
#include <jni.h>
#include <stdint.h>
#include <stdio.h>

#include "cordagpu.h"

#define ADDR(b) ((b) ? (*env)->GetDirectBufferAddress(env, (b)) : NULL)

static void throw_state(JNIEnv* env, const char* fn, int rc) {
  char msg[768];
  const char* why = cg_last_error();
  snprintf(msg, sizeof msg, "%s failed (%d): %s", fn, rc, why ? why : "");
  jclass ex = (*env)->FindClass(env, "java/lang/IllegalStateException");
  if (ex) (*env)->ThrowNew(env, ex, msg);
}

static cg_config make_config(jlong chunk_items, jint host_threads, jlong table_bytes_max, jint flags) {
  cg_config cfg = {0}; /* ABI v2: reserved words must be 0 */
  cfg.chunk_items = (uint64_t)chunk_items;
  cfg.host_threads = (uint32_t)host_threads;
  cfg.table_bytes_max = (uint64_t)table_bytes_max; /* 0: automatic (include/cordagpu.h) */
  cfg.flags = (uint32_t)flags;                     /* CG_FLAG_RSA when gpuVerifier.gpuRsa is set */
  return cfg;
}

JNIEXPORT jlong JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeOpen(JNIEnv* env, jobject self, jint dev,
                                                                         jlong chunk_items, jint host_threads,
                                                                         jlong table_bytes_max, jint flags) {
  cg_config cfg = make_config(chunk_items, host_threads, table_bytes_max, flags);
  cfg.device = dev;
  cg_ctx* ctx = 0;
  int rc = cg_open(&ctx, &cfg);
  if (rc != CG_OK) {
    throw_state(env, "cg_open", rc);
    return 0;
  }
  return (jlong)(intptr_t)ctx;
}

/* Exactly one of ctx / pool is non-zero (CryptoBatch.handles). */
JNIEXPORT void JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeClose(JNIEnv* env, jobject self, jlong ctx,
                                                                          jlong pool) {
  if (ctx) cg_close((cg_ctx*)(intptr_t)ctx);
  if (pool) cg_pool_close((cg_pool*)(intptr_t)pool);
}

/* One JVM process, every GPU of the node: a pool over the device list. */
JNIEXPORT jlong JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeOpenPool(JNIEnv* env, jobject self,
                                                                             jintArray devs, jlong chunk_items,
                                                                             jint host_threads, jlong table_bytes_max,
                                                                             jint flags) {
  jsize n = (*env)->GetArrayLength(env, devs);
  jint* d = (*env)->GetIntArrayElements(env, devs, 0);
  cg_config cfg = make_config(chunk_items, host_threads, table_bytes_max, flags);
  cg_pool* pool = 0;
  int rc = cg_pool_open(&pool, (const int32_t*)d, (uint32_t)n, &cfg);
  (*env)->ReleaseIntArrayElements(env, devs, d, JNI_ABORT);
  if (rc != CG_OK) {
    throw_state(env, "cg_pool_open", rc);
    return 0;
  }
  return (jlong)(intptr_t)pool;
}

/* Crypto.doVerify / isValid over (key, sig, clear) items: cg_verify_batch; stats: a 56-byte cg_stats.
 * pool != 0: cg_pool_verify_batch, the items sharded over every healthy device of the pool (no
 * per-stage stats then: the stats buffer is left untouched and the binding skips its device timers). */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeVerify(
    JNIEnv* env, jobject self, jlong ctx, jlong pool, jobject keys, jint n_keys, jobject items, jlong n_items,
    jobject arena, jlong arena_len, jint mode, jobject status, jobject stats) {
  if (pool)
    return cg_pool_verify_batch((cg_pool*)(intptr_t)pool, (const cg_key*)ADDR(keys), (uint32_t)n_keys,
                                (const cg_item*)ADDR(items), (uint64_t)n_items, (const uint8_t*)ADDR(arena),
                                (uint64_t)arena_len, (uint32_t)mode, (uint8_t*)ADDR(status), 0);
  return cg_verify_batch((cg_ctx*)(intptr_t)ctx, (const cg_key*)ADDR(keys), (uint32_t)n_keys,
                         (const cg_item*)ADDR(items), (uint64_t)n_items, (const uint8_t*)ADDR(arena),
                         (uint64_t)arena_len, (uint32_t)mode, (uint8_t*)ADDR(status), (cg_stats*)ADDR(stats));
}

/* Crypto.doVerify(txId, TransactionSignature) over many transactions, over the 12-byte signature
 * table and the dense signature stream: cg_verify_tx_signatures_packed (pool != 0:
 * cg_pool_verify_tx_signatures_packed over every device of the pool; no per-stage stats then). */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeVerifyTxSignaturesPacked(
    JNIEnv* env, jobject self, jlong ctx, jlong pool, jobject keys, jint n_keys, jobject ids, jlong n_ids,
    jobject sigs, jlong n_sigs, jobject sig_bytes, jlong sig_bytes_len, jobject tmpls, jint n_tmpls, jobject arena,
    jlong arena_len, jint mode, jobject status, jobject stats) {
  if (pool)
    return cg_pool_verify_tx_signatures_packed((cg_pool*)(intptr_t)pool, (const cg_key*)ADDR(keys), (uint32_t)n_keys,
                                               (const uint8_t*)ADDR(ids), (uint64_t)n_ids,
                                               (const cg_txsig_packed*)ADDR(sigs), (uint64_t)n_sigs,
                                               (const uint8_t*)ADDR(sig_bytes), (uint64_t)sig_bytes_len,
                                               (const cg_signable_tmpl*)ADDR(tmpls), (uint32_t)n_tmpls,
                                               (const uint8_t*)ADDR(arena), (uint64_t)arena_len, (uint32_t)mode,
                                               (uint8_t*)ADDR(status), 0);
  return cg_verify_tx_signatures_packed((cg_ctx*)(intptr_t)ctx, (const cg_key*)ADDR(keys), (uint32_t)n_keys,
                                        (const uint8_t*)ADDR(ids), (uint64_t)n_ids, (const cg_txsig_packed*)ADDR(sigs),
                                        (uint64_t)n_sigs, (const uint8_t*)ADDR(sig_bytes), (uint64_t)sig_bytes_len,
                                        (const cg_signable_tmpl*)ADDR(tmpls), (uint32_t)n_tmpls,
                                        (const uint8_t*)ADDR(arena), (uint64_t)arena_len, (uint32_t)mode,
                                        (uint8_t*)ADDR(status), (cg_stats*)ADDR(stats));
}

/* SignedTransaction.verifyRequiredSignatures over many transactions: the packed tx-signature call followed
 * by the per-transaction verdict kernels (cg_verify_required_signatures_packed; pool != 0:
 * cg_pool_verify_required_signatures_packed). key_class and status may be null buffers (ADDR gives 0). */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeVerifyRequiredPacked(
    JNIEnv* env, jobject self, jlong ctx, jlong pool, jobject keys, jint n_keys, jobject ids, jlong n_ids,
    jobject sigs, jlong n_sigs, jobject sig_bytes, jlong sig_bytes_len, jobject tmpls, jint n_tmpls, jobject arena,
    jlong arena_len, jint mode, jobject key_class, jobject checks, jlong n_tx, jobject reqs, jint n_reqs,
    jobject nodes, jint n_nodes, jobject status, jobject verdicts, jobject req_status) {
  if (pool)
    return cg_pool_verify_required_signatures_packed(
        (cg_pool*)(intptr_t)pool, (const cg_key*)ADDR(keys), (uint32_t)n_keys, (const uint8_t*)ADDR(ids),
        (uint64_t)n_ids, (const cg_txsig_packed*)ADDR(sigs), (uint64_t)n_sigs, (const uint8_t*)ADDR(sig_bytes),
        (uint64_t)sig_bytes_len, (const cg_signable_tmpl*)ADDR(tmpls), (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena),
        (uint64_t)arena_len, (uint32_t)mode, (const uint32_t*)ADDR(key_class), (const cg_tx_check*)ADDR(checks),
        (uint64_t)n_tx, (const uint32_t*)ADDR(reqs), (uint32_t)n_reqs, (const cg_req_node*)ADDR(nodes),
        (uint32_t)n_nodes, (uint8_t*)ADDR(status), (cg_tx_verdict*)ADDR(verdicts), (uint8_t*)ADDR(req_status), 0);
  return cg_verify_required_signatures_packed(
      (cg_ctx*)(intptr_t)ctx, (const cg_key*)ADDR(keys), (uint32_t)n_keys, (const uint8_t*)ADDR(ids), (uint64_t)n_ids,
      (const cg_txsig_packed*)ADDR(sigs), (uint64_t)n_sigs, (const uint8_t*)ADDR(sig_bytes), (uint64_t)sig_bytes_len,
      (const cg_signable_tmpl*)ADDR(tmpls), (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena), (uint64_t)arena_len,
      (uint32_t)mode, (const uint32_t*)ADDR(key_class), (const cg_tx_check*)ADDR(checks), (uint64_t)n_tx,
      (const uint32_t*)ADDR(reqs), (uint32_t)n_reqs, (const cg_req_node*)ADDR(nodes), (uint32_t)n_nodes,
      (uint8_t*)ADDR(status), (cg_tx_verdict*)ADDR(verdicts), (uint8_t*)ADDR(req_status), 0);
}

/* WireTransaction ids + every signature (cg_verify_transactions; pool != 0: cg_pool_verify_transactions,
 * the whole call on one healthy device, the next one on a device fault). */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeVerifyTransactions(
    JNIEnv* env, jobject self, jlong ctx, jlong pool, jobject txs, jlong n_tx, jobject comps, jlong n_comps,
    jobject keys, jint n_keys, jobject sigs, jlong n_sigs, jobject tmpls, jint n_tmpls, jobject arena, jlong arena_len,
    jint mode, jobject ids_out, jobject tx_status_out, jobject sig_status_out) {
  if (pool)
    return cg_pool_verify_transactions((cg_pool*)(intptr_t)pool, (const cg_tx*)ADDR(txs), (uint64_t)n_tx,
                                       (const cg_component*)ADDR(comps), (uint64_t)n_comps, (const cg_key*)ADDR(keys),
                                       (uint32_t)n_keys, (const cg_txsig*)ADDR(sigs), (uint64_t)n_sigs,
                                       (const cg_signable_tmpl*)ADDR(tmpls), (uint32_t)n_tmpls,
                                       (const uint8_t*)ADDR(arena), (uint64_t)arena_len, (uint32_t)mode,
                                       (uint8_t*)ADDR(ids_out), (uint8_t*)ADDR(tx_status_out),
                                       (uint8_t*)ADDR(sig_status_out), 0);
  return cg_verify_transactions((cg_ctx*)(intptr_t)ctx, (const cg_tx*)ADDR(txs), (uint64_t)n_tx,
                                (const cg_component*)ADDR(comps), (uint64_t)n_comps, (const cg_key*)ADDR(keys),
                                (uint32_t)n_keys, (const cg_txsig*)ADDR(sigs), (uint64_t)n_sigs,
                                (const cg_signable_tmpl*)ADDR(tmpls), (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena),
                                (uint64_t)arena_len, (uint32_t)mode, (uint8_t*)ADDR(ids_out),
                                (uint8_t*)ADDR(tx_status_out), (uint8_t*)ADDR(sig_status_out));
}

/* EdDSAPrivateKeySpec(seed) for every 32-byte seed: the signer set of the context (cg_signers_load), or of
 * every device of the pool (cg_pool_signers_load). pubkeys_out: each key's Abyte, which the binding
 * compares with keyPair.public (Crypto.kt:416-419). The binding zeroes its seed buffer afterwards. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeLoadSigners(JNIEnv* env, jobject self, jlong ctx,
                                                                              jlong pool, jobject seeds, jint n,
                                                                              jobject pubkeys_out) {
  if (pool)
    return cg_pool_signers_load((cg_pool*)(intptr_t)pool, (const uint8_t*)ADDR(seeds), (uint32_t)n,
                                (uint8_t*)ADDR(pubkeys_out));
  return cg_signers_load((cg_ctx*)(intptr_t)ctx, (const uint8_t*)ADDR(seeds), (uint32_t)n, (uint8_t*)ADDR(pubkeys_out));
}

/* Crypto.doSign(keyPair, SignableData(id, metadata)) over many ids (NotaryService.sign, NotaryService.kt:77-80):
 * cg_sign_tx_ids (pool != 0: cg_pool_sign_tx_ids, the whole call on one healthy device, the next one on a
 * device fault). sigs_out: 64 bytes per request, status_out: one byte per request. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeSignTxIds(
    JNIEnv* env, jobject self, jlong ctx, jlong pool, jobject ids, jlong n_ids, jobject reqs, jlong n, jobject tmpls,
    jint n_tmpls, jobject arena, jlong arena_len, jobject sigs_out, jobject status_out) {
  if (pool)
    return cg_pool_sign_tx_ids((cg_pool*)(intptr_t)pool, (const uint8_t*)ADDR(ids), (uint64_t)n_ids,
                               (const cg_sign_req*)ADDR(reqs), (uint64_t)n, (const cg_signable_tmpl*)ADDR(tmpls),
                               (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena), (uint64_t)arena_len,
                               (uint8_t*)ADDR(sigs_out), (uint8_t*)ADDR(status_out), 0);
  return cg_sign_tx_ids((cg_ctx*)(intptr_t)ctx, (const uint8_t*)ADDR(ids), (uint64_t)n_ids,
                        (const cg_sign_req*)ADDR(reqs), (uint64_t)n, (const cg_signable_tmpl*)ADDR(tmpls),
                        (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena), (uint64_t)arena_len, (uint8_t*)ADDR(sigs_out),
                        (uint8_t*)ADDR(status_out));
}

/* The ECDSA signer set (cg_ec_signers_load; pool != 0: cg_pool_ec_signers_load, every device): a scheme byte and
 * 32 bytes of d per key; pubs_out 64 bytes (X || Y) and status_out one byte per key. The binding zeroes the
 * secrets buffer afterwards. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeLoadEcSigners(JNIEnv* env, jobject self, jlong ctx,
                                                                                jlong pool, jobject schemes,
                                                                                jobject secrets, jint n, jobject pubs_out,
                                                                                jobject status_out) {
  if (pool)
    return cg_pool_ec_signers_load((cg_pool*)(intptr_t)pool, (const uint8_t*)ADDR(schemes), (const uint8_t*)ADDR(secrets),
                                   (uint32_t)n, (uint8_t*)ADDR(pubs_out), (uint8_t*)ADDR(status_out));
  return cg_ec_signers_load((cg_ctx*)(intptr_t)ctx, (const uint8_t*)ADDR(schemes), (const uint8_t*)ADDR(secrets),
                            (uint32_t)n, (uint8_t*)ADDR(pubs_out), (uint8_t*)ADDR(status_out));
}

/* Crypto.doSign(keyPair, SignableData(id, metadata)) for ECDSA key pairs over many ids: cg_ec_sign_tx_ids (pool != 0:
 * cg_pool_ec_sign_tx_ids). nonces: 32 bytes per request, the candidate k the binding drew; sigs_out: 72 bytes per
 * request (the DER bytes, then zeros), sig_len_out and status_out: one byte per request. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeEcSignTxIds(
    JNIEnv* env, jobject self, jlong ctx, jlong pool, jobject ids, jlong n_ids, jobject reqs, jlong n, jobject tmpls,
    jint n_tmpls, jobject arena, jlong arena_len, jobject nonces, jobject sigs_out, jobject sig_len_out,
    jobject status_out) {
  if (pool)
    return cg_pool_ec_sign_tx_ids((cg_pool*)(intptr_t)pool, (const uint8_t*)ADDR(ids), (uint64_t)n_ids,
                                  (const cg_sign_req*)ADDR(reqs), (uint64_t)n, (const cg_signable_tmpl*)ADDR(tmpls),
                                  (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena), (uint64_t)arena_len,
                                  (const uint8_t*)ADDR(nonces), (uint8_t*)ADDR(sigs_out), (uint8_t*)ADDR(sig_len_out),
                                  (uint8_t*)ADDR(status_out), 0);
  return cg_ec_sign_tx_ids((cg_ctx*)(intptr_t)ctx, (const uint8_t*)ADDR(ids), (uint64_t)n_ids,
                           (const cg_sign_req*)ADDR(reqs), (uint64_t)n, (const cg_signable_tmpl*)ADDR(tmpls),
                           (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena), (uint64_t)arena_len,
                           (const uint8_t*)ADDR(nonces), (uint8_t*)ADDR(sigs_out), (uint8_t*)ADDR(sig_len_out),
                           (uint8_t*)ADDR(status_out));
}

/* The RSA signer set (cg_rsa_signers_load; pool != 0: cg_pool_rsa_signers_load, every device): n cg_rsa_signer
 * records over the big-endian numbers (n, p, q, dP, dQ, qInv) the binding wrote into `secrets`; status_out one
 * byte per key. The binding zeroes the secrets buffer afterwards. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeLoadRsaSigners(JNIEnv* env, jobject self, jlong ctx,
                                                                                 jlong pool, jobject signers, jint n,
                                                                                 jobject secrets, jlong secrets_len,
                                                                                 jobject status_out) {
  if (pool)
    return cg_pool_rsa_signers_load((cg_pool*)(intptr_t)pool, (const cg_rsa_signer*)ADDR(signers), (uint32_t)n,
                                    (const uint8_t*)ADDR(secrets), (uint64_t)secrets_len, (uint8_t*)ADDR(status_out));
  return cg_rsa_signers_load((cg_ctx*)(intptr_t)ctx, (const cg_rsa_signer*)ADDR(signers), (uint32_t)n,
                             (const uint8_t*)ADDR(secrets), (uint64_t)secrets_len, (uint8_t*)ADDR(status_out));
}

/* Crypto.doSign(keyPair, SignableData(id, metadata)) for RSA key pairs over many ids: cg_rsa_sign_tx_ids (pool != 0:
 * cg_pool_rsa_sign_tx_ids). salts: 32 bytes per request, the salt the binding drew; sigs_out: 512 bytes per request
 * (the signature, then zeros), sig_len_out: one uint16 and status_out: one byte per request. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeRsaSignTxIds(
    JNIEnv* env, jobject self, jlong ctx, jlong pool, jobject ids, jlong n_ids, jobject reqs, jlong n, jobject tmpls,
    jint n_tmpls, jobject arena, jlong arena_len, jobject salts, jobject sigs_out, jobject sig_len_out,
    jobject status_out) {
  if (pool)
    return cg_pool_rsa_sign_tx_ids((cg_pool*)(intptr_t)pool, (const uint8_t*)ADDR(ids), (uint64_t)n_ids,
                                   (const cg_sign_req*)ADDR(reqs), (uint64_t)n, (const cg_signable_tmpl*)ADDR(tmpls),
                                   (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena), (uint64_t)arena_len,
                                   (const uint8_t*)ADDR(salts), (uint8_t*)ADDR(sigs_out), (uint16_t*)ADDR(sig_len_out),
                                   (uint8_t*)ADDR(status_out), 0);
  return cg_rsa_sign_tx_ids((cg_ctx*)(intptr_t)ctx, (const uint8_t*)ADDR(ids), (uint64_t)n_ids,
                            (const cg_sign_req*)ADDR(reqs), (uint64_t)n, (const cg_signable_tmpl*)ADDR(tmpls),
                            (uint32_t)n_tmpls, (const uint8_t*)ADDR(arena), (uint64_t)arena_len,
                            (const uint8_t*)ADDR(salts), (uint8_t*)ADDR(sigs_out), (uint16_t*)ADDR(sig_len_out),
                            (uint8_t*)ADDR(status_out));
}

/* Crypto.deriveKeyPair(privateKey, seed) over many seeds (Crypto.kt:646-771): cg_derive_keys (pool != 0:
 * cg_pool_derive_keys, the whole call on one healthy device, the next one on a device fault). parents:
 * cg_derive_parent records over keyData the binding wrote into the arena; secrets_out 32 bytes, pubs_out
 * 64 bytes, status_out and retries_out one byte per request. The binding zeroes the arena and the
 * secrets buffer afterwards. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeDeriveKeys(
    JNIEnv* env, jobject self, jlong ctx, jlong pool, jobject parents, jint n_parents, jobject reqs, jlong n,
    jobject arena, jlong arena_len, jobject secrets_out, jobject pubs_out, jobject status_out, jobject retries_out) {
  if (pool)
    return cg_pool_derive_keys((cg_pool*)(intptr_t)pool, (const cg_derive_parent*)ADDR(parents), (uint32_t)n_parents,
                               (const cg_derive_req*)ADDR(reqs), (uint64_t)n, (const uint8_t*)ADDR(arena),
                               (uint64_t)arena_len, (uint8_t*)ADDR(secrets_out), (uint8_t*)ADDR(pubs_out),
                               (uint8_t*)ADDR(status_out), (uint8_t*)ADDR(retries_out), 0);
  return cg_derive_keys((cg_ctx*)(intptr_t)ctx, (const cg_derive_parent*)ADDR(parents), (uint32_t)n_parents,
                        (const cg_derive_req*)ADDR(reqs), (uint64_t)n, (const uint8_t*)ADDR(arena), (uint64_t)arena_len,
                        (uint8_t*)ADDR(secrets_out), (uint8_t*)ADDR(pubs_out), (uint8_t*)ADDR(status_out),
                        (uint8_t*)ADDR(retries_out));
}

/* Private key -> public key for n 32-byte private keys of one scheme: cg_public_keys / cg_pool_public_keys. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativePublicKeys(JNIEnv* env, jobject self, jlong ctx,
                                                                             jlong pool, jint scheme, jobject secrets,
                                                                             jlong n, jobject pubs_out,
                                                                             jobject status_out) {
  if (pool)
    return cg_pool_public_keys((cg_pool*)(intptr_t)pool, (uint32_t)scheme, (const uint8_t*)ADDR(secrets), (uint64_t)n,
                               (uint8_t*)ADDR(pubs_out), (uint8_t*)ADDR(status_out), 0);
  return cg_public_keys((cg_ctx*)(intptr_t)ctx, (uint32_t)scheme, (const uint8_t*)ADDR(secrets), (uint64_t)n,
                        (uint8_t*)ADDR(pubs_out), (uint8_t*)ADDR(status_out));
}

/* A direct buffer the node keeps across calls: pinned once (cg_host_register), so its bytes reach
 * every device by DMA without the runtime's CPU staging copy. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeHostRegister(JNIEnv* env, jobject self,
                                                                               jobject buf, jlong len) {
  return cg_host_register(ADDR(buf), (uint64_t)len);
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_CryptoBatch_nativeHostUnregister(JNIEnv* env, jobject self,
                                                                                 jobject buf) {
  return cg_host_unregister(ADDR(buf));
}
