// core/src/main/kotlin/net/corda/core/crypto/CryptoBatch.kt (new file in the Corda tree).
// The JVM side of libcordagpu.so (include/cordagpu.h) through jvm/jni/cordagpu_jni.c. Not compiled
// in this repository (no JDK / Kotlin compiler in its image); corda_amd/ is the Python mirror of the
// same calls, and the GPU tests drive that mirror. tests/test_jvm_binding.py checks this file's
// status mapping, packing constants and config keys against the Python mirror and the C header.
package net.corda.core.crypto

import com.codahale.metrics.Gauge
import com.codahale.metrics.MetricRegistry
import com.typesafe.config.Config
import net.corda.core.crypto.composite.CompositeKey
import net.corda.core.serialization.serialize
import net.corda.core.transactions.SignedTransaction
import net.i2p.crypto.eddsa.EdDSAPrivateKey
import net.i2p.crypto.eddsa.EdDSAPublicKey
import net.i2p.crypto.eddsa.spec.EdDSANamedCurveSpec
import net.i2p.crypto.eddsa.spec.EdDSAPrivateKeySpec
import net.i2p.crypto.eddsa.spec.EdDSAPublicKeySpec
import org.bouncycastle.jcajce.provider.asymmetric.ec.BCECPrivateKey
import org.bouncycastle.jcajce.provider.asymmetric.ec.BCECPublicKey
import org.bouncycastle.jce.provider.BouncyCastleProvider
import org.bouncycastle.jce.spec.ECParameterSpec
import org.bouncycastle.jce.spec.ECPrivateKeySpec
import org.bouncycastle.jce.spec.ECPublicKeySpec
import java.math.BigInteger
import java.nio.ByteBuffer
import java.nio.ByteOrder
import java.security.InvalidKeyException
import java.security.KeyPair
import java.security.PrivateKey
import java.security.PublicKey
import java.security.SecureRandom
import java.security.SignatureException
import java.security.interfaces.RSAPrivateCrtKey
import java.security.interfaces.RSAPublicKey
import java.util.concurrent.TimeUnit
import java.util.concurrent.atomic.AtomicInteger
import java.util.concurrent.locks.ReentrantLock
import java.util.concurrent.locks.ReentrantReadWriteLock
import kotlin.concurrent.read
import kotlin.concurrent.withLock
import kotlin.concurrent.write

data class BatchItem(val publicKey: PublicKey, val signatureData: ByteArray, val clearData: ByteArray)

/**
 * The engine's node.conf block (INTEGRATION.md §5), beside the reference's verifierType
 * (NodeConfiguration.kt:33,98-101):
 *
 *   gpuVerifier { devices = [0, 1, 2, 3, 4, 5, 6, 7], minBatch = 4096, chunkItems = 0, hostThreads = 0,
 *                 tableBytesMax = 0, gpuRsa = false }
 *
 * devices: HIP ordinals this process drives (one: a cg_ctx; several: a cg_pool sharding every batch:
 *   every entry point works with either, see CryptoBatch.withHandles).
 * minBatch: batches with fewer signatures than this never leave the JVM (Crypto.doVerify per
 *   signature, the reference's own serial path): a GPU call has a fixed cost of a few ms.
 * chunkItems: cg_config.chunk_items (0: the library's default).
 * hostThreads: cg_config.host_threads, host threads of this process's scans (0: the cgroup CPU quota
 *   divided by the contexts the process opens).
 * tableBytesMax: cg_config.table_bytes_max, HBM per device for the constant fixed-base tables (0:
 *   automatic: ~91 GB when the device has room, ~25 / ~6.9 GB when other processes share it; a node
 *   that runs several verifier processes per GPU sets e.g. 26000000000).
 * gpuRsa: CG_FLAG_RSA in cg_config.flags: RSA_SHA256 (SHA256WITHRSAANDMGF1) signatures whose key the
 *   engine's strict decode accepts (canonical X.509, 1024..4096-bit odd modulus, e < 2^32) are verified
 *   on the GPU; everything else still comes back CG_UNSUPPORTED and goes to Crypto.doVerify (raiseForStatus).
 */
data class GpuVerifierConfig(val devices: IntArray = intArrayOf(0), val minBatch: Int = 4096,
                             val chunkItems: Long = 0, val hostThreads: Int = 0, val tableBytesMax: Long = 0,
                             val gpuRsa: Boolean = false) {
    init {
        require(devices.isNotEmpty() && devices.all { it >= 0 }) { "gpuVerifier.devices: at least one ordinal >= 0" }
        require(minBatch >= 0 && chunkItems >= 0 && hostThreads >= 0 && tableBytesMax >= 0) { "gpuVerifier: negative setting" }
    }

    companion object {
        fun fromConfig(c: Config): GpuVerifierConfig {
            val g = c.getConfig("gpuVerifier")
            fun <T> opt(key: String, get: (String) -> T, def: T) = if (g.hasPath(key)) get(key) else def
            return GpuVerifierConfig(
                devices = opt("devices", { g.getIntList(it).toIntArray() }, intArrayOf(0)),
                minBatch = opt("minBatch", g::getInt, 4096),
                chunkItems = opt("chunkItems", g::getLong, 0L),
                hostThreads = opt("hostThreads", g::getInt, 0),
                tableBytesMax = opt("tableBytesMax", g::getLong, 0L),
                gpuRsa = g.hasPath("gpuRsa") && g.getBoolean("gpuRsa"))
        }
    }
}

object CryptoBatch {
    init { System.loadLibrary("cordagpu_jni") }           // links libcordagpu.so

    private const val CG_FLAG_RSA = 2                     // include/cordagpu.h cg_config.flags
    private external fun nativeOpen(device: Int, chunkItems: Long, hostThreads: Int, tableBytesMax: Long, flags: Int): Long
    private external fun nativeOpenPool(devices: IntArray, chunkItems: Long, hostThreads: Int, tableBytesMax: Long,
                                        flags: Int): Long
    private external fun nativeClose(ctx: Long, pool: Long)
    private external fun nativeVerify(ctx: Long, pool: Long, keys: ByteBuffer, nKeys: Int, items: ByteBuffer, nItems: Long,
                                      arena: ByteBuffer, arenaLen: Long, mode: Int, status: ByteBuffer,
                                      stats: ByteBuffer): Int
    private external fun nativeVerifyTransactions(ctx: Long, pool: Long, txs: ByteBuffer, nTx: Long, comps: ByteBuffer, nComps: Long,
                                                  keys: ByteBuffer, nKeys: Int, sigs: ByteBuffer, nSigs: Long,
                                                  tmpls: ByteBuffer, nTmpls: Int, arena: ByteBuffer, arenaLen: Long,
                                                  mode: Int, idsOut: ByteBuffer, txStatusOut: ByteBuffer,
                                                  sigStatusOut: ByteBuffer): Int
    /** cg_(pool_)verify_tx_signatures_packed: the 12-byte table (cg_txsig_packed: tx_idx, key_idx,
     *  sig_len, tmpl) and the signatures back to back, each at a 4-byte boundary, in their own buffer
     *  (round 6; the 24-byte cg_txsig form shipped ~12 B more per signature). */
    private external fun nativeVerifyTxSignaturesPacked(ctx: Long, pool: Long, keys: ByteBuffer, nKeys: Int,
                                                        ids: ByteBuffer, nIds: Long, sigs: ByteBuffer, nSigs: Long,
                                                        sigBytes: ByteBuffer, sigBytesLen: Long, tmpls: ByteBuffer,
                                                        nTmpls: Int, arena: ByteBuffer, arenaLen: Long, mode: Int,
                                                        status: ByteBuffer, stats: ByteBuffer): Int
    /** cg_host_register / cg_host_unregister: a direct buffer the node keeps for many calls, pinned
     *  once so that its bytes reach the device by DMA without the runtime's CPU staging copy. */
    private external fun nativeVerifyRequiredPacked(ctx: Long, pool: Long, keys: ByteBuffer, nKeys: Int,
                                                    ids: ByteBuffer, nIds: Long, sigs: ByteBuffer, nSigs: Long,
                                                    sigBytes: ByteBuffer, sigBytesLen: Long, tmpls: ByteBuffer,
                                                    nTmpls: Int, arena: ByteBuffer, arenaLen: Long, mode: Int,
                                                    keyClass: ByteBuffer, checks: ByteBuffer, nTx: Long,
                                                    reqs: ByteBuffer, nReqs: Int, nodes: ByteBuffer, nNodes: Int,
                                                    status: ByteBuffer?, verdicts: ByteBuffer, reqStatus: ByteBuffer): Int
    /** cg_(pool_)signers_load: EdDSAPrivateKeySpec(seed) per 32-byte seed, the context's (every pool
     *  device's) signer set; pubkeysOut receives each key's Abyte. */
    private external fun nativeLoadSigners(ctx: Long, pool: Long, seeds: ByteBuffer, n: Int, pubkeysOut: ByteBuffer): Int
    /** cg_(pool_)sign_tx_ids: Crypto.doSign(keyPair, SignableData(id, metadata)) per 8-byte request
     *  (cg_sign_req: tx_idx, signer, tmpl); 64 signature bytes and one status byte per request. */
    private external fun nativeSignTxIds(ctx: Long, pool: Long, ids: ByteBuffer, nIds: Long, reqs: ByteBuffer, n: Long,
                                         tmpls: ByteBuffer, nTmpls: Int, arena: ByteBuffer, arenaLen: Long,
                                         sigsOut: ByteBuffer, statusOut: ByteBuffer): Int
    /** cg_(pool_)ec_signers_load: the ECDSA signer set (separate from the Ed25519 one): a scheme byte (2 / 3)
     *  and 32 bytes of d, big-endian, per key; pubsOut receives X || Y, statusOut the load status. */
    private external fun nativeLoadEcSigners(ctx: Long, pool: Long, schemes: ByteBuffer, secrets: ByteBuffer, n: Int,
                                             pubsOut: ByteBuffer, statusOut: ByteBuffer): Int
    /** cg_(pool_)ec_sign_tx_ids: Crypto.doSign(keyPair, SignableData(id, metadata)) for ECDSA key pairs per 8-byte
     *  request, with one 32-byte candidate k per request (nonces); a 72-byte slot (the DER bytes, then zeros), a
     *  length byte and a status byte per request. */
    private external fun nativeEcSignTxIds(ctx: Long, pool: Long, ids: ByteBuffer, nIds: Long, reqs: ByteBuffer, n: Long,
                                           tmpls: ByteBuffer, nTmpls: Int, arena: ByteBuffer, arenaLen: Long,
                                           nonces: ByteBuffer, sigsOut: ByteBuffer, sigLenOut: ByteBuffer,
                                           statusOut: ByteBuffer): Int
    /** cg_(pool_)rsa_signers_load: the RSA signer set (the third one): n 52-byte cg_rsa_signer records (offset and
     *  length of n, p, q, dP, dQ, qInv in `secrets`, then e); statusOut receives the load status per key. */
    private external fun nativeLoadRsaSigners(ctx: Long, pool: Long, signers: ByteBuffer, n: Int, secrets: ByteBuffer,
                                              secretsLen: Long, statusOut: ByteBuffer): Int
    /** cg_(pool_)rsa_sign_tx_ids: Crypto.doSign(keyPair, SignableData(id, metadata)) for RSA key pairs per 8-byte
     *  request, with one 32-byte salt per request (salts); a 512-byte slot (the signature, then zeros), a 16-bit
     *  length and a status byte per request. */
    private external fun nativeRsaSignTxIds(ctx: Long, pool: Long, ids: ByteBuffer, nIds: Long, reqs: ByteBuffer, n: Long,
                                            tmpls: ByteBuffer, nTmpls: Int, arena: ByteBuffer, arenaLen: Long,
                                            salts: ByteBuffer, sigsOut: ByteBuffer, sigLenOut: ByteBuffer,
                                            statusOut: ByteBuffer): Int
    /** cg_(pool_)derive_keys: Crypto.deriveKeyPair(privateKey, seed) per 16-byte request (cg_derive_req: seed
     *  offset and length, parent) over 16-byte parents (cg_derive_parent: keyData offset and length, scheme);
     *  32 secret bytes, 64 public bytes, a status byte and a rehash count per request. */
    private external fun nativeDeriveKeys(ctx: Long, pool: Long, parents: ByteBuffer, nParents: Int, reqs: ByteBuffer, n: Long,
                                          arena: ByteBuffer, arenaLen: Long, secretsOut: ByteBuffer, pubsOut: ByteBuffer,
                                          statusOut: ByteBuffer, retriesOut: ByteBuffer): Int
    /** cg_(pool_)public_keys: the public key of each 32-byte private key of one scheme. */
    private external fun nativePublicKeys(ctx: Long, pool: Long, scheme: Int, secrets: ByteBuffer, n: Long,
                                          pubsOut: ByteBuffer, statusOut: ByteBuffer): Int
    private external fun nativeHostRegister(buf: ByteBuffer, len: Long): Int
    private external fun nativeHostUnregister(buf: ByteBuffer): Int

    const val MODE_DOVERIFY = 0
    const val MODE_ISVALID = 1
    private const val KEY_SPKI = 1

    // include/cordagpu.h per-item verdicts
    const val CG_VALID = 0
    const val CG_INVALID = 1
    const val CG_SIG_MALFORMED = 2
    const val CG_KEY_INVALID = 3
    const val CG_UNSUPPORTED = 4
    const val CG_EMPTY = 5
    const val CG_NOT_RUN = 255
    // key derivation (cg_derive_keys / cg_public_keys)
    const val CG_DERIVE_HOST = 6
    const val CG_DERIVE_BAD_PARENT = 7
    const val CG_KEY_REJECTED = 8
    // include/cordagpu.h return codes
    // per-transaction verdicts (include/cordagpu.h cg_tx_verdict.flags, req_status codes, struct sizes)
    const val CG_TXV_SPAN_BAD = 1
    const val CG_TXV_REQ_HOST = 2
    const val CG_TXV_COMPOSITE_SIGNER = 4
    const val CG_REQ_FULFILLED = 0
    const val CG_REQ_MISSING = 1
    const val CG_REQ_HOST = 2
    const val CG_REQ_BAD = 255
    private const val TX_CHECK_BYTES = 24
    private const val REQ_NODE_BYTES = 16
    private const val TX_VERDICT_BYTES = 8
    private const val NO_BAD = -1                          // cg_tx_verdict.first_bad == 0xFFFFFFFF

    private const val CG_OK = 0
    private const val CG_ERR_DEVICE = -2

    // cg_item.sig_len / cg_txsig.sig_len are 16-bit. A longer JVM signature is packed as a short
    // surrogate with the verdict the JVM gives the real bytes (corda_amd/batch.py sig_field):
    // Ed25519: length != 64 -> SIG_MALFORMED; ECDSA: a canonical SEQUENCE{INTEGER, INTEGER} has an
    // INTEGER of 32k+ content bytes, out of [1, n-1] -> INVALID; anything else fails BC's decode.
    const val SIG_LEN_MAX = 0xFFFF
    private val SIG_SURROGATE_MALFORMED = byteArrayOf(0x00)
    private val SIG_SURROGATE_INVALID = byteArrayOf(0x30, 0x06, 0x02, 0x01, 0x00, 0x02, 0x01, 0x01)

    // cg_stats: n_items, n_keys (u64), ms_h2d, ms_key_prep, ms_verify, ms_d2h, ms_total (f64)
    private const val STATS_BYTES = 56

    @Volatile private var config = GpuVerifierConfig()
    // the native handles (exactly one non-zero while open: ctx for one device, pool for several). Every
    // native call holds the read lock from reading them until it returns; open and close() take the
    // write lock, so close() waits for the calls in flight and never frees a handle under one (ADVICE r5)
    private val rw = ReentrantReadWriteLock()
    private var ctx: Long = 0
    private var pool: Long = 0

    // Metrics named like the reference's verifier service (OutOfProcessTransactionVerifierService.kt:35-46)
    private fun metric(name: String) = "CryptoBatch.$name"
    @Volatile private var metrics: MetricRegistry? = null
    private val inFlight = AtomicInteger(0)

    /** Applies node.conf's gpuVerifier block; takes effect at the next open (close() first to re-open). */
    fun configure(c: GpuVerifierConfig) { config = c }

    /** Feeds a node's MetricRegistry: a timer per batch, success / failure meters per signature, the
     *  batches in flight, and the device's stage times from cg_stats. */
    fun registerMetrics(registry: MetricRegistry) {
        registry.register(metric("VerificationsInFlight"), Gauge { inFlight.get() })
        metrics = registry
    }

    /** Runs one native call with the open handles (ctx, pool), opening them on first use, under the
     *  read lock: close() cannot free them until the call has returned. Every entry point calls the
     *  engine through here, whichever of ctx (one device) / pool (several) is open. */
    private inline fun <T> withHandles(call: (Long, Long) -> T): T {
        while (true) {
            rw.read { if (ctx != 0L || pool != 0L) return call(ctx, pool) }
            rw.write {
                if (ctx == 0L && pool == 0L) {
                    val c = config
                    val flags = if (c.gpuRsa) CG_FLAG_RSA else 0
                    if (c.devices.size == 1) ctx = nativeOpen(c.devices[0], c.chunkItems, c.hostThreads, c.tableBytesMax, flags)
                    else pool = nativeOpenPool(c.devices, c.chunkItems, c.hostThreads, c.tableBytesMax, flags)
                }
            }
        }
    }

    /** Releases the device context / pool (cg_close / cg_pool_close) once the calls in flight have
     *  returned (write lock). A later call opens a new one. */
    fun close() {
        rw.write {
            if (ctx != 0L || pool != 0L) nativeClose(ctx, pool)   // cg_close zeroes the signer store
            ctx = 0
            pool = 0
            signerLock.withLock { signerHandle = 0; ecSignerHandle = 0 }
        }
    }

    /** The C ABI's failure contract (include/cordagpu.h): CG_ERR_DEVICE leaves exactly the items no
     *  device could run as CG_NOT_RUN (a pool has already re-run a failed device's shard on the healthy
     *  ones). Those items, and only those, go to the engine once more through `rerun` (given their
     *  indices, it returns their new statuses); what is still NOT_RUN after that stays NOT_RUN, and
     *  raiseForStatus verifies it with the JVM's own Crypto.doVerify. Any other non-zero code is the
     *  caller's input, not the device: thrown. Never throws for the whole batch on a device fault. */
    private fun requeueNotRun(rc: Int, what: String, status: ByteArray, rerun: ((IntArray) -> ByteArray)?) {
        if (rc == CG_OK) return
        check(rc == CG_ERR_DEVICE) { "$what failed: $rc" }
        val todo = status.indices.filter { (status[it].toInt() and 0xff) == CG_NOT_RUN }.toIntArray()
        if (todo.isEmpty() || rerun == null) return
        val again = try { rerun(todo) } catch (e: IllegalStateException) { return }   // still no device: stay NOT_RUN
        for ((k, i) in todo.withIndex()) status[i] = again[k]
    }

    private inline fun <T> timed(n: Int, body: () -> T): T {
        val m = metrics
        val t = m?.timer(metric("Verification.Duration"))?.time()
        inFlight.incrementAndGet()
        try {
            return body()
        } finally {
            inFlight.decrementAndGet()
            t?.stop()
            m?.meter(metric("Verification.Signatures"))?.mark(n.toLong())
        }
    }

    private fun record(stats: ByteBuffer, status: ByteArray) {
        val m = metrics ?: return
        val ok = status.count { it.toInt() == CG_VALID }
        m.meter(metric("Verification.Success")).mark(ok.toLong())
        m.meter(metric("Verification.Failure")).mark((status.size - ok).toLong())
        // a pool call fills no cg_stats (n_items stays 0): no device stage times to report (ADVICE r5)
        if (stats.getLong(0) == 0L) return
        val names = arrayOf("Device.H2D", "Device.KeyPrep", "Device.Verify", "Device.D2H", "Device.Total")
        for ((i, n) in names.withIndex())
            m.timer(metric(n)).update((stats.getDouble(16 + 8 * i) * 1e6).toLong(), TimeUnit.NANOSECONDS)
    }

    private fun direct(n: Int): ByteBuffer = ByteBuffer.allocateDirect(maxOf(n, 1)).order(ByteOrder.LITTLE_ENDIAN)
    private fun ByteBuffer.align4() { while (position() % 4 != 0) put(0) }

    /** The bytes to pack for a signature: itself, or its surrogate past the 16-bit length field. */
    fun sigField(scheme: SignatureScheme, sig: ByteArray): ByteArray = when {
        sig.size <= SIG_LEN_MAX -> sig
        (scheme == Crypto.ECDSA_SECP256K1_SHA256 || scheme == Crypto.ECDSA_SECP256R1_SHA256) && derIsTwoIntegers(sig) ->
            SIG_SURROGATE_INVALID
        else -> SIG_SURROGATE_MALFORMED
    }

    /** (length, next index) of a minimal definite DER length at b[i], or null (batch.py _der_len_at). */
    private fun derLenAt(b: ByteArray, i: Int): Pair<Int, Int>? {
        if (i >= b.size) return null
        val l0 = b[i].toInt() and 0xff
        if (l0 < 0x80) return l0 to i + 1
        val nb = l0 and 0x7f
        if (nb == 0 || nb > 4 || i + 1 + nb > b.size || b[i + 1].toInt() == 0) return null
        var v = 0L
        for (k in 0 until nb) v = (v shl 8) or (b[i + 1 + k].toLong() and 0xff)
        if (v < 0x80 || v > Int.MAX_VALUE) return null
        return v.toInt() to i + 1 + nb
    }

    /** Exactly the canonical DER of SEQUENCE{INTEGER, INTEGER} (batch.py der_is_two_integers). */
    fun derIsTwoIntegers(b: ByteArray): Boolean {
        if (b.size < 2 || b[0].toInt() != 0x30) return false
        val r = derLenAt(b, 1) ?: return false
        if (r.second.toLong() + r.first != b.size.toLong()) return false
        var i = r.second
        var n = 0
        while (i < b.size) {
            if (b[i].toInt() != 0x02) return false
            val (ln, j) = derLenAt(b, i + 1) ?: return false
            if (ln == 0 || j.toLong() + ln > b.size) return false
            if (ln > 1) {
                val b0 = b[j].toInt() and 0xff
                val b1 = b[j + 1].toInt() and 0xff
                if ((b0 == 0 && b1 < 0x80) || (b0 == 0xff && b1 >= 0x80)) return false
            }
            i = j + ln
            n++
        }
        return n == 2
    }

    /** cg_key table + arena prefix for the distinct keys, in first-use order. */
    private class Keys(keys: Collection<PublicKey>, arena: ByteBuffer) {
        val index = LinkedHashMap<PublicKey, Int>()
        val schemes = ArrayList<SignatureScheme>()
        val table: ByteBuffer
        init {
            keys.forEach { index.getOrPut(it) { index.size } }
            table = ByteBuffer.allocateDirect(16 * maxOf(index.size, 1)).order(ByteOrder.LITTLE_ENDIAN)
            for (k in index.keys) {
                val scheme = Crypto.findSignatureScheme(k)
                schemes.add(scheme)
                // cg_key.len is 16-bit; no key of a GPU scheme is that long, so one byte (which fails
                // to decode, as the real key would) stands in (batch.py Builder.key)
                val enc = k.encoded.let { if (it.size > SIG_LEN_MAX) byteArrayOf(0) else it }
                arena.align4()
                table.putLong(arena.position().toLong()).putShort(enc.size.toShort())
                    .put(scheme.schemeNumberID.toByte()).put(KEY_SPKI.toByte()).putInt(0)
                arena.put(enc)
            }
        }
    }

    /** Batch overload of Crypto.doVerify / isValid: one status byte per item (include/cordagpu.h).
     *  One device or several (the pool shards the items); on a device fault the items left NOT_RUN are
     *  re-queued once (requeueNotRun), and any still NOT_RUN reach the caller as NOT_RUN. */
    fun verifyBatch(items: List<BatchItem>, mode: Int = MODE_DOVERIFY): ByteArray = timed(items.size) {
        verifyItems(items, mode, requeue = true)
    }

    private fun verifyItems(items: List<BatchItem>, mode: Int, requeue: Boolean): ByteArray {
        val arena = direct(items.sumOf { minOf(it.signatureData.size, SIG_LEN_MAX) + it.clearData.size + 8 } +
                           items.map { it.publicKey }.distinct().sumOf { it.encoded.size + 4 } + 16)
        val keys = Keys(items.map { it.publicKey }, arena)
        val rec = direct(32 * items.size)
        for (it in items) {
            val ki = keys.index[it.publicKey]!!
            val sig = sigField(keys.schemes[ki], it.signatureData)
            arena.align4()
            val sigOff = arena.position().toLong(); arena.put(sig)
            arena.align4()
            val msgOff = arena.position().toLong(); arena.put(it.clearData)
            rec.putLong(sigOff).putLong(msgOff).putInt(it.clearData.size).putInt(ki)
               .putShort(sig.size.toShort()).putShort(0).putInt(0)
        }
        val status = direct(items.size)
        val stats = direct(STATS_BYTES)
        val rc = withHandles { c, p ->
            nativeVerify(c, p, keys.table, keys.index.size, rec, items.size.toLong(), arena, arena.position().toLong(),
                         mode, status, stats)
        }
        val st = ByteArray(items.size).also { status.get(it) }
        requeueNotRun(rc, "cg_verify_batch", st,
                      if (requeue) { todo -> verifyItems(todo.map { items[it] }, mode, requeue = false) } else null)
        record(stats, st)
        return st
    }

    /** Crypto.doVerify for every item, throwing what the first failing item's serial call throws.
     *  Below gpuVerifier.minBatch the items never leave the JVM. */
    fun doVerifyAll(items: List<BatchItem>) {
        if (items.size < config.minBatch) {
            for (it in items) Crypto.doVerify(it.publicKey, it.signatureData, it.clearData)
            return
        }
        val st = verifyBatch(items, MODE_DOVERIFY)
        for ((i, it) in items.withIndex()) if (st[i].toInt() != CG_VALID) raiseForStatus(st[i], it)
    }

    /** SignableData(id, metadata) = prefix || id || suffix: found by serialising with two ids that
     *  differ in every byte (0^32 and 0xFF^32) and taking the first differing offset, then checking
     *  that the bytes around the id agree (a prefix that happens to end in 0x00, or an earlier run of
     *  zero bytes, cannot shift the split). Mirrors corda_amd/signable.py:template. */
    fun signableTemplate(m: SignatureMetadata): Pair<ByteArray, ByteArray> {
        val a = SignableData(SecureHash.zeroHash, m).serialize().bytes
        val b = SignableData(SecureHash.SHA256(ByteArray(32) { 0xFF.toByte() }), m).serialize().bytes
        check(a.size == b.size) { "SignableData serialisation depends on the id's value" }
        val at = a.indices.first { a[it] != b[it] }
        check(at + 32 <= a.size && (at until at + 32).all { a[it] == 0.toByte() && b[it] == 0xFF.toByte() } &&
              (at + 32 until a.size).all { a[it] == b[it] }) { "id not found as 32 contiguous bytes" }
        return a.copyOfRange(0, at) to a.copyOfRange(at + 32, a.size)
    }

    /** Batch Crypto.doVerify(txId, TransactionSignature) (Crypto.kt:499-502) for every signature of
     *  every transaction, SignableData spliced on the device: one status byte per signature, in order.
     *  With several devices configured the call shards over the pool (cg_pool_verify_tx_signatures). On
     *  a device fault only the signatures left NOT_RUN are re-queued (requeueNotRun). */
    fun verifyTxSignatures(txs: List<Pair<SecureHash, List<TransactionSignature>>>, mode: Int = MODE_DOVERIFY): ByteArray {
        val all = txs.flatMap { it.second }
        return timed(all.size) { verifySigs(txs, mode, requeue = true) }
    }

    private fun verifySigs(txs: List<Pair<SecureHash, List<TransactionSignature>>>, mode: Int, requeue: Boolean): ByteArray {
        val all = txs.flatMap { it.second }
        val metas = LinkedHashMap<SignatureMetadata, Int>()
        all.forEach { metas.getOrPut(it.signatureMetadata) { metas.size } }
        val split = metas.keys.map { signableTemplate(it) }
        // arena: key and template bytes; the signatures go to their own stream (cg_txsig_packed, round 6:
        // 12 bytes of table per signature instead of the 24-byte cg_txsig, no offsets)
        val arena = direct(split.sumOf { it.first.size + it.second.size + 8 } +
                           all.map { it.by }.distinct().sumOf { it.encoded.size + 4 } + 16)
        val keys = Keys(all.map { it.by }, arena)
        val tmpls = direct(24 * split.size)
        for ((pre, suf) in split) {
            arena.align4(); val p = arena.position().toLong(); arena.put(pre)
            arena.align4(); val s = arena.position().toLong(); arena.put(suf)
            tmpls.putLong(p).putLong(s).putInt(pre.size).putInt(suf.size)
        }
        val ids = direct(32 * txs.size)
        val sigs = direct(12 * all.size)
        val stream = direct(all.sumOf { minOf(it.bytes.size, SIG_LEN_MAX) + 4 })
        txs.forEachIndexed { t, (id, list) ->
            ids.put(id.bytes)
            for (sig in list) {
                val ki = keys.index[sig.by]!!
                val bytes = sigField(keys.schemes[ki], sig.bytes)
                stream.put(bytes).align4()          // signature i at the 4-byte-aligned end of signature i - 1
                sigs.putInt(t).putInt(ki).putShort(bytes.size.toShort())
                    .putShort(metas[sig.signatureMetadata]!!.toShort())
            }
        }
        val status = direct(all.size)
        val stats = direct(STATS_BYTES)
        val rc = withHandles { c, p ->
            nativeVerifyTxSignaturesPacked(c, p, keys.table, keys.index.size, ids, txs.size.toLong(), sigs,
                                           all.size.toLong(), stream, stream.position().toLong(), tmpls, split.size,
                                           arena, arena.position().toLong(), mode, status, stats)
        }
        val st = ByteArray(all.size).also { status.get(it) }
        // the re-queue: the NOT_RUN signatures, each as a one-signature transaction of its own id
        val owner = txs.flatMap { (id, list) -> list.map { id to it } }
        requeueNotRun(rc, "cg_verify_tx_signatures_packed", st,
                      if (requeue) { todo -> verifySigs(todo.map { owner[it].first to listOf(owner[it].second) }, mode, false) }
                      else null)
        record(stats, st)
        return st
    }

    // ---- Ed25519 signing (include/cordagpu.h, "Ed25519 signing"). The signer set lives in the open context
    // (every device of the pool); signerHandle is the handle it was loaded into, so a context opened
    // after close() gets the set again before its first sign call.
    private const val CG_SIGNERS_MAX = 65535
    private val signerLock = ReentrantLock()
    private var signerKeys: List<KeyPair> = emptyList()
    private var signerHandle = 0L

    private fun isEd25519(k: KeyPair) = Crypto.findSignatureScheme(k.private) == Crypto.EDDSA_ED25519_SHA512 &&
        Crypto.findSignatureScheme(k.public) == Crypto.EDDSA_ED25519_SHA512

    /** The public half is the private half's A: checked on the JVM before a pair joins the signer set, so a
     *  pair that does not belong together never reaches it (ensureSigners checks the device's Abyte too). */
    private fun requireAligned(k: KeyPair) =
        require((k.private as EdDSAPrivateKey).abyte.contentEquals((k.public as EdDSAPublicKey).abyte)) {
            "the public key of this pair is not the private key's"
        }

    /** The notary's (node's) own Ed25519 key pairs, the keys PersistentKeyManagementService holds in this
     *  process (PersistentKeyManagementService.kt:84-95), as the engine's signer set: loaded into the
     *  device at the next signAll. Key pairs of other schemes are not accepted here; signAll signs with
     *  them on the JVM. */
    fun loadSigners(keyPairs: List<KeyPair>) {
        require(keyPairs.size in 1..CG_SIGNERS_MAX) { "1..$CG_SIGNERS_MAX signers" }
        require(keyPairs.all { isEd25519(it) }) { "the GPU signer takes EDDSA_ED25519_SHA512 key pairs only" }
        keyPairs.forEach { requireAligned(it) }
        signerLock.withLock {
            signerKeys = keyPairs.toList()
            signerHandle = 0
        }
    }

    /** With signerLock held, inside withHandles: the set is in the open context. The device returns each
     *  key's Abyte, and a pair whose public half is another key's is refused here, the way
     *  Crypto.doSign(keyPair, signableData) refuses a misaligned pair (Crypto.kt:416-419). The seed
     *  buffer is zeroed before it is released. */
    private fun ensureSigners(c: Long, p: Long): Boolean {
        val h = if (c != 0L) c else p
        if (signerHandle == h) return true
        val n = signerKeys.size
        val seeds = direct(32 * n)
        val pubs = direct(32 * n)
        val rc = try {
            signerKeys.forEach { seeds.put((it.private as EdDSAPrivateKey).seed) }
            nativeLoadSigners(c, p, seeds, n, pubs)
        } finally {
            for (i in 0 until seeds.capacity()) seeds.put(i, 0)
        }
        if (rc != CG_OK) return false
        val bad = signerKeys.indices.filter { i ->
            val abyte = ByteArray(32).also { pubs.position(32 * i); pubs.get(it) }
            !abyte.contentEquals((signerKeys[i].public as EdDSAPublicKey).abyte)
        }
        if (bad.isNotEmpty()) {
            // the offending pairs leave the set, and the next sign call loads what remains (signerHandle
            // stays 0), so one bad pair fails its own call and no later one
            signerKeys = signerKeys.filterIndexed { i, _ -> i !in bad }
            signerHandle = 0
            throw IllegalArgumentException("signer ${bad.first()}: the public key is not the private key's")
        }
        signerHandle = h
        return true
    }

    /** NotaryService.sign(txId) (NotaryService.kt:77-80; BFTSMaRt.kt:249-255) for many ids in one call:
     *  Crypto.doSign(keyPair, SignableData(id, signatureMetadata)) each (Crypto.kt:415-422), byte for
     *  byte what i2p's EdDSAEngine writes. ECDSA_SECP256R1_SHA256 / ECDSA_SECP256K1_SHA256 key pairs go to the
     *  device too (signAllEcdsa: k drawn here from a SecureRandom), and so do RSA_SHA256 key pairs with CRT
     *  parts (signAllRsa: the PSS salt drawn here). A key pair of another scheme, fewer ids than minBatch, a
     *  device fault, or any other non-zero status falls back to Crypto.doSign on the JVM for those ids,
     *  which also raises the reference's own exceptions. */
    fun signAll(keyPair: KeyPair, txIds: List<SecureHash>, signatureMetadata: SignatureMetadata,
                random: SecureRandom = ecNonceRandom): List<TransactionSignature> {
        fun onJvm(id: SecureHash) = Crypto.doSign(keyPair, SignableData(id, signatureMetadata))
        if (txIds.isEmpty()) return emptyList()
        if (txIds.size >= config.minBatch && ecdsaSchemeId(keyPair) != 0)
            return signAllEcdsa(keyPair, txIds, signatureMetadata, random)
        if (txIds.size >= config.minBatch && isRsaCrt(keyPair))
            return signAllRsa(keyPair, txIds, signatureMetadata, random)
        if (!isEd25519(keyPair) || txIds.size < config.minBatch) return txIds.map(::onJvm)
        requireAligned(keyPair)
        val (pre, suf) = signableTemplate(signatureMetadata)
        val arena = direct(pre.size + suf.size + 16)
        val tmpls = direct(24)
        arena.align4(); val po = arena.position().toLong(); arena.put(pre)
        arena.align4(); val so = arena.position().toLong(); arena.put(suf)
        tmpls.putLong(po).putLong(so).putInt(pre.size).putInt(suf.size)
        val n = txIds.size
        val ids = direct(32 * n)
        txIds.forEach { ids.put(it.bytes) }
        val reqs = direct(8 * n)
        val sigs = direct(64 * n)
        val status = direct(n)
        val rc = withHandles { c, p ->
            signerLock.withLock {
                var signer = signerKeys.indexOfFirst { it.public == keyPair.public && it.private == keyPair.private }
                if (signer < 0 && signerKeys.size < CG_SIGNERS_MAX) {   // a key not announced with loadSigners joins the set
                    signerKeys = signerKeys + keyPair
                    signerHandle = 0
                    signer = signerKeys.size - 1
                }
                if (signer < 0 || !ensureSigners(c, p)) CG_ERR_DEVICE
                else {
                    for (j in 0 until n) reqs.putInt(8 * j, j).putShort(8 * j + 4, signer.toShort()).putShort(8 * j + 6, 0)
                    nativeSignTxIds(c, p, ids, n.toLong(), reqs, n.toLong(), tmpls, 1, arena, arena.position().toLong(),
                                    sigs, status)
                }
            }
        }
        return txIds.mapIndexed { j, id ->
            if (rc == CG_OK && status.get(j).toInt() == 0)
                TransactionSignature(ByteArray(64).also { sigs.position(64 * j); sigs.get(it) }, keyPair.public, signatureMetadata)
            else onJvm(id)
        }
    }

    private fun wipe(b: ByteBuffer) { for (i in 0 until b.capacity()) b.put(i, 0) }

    // ---- ECDSA signing (include/cordagpu.h, "ECDSA signing"). A signer set of its own, in the open context
    // (every device of the pool), beside the Ed25519 one and under the same lock.
    private const val CG_NONCE_REJECTED = 9
    private const val CG_EC_SIG_MAX = 72
    private val ecNonceRandom = SecureRandom()
    private var ecSignerKeys: List<KeyPair> = emptyList()
    private var ecSignerHandle = 0L

    /** The scheme id (2 / 3) when both halves are keys of the same ECDSA scheme, else 0. */
    private fun ecdsaSchemeId(k: KeyPair): Int {
        val s = Crypto.findSignatureScheme(k.private)
        if (s != Crypto.findSignatureScheme(k.public)) return 0
        return if (s == Crypto.ECDSA_SECP256R1_SHA256 || s == Crypto.ECDSA_SECP256K1_SHA256) s.schemeNumberID else 0
    }

    /** 32 big-endian bytes of a value below 2^256. */
    private fun be32(v: BigInteger): ByteArray {
        val b = v.toByteArray()
        val out = ByteArray(32)
        val n = minOf(b.size, 32)
        System.arraycopy(b, b.size - n, out, 32 - n, n)
        return out
    }

    /** With signerLock held, inside withHandles: the ECDSA set is in the open context. The device returns each
     *  key's Q = d G, and a pair whose public half is another key's is refused here, as
     *  Crypto.doSign(keyPair, signableData) refuses a misaligned pair (Crypto.kt:416-419). The buffer that
     *  held d is zeroed before it is released. */
    private fun ensureEcSigners(c: Long, p: Long): Boolean {
        val h = if (c != 0L) c else p
        if (ecSignerHandle == h) return true
        val n = ecSignerKeys.size
        val schemes = direct(n)
        val secrets = direct(32 * n)
        val pubs = direct(64 * n)
        val st = direct(n)
        val rc = try {
            ecSignerKeys.forEach {
                schemes.put(ecdsaSchemeId(it).toByte())
                val d = be32((it.private as BCECPrivateKey).d)
                secrets.put(d)
                d.fill(0)
            }
            nativeLoadEcSigners(c, p, schemes, secrets, n, pubs, st)
        } finally {
            wipe(secrets)
        }
        if (rc != CG_OK) return false
        val bad = ecSignerKeys.indices.filter { i ->
            val q = (ecSignerKeys[i].public as BCECPublicKey).q.normalize()
            val want = be32(q.affineXCoord.toBigInteger()) + be32(q.affineYCoord.toBigInteger())
            val got = ByteArray(64).also { pubs.position(64 * i); pubs.get(it) }
            st.get(i).toInt() != 0 || !got.contentEquals(want)
        }
        if (bad.isNotEmpty()) {   // as ensureSigners: the offending pairs leave the set, the next call loads the rest
            ecSignerKeys = ecSignerKeys.filterIndexed { i, _ -> i !in bad }
            ecSignerHandle = 0
            throw IllegalArgumentException("ECDSA signer ${bad.first()}: the public key is not the private key's")
        }
        ecSignerHandle = h
        return true
    }

    /** signAll for an ECDSA key pair: BC 1.57's ECDSASigner.generateSignature with the k candidates drawn here,
     *  32 bytes per attempt as RandomDSAKCalculator.nextK's BigInteger(256, random) does. The device applies
     *  BC's refusals; an id that comes back CG_NONCE_REJECTED is redrawn and resubmitted, the others keep
     *  their signatures. A device fault or any other status falls back to Crypto.doSign on the JVM for that
     *  id. The nonce buffer is zeroed after every call. */
    private fun signAllEcdsa(keyPair: KeyPair, txIds: List<SecureHash>, signatureMetadata: SignatureMetadata,
                             random: SecureRandom): List<TransactionSignature> {
        fun onJvm(id: SecureHash) = Crypto.doSign(keyPair, SignableData(id, signatureMetadata))
        val (pre, suf) = signableTemplate(signatureMetadata)
        val arena = direct(pre.size + suf.size + 16)
        val tmpls = direct(24)
        arena.align4(); val po = arena.position().toLong(); arena.put(pre)
        arena.align4(); val so = arena.position().toLong(); arena.put(suf)
        tmpls.putLong(po).putLong(so).putInt(pre.size).putInt(suf.size)
        val out = arrayOfNulls<TransactionSignature>(txIds.size)
        var pending = txIds.indices.toList()
        val draw = ByteArray(32)
        while (pending.isNotEmpty()) {
            val n = pending.size
            val ids = direct(32 * n)
            pending.forEach { ids.put(txIds[it].bytes) }
            val reqs = direct(8 * n)
            val nonces = direct(32 * n)
            val sigs = direct(CG_EC_SIG_MAX * n)
            val lens = direct(n)
            val status = direct(n)
            val rc = try {
                for (j in 0 until n) { random.nextBytes(draw); nonces.put(draw) }
                withHandles { c, p ->
                    signerLock.withLock {
                        var signer = ecSignerKeys.indexOfFirst { it.public == keyPair.public && it.private == keyPair.private }
                        if (signer < 0 && ecSignerKeys.size < CG_SIGNERS_MAX) {
                            ecSignerKeys = ecSignerKeys + keyPair
                            ecSignerHandle = 0
                            signer = ecSignerKeys.size - 1
                        }
                        if (signer < 0 || !ensureEcSigners(c, p)) CG_ERR_DEVICE
                        else {
                            for (j in 0 until n) reqs.putInt(8 * j, j).putShort(8 * j + 4, signer.toShort()).putShort(8 * j + 6, 0)
                            nativeEcSignTxIds(c, p, ids, n.toLong(), reqs, n.toLong(), tmpls, 1, arena, arena.position().toLong(),
                                              nonces, sigs, lens, status)
                        }
                    }
                }
            } finally {
                wipe(nonces)
                draw.fill(0)
            }
            val again = ArrayList<Int>()
            pending.forEachIndexed { j, i ->
                val st = if (rc == CG_OK) status.get(j).toInt() and 0xFF else -1
                when (st) {
                    0 -> out[i] = TransactionSignature(ByteArray(lens.get(j).toInt() and 0xFF).also { sigs.position(CG_EC_SIG_MAX * j); sigs.get(it) },
                                                       keyPair.public, signatureMetadata)
                    CG_NONCE_REJECTED -> again.add(i)
                    else -> out[i] = onJvm(txIds[i])
                }
            }
            pending = again
        }
        return out.map { it!! }
    }

    // ---- RSA-PSS signing (include/cordagpu.h, "RSA-PSS signing"). The third signer set, under the same lock.
    private const val CG_RSA_SIG_MAX = 512
    private var rsaSignerKeys: List<KeyPair> = emptyList()
    private var rsaSignerHandle = 0L

    /** Both halves RSA_SHA256 keys, the private one with CRT parts and a public exponent that fits the C ABI's
     *  32-bit e. */
    private fun isRsaCrt(k: KeyPair): Boolean {
        if (Crypto.findSignatureScheme(k.private) != Crypto.RSA_SHA256 || Crypto.findSignatureScheme(k.public) != Crypto.RSA_SHA256) return false
        val priv = k.private as? RSAPrivateCrtKey ?: return false
        return priv.publicExponent.signum() > 0 && priv.publicExponent.bitLength() <= 32
    }

    /** The magnitude bytes of a non-negative value, big-endian, without BigInteger's sign byte. */
    private fun magnitude(v: BigInteger): ByteArray {
        val b = v.toByteArray()
        return if (b.size > 1 && b[0] == 0.toByte()) b.copyOfRange(1, b.size).also { b.fill(0) } else b
    }

    /** With signerLock held, inside withHandles: the RSA set is in the open context. A pair whose public half is
     *  not (n, e) of the private key is refused here, as Crypto.doSign(keyPair, signableData) refuses a
     *  misaligned pair (Crypto.kt:416-419); a key the device refuses (its load self-test) leaves the set. The
     *  buffer that held the CRT parts is zeroed before it is released. */
    private fun ensureRsaSigners(c: Long, p: Long): Boolean {
        val h = if (c != 0L) c else p
        if (rsaSignerHandle == h) return true
        val n = rsaSignerKeys.size
        val table = direct(52 * n)
        val secrets = direct(n * (513 + 5 * 257))
        val st = direct(n)
        val rc = try {
            rsaSignerKeys.forEach {
                val k = it.private as RSAPrivateCrtKey
                for (v in listOf(k.modulus, k.primeP, k.primeQ, k.primeExponentP, k.primeExponentQ, k.crtCoefficient)) {
                    val m = magnitude(v)
                    table.putInt(secrets.position()).putInt(m.size)
                    secrets.put(m)
                    m.fill(0)
                }
                table.putInt(k.publicExponent.toInt())
            }
            nativeLoadRsaSigners(c, p, table, n, secrets, secrets.position().toLong(), st)
        } finally {
            wipe(secrets)
        }
        if (rc != CG_OK) return false
        val bad = rsaSignerKeys.indices.filter { i ->
            val pub = rsaSignerKeys[i].public as RSAPublicKey
            val priv = rsaSignerKeys[i].private as RSAPrivateCrtKey
            st.get(i).toInt() != 0 || pub.modulus != priv.modulus || pub.publicExponent != priv.publicExponent
        }
        if (bad.isNotEmpty()) {   // as ensureSigners: the offending pairs leave the set, the next call loads the rest
            rsaSignerKeys = rsaSignerKeys.filterIndexed { i, _ -> i !in bad }
            rsaSignerHandle = 0
            throw IllegalArgumentException("RSA signer ${bad.first()}: the public key is not the private key's, or the device refused the key")
        }
        rsaSignerHandle = h
        return true
    }

    /** signAll for an RSA key pair: BC 1.57's PSSSigner.generateSignature with the salts drawn here, 32 bytes per
     *  signature as its random.nextBytes(salt) does, exactly once: BC never refuses a salt. A device fault or
     *  any non-zero status (CG_SIGN_CHECK_FAILED among them) falls back to Crypto.doSign on the JVM for that id.
     *  The salt buffer is zeroed after the call. */
    private fun signAllRsa(keyPair: KeyPair, txIds: List<SecureHash>, signatureMetadata: SignatureMetadata,
                           random: SecureRandom): List<TransactionSignature> {
        fun onJvm(id: SecureHash) = Crypto.doSign(keyPair, SignableData(id, signatureMetadata))
        val (pre, suf) = signableTemplate(signatureMetadata)
        val arena = direct(pre.size + suf.size + 16)
        val tmpls = direct(24)
        arena.align4(); val po = arena.position().toLong(); arena.put(pre)
        arena.align4(); val so = arena.position().toLong(); arena.put(suf)
        tmpls.putLong(po).putLong(so).putInt(pre.size).putInt(suf.size)
        val n = txIds.size
        val ids = direct(32 * n)
        txIds.forEach { ids.put(it.bytes) }
        val reqs = direct(8 * n)
        val salts = direct(32 * n)
        val sigs = direct(CG_RSA_SIG_MAX * n)
        val lens = direct(2 * n)
        val status = direct(n)
        val draw = ByteArray(32)
        val rc = try {
            for (j in 0 until n) { random.nextBytes(draw); salts.put(draw) }
            withHandles { c, p ->
                signerLock.withLock {
                    var signer = rsaSignerKeys.indexOfFirst { it.public == keyPair.public && it.private == keyPair.private }
                    if (signer < 0 && rsaSignerKeys.size < CG_SIGNERS_MAX) {
                        rsaSignerKeys = rsaSignerKeys + keyPair
                        rsaSignerHandle = 0
                        signer = rsaSignerKeys.size - 1
                    }
                    if (signer < 0 || !ensureRsaSigners(c, p)) CG_ERR_DEVICE
                    else {
                        for (j in 0 until n) reqs.putInt(8 * j, j).putShort(8 * j + 4, signer.toShort()).putShort(8 * j + 6, 0)
                        nativeRsaSignTxIds(c, p, ids, n.toLong(), reqs, n.toLong(), tmpls, 1, arena, arena.position().toLong(),
                                           salts, sigs, lens, status)
                    }
                }
            }
        } finally {
            wipe(salts)
            draw.fill(0)
        }
        return txIds.mapIndexed { j, id ->
            if (rc == CG_OK && status.get(j).toInt() == 0)
                TransactionSignature(ByteArray(lens.getShort(2 * j).toInt() and 0xFFFF).also { sigs.position(CG_RSA_SIG_MAX * j); sigs.get(it) },
                                     keyPair.public, signatureMetadata)
            else onJvm(id)
        }
    }

    /** deriveHMAC's keyData (Crypto.kt:759-771) and the scheme id of a private key the device derives
     *  from, or null: d.toByteArray() of a BC EC key on secp256r1 / secp256k1, geta() of an EdDSA key. */
    private fun deriveKeyData(privateKey: PrivateKey): Pair<Int, ByteArray>? = when (Crypto.findSignatureScheme(privateKey)) {
        Crypto.EDDSA_ED25519_SHA512 -> Crypto.EDDSA_ED25519_SHA512.schemeNumberID to (privateKey as EdDSAPrivateKey).geta()
        Crypto.ECDSA_SECP256R1_SHA256 -> Crypto.ECDSA_SECP256R1_SHA256.schemeNumberID to (privateKey as BCECPrivateKey).d.toByteArray()
        Crypto.ECDSA_SECP256K1_SHA256 -> Crypto.ECDSA_SECP256K1_SHA256.schemeNumberID to (privateKey as BCECPrivateKey).d.toByteArray()
        else -> null
    }

    /** The key pair of the child bytes the device wrote: EdDSAPrivateKeySpec(seed) with the device's Abyte,
     *  or ECPrivateKeySpec(d) with the device's Q = (X, Y), as deriveKeyPairEdDSA / deriveKeyPairECDSA
     *  build them (Crypto.kt:713-737, 676-711). */
    private fun childKeyPair(parent: PrivateKey, schemeId: Int, secret: ByteArray, pub: ByteArray): KeyPair {
        if (schemeId == Crypto.EDDSA_ED25519_SHA512.schemeNumberID) {
            val params = Crypto.EDDSA_ED25519_SHA512.algSpec as EdDSANamedCurveSpec
            val priv = EdDSAPrivateKeySpec(secret, params)
            val abyte = pub.copyOf(32)
            check(abyte.contentEquals(priv.a.toByteArray())) { "the device's Abyte is not the child seed's" }
            return KeyPair(EdDSAPublicKey(EdDSAPublicKeySpec(abyte, params)), EdDSAPrivateKey(priv))
        }
        val scheme = if (schemeId == Crypto.ECDSA_SECP256R1_SHA256.schemeNumberID) Crypto.ECDSA_SECP256R1_SHA256
                     else Crypto.ECDSA_SECP256K1_SHA256
        val spec = scheme.algSpec as ECParameterSpec
        val q = spec.curve.createPoint(BigInteger(1, pub.copyOfRange(0, 32)), BigInteger(1, pub.copyOfRange(32, 64)))
        return KeyPair(BCECPublicKey(parent.algorithm, ECPublicKeySpec(q, spec), BouncyCastleProvider.CONFIGURATION),
                       BCECPrivateKey(parent.algorithm, ECPrivateKeySpec(BigInteger(1, secret), spec), BouncyCastleProvider.CONFIGURATION))
    }

    /** Crypto.deriveKeyPair(privateKey, seed) (Crypto.kt:646-771) for many seeds in one call: a key pair
     *  per transaction and party (Crypto.kt:631-637), byte for byte what the JVM derives. A scheme the
     *  device does not derive for (RSA, SPHINCS: the reference throws), fewer seeds than minBatch, a
     *  device fault or any non-zero status (CG_DERIVE_HOST: more than four rehashes) falls back to
     *  Crypto.deriveKeyPair on the JVM for those seeds, which also raises the reference's own exceptions.
     *  The direct buffers that held key bytes (the arena with keyData, the child secrets) are zeroed
     *  before they are released, and so is the keyData array. */
    fun deriveAll(privateKey: PrivateKey, seeds: List<ByteArray>): List<KeyPair> {
        fun onJvm(seed: ByteArray) = Crypto.deriveKeyPair(privateKey, seed)
        if (seeds.isEmpty()) return emptyList()
        val kd = if (seeds.size < config.minBatch) null else deriveKeyData(privateKey)
        if (kd == null || kd.second.isEmpty() || kd.second.size > 128) return seeds.map(::onJvm)
        val (schemeId, keyData) = kd
        val n = seeds.size
        val arena = direct(keyData.size + seeds.sumOf { it.size } + 16)
        val parents = direct(16)
        val reqs = direct(16 * n)
        val secrets = direct(32 * n)
        val pubs = direct(64 * n)
        val status = direct(n)
        val retries = direct(n)
        try {
            parents.putLong(0L).putShort(keyData.size.toShort()).put(schemeId.toByte())
            arena.put(keyData)
            seeds.forEach { reqs.putLong(arena.position().toLong()).putInt(it.size).putInt(0); arena.put(it) }
            val rc = withHandles { c, p ->
                nativeDeriveKeys(c, p, parents, 1, reqs, n.toLong(), arena, arena.position().toLong(), secrets, pubs, status, retries)
            }
            return seeds.mapIndexed { j, seed ->
                if (rc == CG_OK && status.get(j).toInt() == 0)
                    childKeyPair(privateKey, schemeId, ByteArray(32).also { secrets.position(32 * j); secrets.get(it) },
                                 ByteArray(64).also { pubs.position(64 * j); pubs.get(it) })
                else onJvm(seed)
            }
        } finally {
            wipe(arena); wipe(secrets); keyData.fill(0)
        }
    }

    /** The public halves of 32-byte private keys of one scheme (cg_public_keys): Abyte for Ed25519 seeds
     *  (deriveKeyPairFromEntropy, generateKeyPair with bytes the caller drew from SecureRandom), X || Y for
     *  ECDSA candidates d, whose status is CG_KEY_REJECTED when BC's accept rule refuses them (the caller
     *  redraws). Returns (public keys 64 bytes each, status bytes); null on a device fault. The secrets
     *  buffer is zeroed before it is released. */
    fun publicKeys(schemeId: Int, privateKeys: List<ByteArray>): Pair<ByteArray, ByteArray>? {
        require(privateKeys.all { it.size == 32 }) { "a private key is 32 bytes" }
        val n = privateKeys.size
        if (n == 0) return ByteArray(0) to ByteArray(0)
        val secrets = direct(32 * n)
        val pubs = direct(64 * n)
        val status = direct(n)
        try {
            privateKeys.forEach { secrets.put(it) }
            val rc = withHandles { c, p -> nativePublicKeys(c, p, schemeId, secrets, n.toLong(), pubs, status) }
            if (rc != CG_OK) return null
            return ByteArray(64 * n).also { pubs.position(0); pubs.get(it) } to ByteArray(n).also { status.position(0); status.get(it) }
        } finally {
            wipe(secrets)
        }
    }

    /** cg_verify_batch over tables already in the C ABI's layout (the out-of-process verifier's batch
     *  request body, VerifierBatchApi.kt): no re-encoding. One status byte per item; one device or a
     *  pool. On a device fault the NOT_RUN items' records are re-queued once as a table of their own
     *  (same keys and arena); any still NOT_RUN go back to the node as NOT_RUN. */
    fun verifyPacked(keys: ByteBuffer, nKeys: Int, items: ByteBuffer, nItems: Int, arena: ByteBuffer, arenaLen: Long,
                     mode: Int = MODE_DOVERIFY): ByteArray = timed(nItems) {
        require(nKeys >= 0 && nItems >= 0 && arenaLen >= 0) { "negative table size" }
        require(keys.capacity().toLong() >= 16L * nKeys && items.capacity().toLong() >= 32L * nItems &&
                arena.capacity().toLong() >= arenaLen) { "a table is shorter than its count" }
        verifyPackedItems(keys, nKeys, items, nItems, arena, arenaLen, mode, requeue = true)
    }

    private fun verifyPackedItems(keys: ByteBuffer, nKeys: Int, items: ByteBuffer, nItems: Int, arena: ByteBuffer,
                                  arenaLen: Long, mode: Int, requeue: Boolean): ByteArray {
        val status = direct(nItems)
        val stats = direct(STATS_BYTES)
        val rc = withHandles { c, p -> nativeVerify(c, p, keys, nKeys, items, nItems.toLong(), arena, arenaLen, mode, status, stats) }
        val st = ByteArray(nItems).also { status.get(it) }
        requeueNotRun(rc, "cg_verify_batch", st, if (!requeue) null else { todo ->
            val sub = direct(32 * todo.size)
            val rec = ByteArray(32)
            for (i in todo) { items.duplicate().apply { position(32 * i) }.get(rec); sub.put(rec) }
            verifyPackedItems(keys, nKeys, sub, todo.size, arena, arenaLen, mode, requeue = false)
        })
        record(stats, st)
        return st
    }

    /** WireTransaction ids + every signature in one call (cg_verify_transactions, include/cordagpu.h):
     *  the tables are the C ABI's own (cg_tx / cg_component / cg_txsig / cg_signable_tmpl, built by the
     *  out-of-process verifier from the request body it already holds). Fills the 32-byte ids, one
     *  status per transaction (Merkle) and one per signature. With a pool the call runs whole on one
     *  healthy device and fails over to the next (cg_pool_verify_transactions: a signature may reference
     *  any transaction's id, so it is not sharded). When no device could run it the signatures stay
     *  NOT_RUN and the ids are not computed: IllegalStateException, the request is redelivered whole. */
    fun verifyTransactionsPacked(txs: ByteBuffer, nTx: Long, comps: ByteBuffer, nComps: Long, keys: ByteBuffer,
                                 nKeys: Int, sigs: ByteBuffer, nSigs: Long, tmpls: ByteBuffer, nTmpls: Int,
                                 arena: ByteBuffer, arenaLen: Long, idsOut: ByteBuffer, txStatusOut: ByteBuffer,
                                 sigStatusOut: ByteBuffer, mode: Int = MODE_DOVERIFY) {
        val rc = withHandles { c, p ->
            nativeVerifyTransactions(c, p, txs, nTx, comps, nComps, keys, nKeys, sigs, nSigs, tmpls, nTmpls, arena,
                                     arenaLen, mode, idsOut, txStatusOut, sigStatusOut)
        }
        check(rc == CG_OK) { "cg_verify_transactions failed: $rc (no device could run it: redeliver the request)" }
    }

    /** Pins a direct buffer the caller keeps across calls (cg_host_register); unregister before freeing it. */
    fun registerHostBuffer(buf: ByteBuffer) {
        require(buf.isDirect) { "only a direct buffer can be registered" }
        check(nativeHostRegister(buf, buf.capacity().toLong()) == 0) { "cg_host_register failed" }
    }
    fun unregisterHostBuffer(buf: ByteBuffer) { check(nativeHostUnregister(buf) == 0) { "cg_host_unregister failed" } }

    /** Re-raise what the serial Crypto.doVerify would have done for an item. Fails closed: every
     *  status but CG_VALID ends in a throw, or in the JVM's own doVerify (which throws or returns as the
     *  serial call does) for a scheme the GPU does not run. Mapping (INTEGRATION.md §2):
     *    1 INVALID       SignatureException("Signature Verification failed!")      Crypto.kt:478-483
     *    2 SIG_MALFORMED SignatureException (the engine's decode message)
     *    3 KEY_INVALID   the JVM decoder's own exception, else InvalidKeyException
     *    4 UNSUPPORTED   Crypto.doVerify on the host (RSA / SPHINCS / COMPOSITE)
     *    5 EMPTY         IllegalArgumentException (Crypto.kt:476-477)
     *  255 NOT_RUN       no device ran it (after the re-queue): Crypto.doVerify on the host, as UNSUPPORTED
     *    other           IllegalStateException (not a status the engine writes) */
    fun raiseForStatus(status: Byte, item: BatchItem) {
        val scheme = Crypto.findSignatureScheme(item.publicKey)
        when (status.toInt() and 0xff) {
            CG_VALID -> return
            CG_INVALID -> throw SignatureException("Signature Verification failed!")
            CG_SIG_MALFORMED -> throw SignatureException(if (scheme == Crypto.EDDSA_ED25519_SHA512) "signature length is wrong"
                                                         else "error decoding signature bytes.")
            CG_KEY_INVALID -> {
                Crypto.decodePublicKey(scheme, item.publicKey.encoded)   // throws the JVM's own key exception
                throw InvalidKeyException("public key rejected by the batch engine: ${scheme.schemeCodeName}")
            }
            CG_UNSUPPORTED -> { Crypto.doVerify(item.publicKey, item.signatureData, item.clearData); return }
            CG_NOT_RUN -> { Crypto.doVerify(item.publicKey, item.signatureData, item.clearData); return }
            CG_EMPTY -> throw IllegalArgumentException(if (item.signatureData.isEmpty()) "Signature data is empty!"
                                                      else "Clear data is empty, nothing to verify!")
            else -> throw IllegalStateException("unknown engine status $status")
        }
    }

    /** TransactionWithSignatures.checkSignaturesAreValid (TransactionWithSignatures.kt:58-61) for many
     *  transactions in one call; the first failure in list order throws what the serial loop threw.
     *  Below gpuVerifier.minBatch signatures the reference's serial loop runs unchanged. */
    fun checkSignaturesAreValidBatch(stxs: List<SignedTransaction>) {
        if (stxs.sumOf { it.sigs.size } < config.minBatch) {
            for (stx in stxs) for (sig in stx.sigs) sig.verify(stx.id)
            return
        }
        val st = verifyTxSignatures(stxs.map { it.id to it.sigs })
        var k = 0
        for (stx in stxs) for (sig in stx.sigs) {
            val s = st[k++]
            if (s.toInt() != CG_VALID) raiseForStatus(s, BatchItem(sig.by, sig.bytes,
                                                      SignableData(stx.id, sig.signatureMetadata).serialize().bytes))
        }
    }

    /** The cg_req_node table of a batch: the required keys' roots first, then every distinct CompositeKey's
     *  children as one block, higher trees first, so that a child's index is always greater than its
     *  parent's (the device walk refuses anything else). Equal CompositeKeys share a block, equal
     *  required keys a root. Mirrors corda_amd/batch.py RequirementBuilder. */
    private class Requirements(val classOf: (PublicKey) -> Int) {
        val roots = LinkedHashMap<PublicKey, Int>()
        val reqs = ArrayList<Int>()
        fun add(keys: Collection<PublicKey>): Pair<Int, Int> {
            val first = reqs.size
            for (k in keys) reqs.add(roots.getOrPut(k) { roots.size })
            return first to keys.size
        }
        fun nodes(): ByteBuffer {
            val height = LinkedHashMap<CompositeKey, Int>()
            fun visit(k: CompositeKey): Int = height[k] ?: (1 + (k.children.map { it.node }.filterIsInstance<CompositeKey>()
                                                                  .map { visit(it) }.max() ?: 0)).also { height[k] = it }
            roots.keys.filterIsInstance<CompositeKey>().forEach { visit(it) }
            val block = LinkedHashMap<CompositeKey, Int>()
            var at = roots.size
            for (k in height.keys.sortedByDescending { height[it]!! }) { block[k] = at; at += k.children.size }
            val out = ByteBuffer.allocateDirect(REQ_NODE_BYTES * maxOf(at, 1)).order(ByteOrder.LITTLE_ENDIAN)
            fun fill(i: Int, k: PublicKey, weight: Int) {
                out.position(REQ_NODE_BYTES * i)
                if (k is CompositeKey) out.putInt(block[k]!!).putInt(k.children.size).putInt(weight).putInt(k.threshold)
                else out.putInt(classOf(k)).putInt(0).putInt(weight).putInt(0)
            }
            roots.keys.forEachIndexed { i, k -> fill(i, k, 0) }
            for ((k, first) in block) k.children.forEachIndexed { j, c -> fill(first + j, c.node, c.weight) }
            out.position(REQ_NODE_BYTES * at)
            return out
        }
    }

    /** SignedTransaction.verifyRequiredSignatures / verifySignaturesExcept(allowedToBeMissing)
     *  (TransactionWithSignatures.kt:41-47) for many transactions in one call: the signatures are verified and
     *  reduced per transaction on the device (cg_verify_required_signatures_packed: the first failing
     *  signature, then the required keys the signers do not fulfil, composite-aware). The first transaction
     *  in list order that fails throws what its serial call throws. Key classes come from
     *  PublicKey.equals / hashCode (a HashMap); CompositeKeys are validated here (checkValidity throws on the
     *  host) and flattened. A transaction the device hands back -- CG_TXV_SPAN_BAD, CG_TXV_REQ_HOST without a
     *  failing signature before it, or a first failing status of CG_UNSUPPORTED / CG_NOT_RUN (a scheme the
     *  GPU does not run, a device fault) -- runs the reference's own verifySignaturesExcept.
     *  Below gpuVerifier.minBatch signatures the serial calls run unchanged. */
    fun verifyRequiredSignaturesAll(stxs: List<SignedTransaction>, allowedToBeMissing: Set<PublicKey> = emptySet()) {
        val allowed = allowedToBeMissing.toTypedArray()
        if (stxs.sumOf { it.sigs.size } < config.minBatch) {
            for (stx in stxs) stx.verifySignaturesExcept(*allowed)
            return
        }
        val all = stxs.flatMap { it.sigs }
        val metas = LinkedHashMap<SignatureMetadata, Int>()
        all.forEach { metas.getOrPut(it.signatureMetadata) { metas.size } }
        val split = metas.keys.map { signableTemplate(it) }
        val arena = direct(split.sumOf { it.first.size + it.second.size + 8 } +
                           all.map { it.by }.distinct().sumOf { it.encoded.size + 4 } + 16)
        val keys = Keys(all.map { it.by }, arena)
        val tmpls = direct(24 * split.size)
        for ((pre, suf) in split) {
            arena.align4(); val p = arena.position().toLong(); arena.put(pre)
            arena.align4(); val s = arena.position().toLong(); arena.put(suf)
            tmpls.putLong(p).putLong(s).putInt(pre.size).putInt(suf.size)
        }
        // classes from PublicKey.equals: the key table's entries first (entry k has class k: Keys already merges
        // equal keys), then every required leaf that never signed
        val classes = HashMap<PublicKey, Int>()
        keys.index.forEach { (k, i) -> classes[k] = i }
        val keyClass = direct(4 * keys.index.size)
        for (i in 0 until keys.index.size) keyClass.putInt(i)
        val req = Requirements { k -> classes.getOrPut(k) { classes.size } }
        val ids = direct(32 * stxs.size)
        val sigs = direct(12 * all.size)
        val stream = direct(all.sumOf { minOf(it.bytes.size, SIG_LEN_MAX) + 4 })
        val checks = direct(TX_CHECK_BYTES * stxs.size)
        val needed = ArrayList<List<PublicKey>>()
        var pos = 0L
        stxs.forEachIndexed { t, stx ->
            ids.put(stx.id.bytes)
            for (sig in stx.sigs) {
                val k = keys.index[sig.by]!!
                val bytes = sigField(keys.schemes[k], sig.bytes)
                stream.put(bytes).align4()
                sigs.putInt(t).putInt(k).putShort(bytes.size.toShort()).putShort(metas[sig.signatureMetadata]!!.toShort())
            }
            val want = stx.requiredSigningKeys.filter { it !in allowedToBeMissing }
            want.filterIsInstance<CompositeKey>().forEach { it.checkValidity() }   // throws as isFulfilledBy would
            val (first, n) = req.add(want)
            needed.add(want)
            checks.putLong(pos).putInt(stx.sigs.size).putInt(first).putInt(n).putInt(0)
            pos += stx.sigs.size
        }
        val nodes = req.nodes()
        val reqs = direct(4 * req.reqs.size)
        req.reqs.forEach { reqs.putInt(it) }
        val verdicts = direct(TX_VERDICT_BYTES * stxs.size)
        val reqStatus = direct(req.reqs.size)
        val rc = timed(all.size) {
            withHandles { c, p ->
                nativeVerifyRequiredPacked(c, p, keys.table, keys.index.size, ids, stxs.size.toLong(), sigs,
                                           all.size.toLong(), stream, stream.position().toLong(), tmpls, split.size,
                                           arena, arena.position().toLong(), MODE_DOVERIFY, keyClass, checks,
                                           stxs.size.toLong(), reqs, req.reqs.size, nodes,
                                           nodes.position() / REQ_NODE_BYTES, null, verdicts, reqStatus)
            }
        }
        // a device fault leaves NOT_RUN verdicts (handled per transaction below); anything else is a bug
        check(rc == CG_OK || rc == CG_ERR_DEVICE) { "cg_verify_required_signatures_packed failed ($rc)" }
        stxs.forEachIndexed { t, stx ->
            val firstBad = verdicts.getInt(TX_VERDICT_BYTES * t)
            val status = verdicts.get(TX_VERDICT_BYTES * t + 4).toInt() and 0xff
            val flags = verdicts.get(TX_VERDICT_BYTES * t + 5).toInt() and 0xff
            val nMissing = verdicts.getShort(TX_VERDICT_BYTES * t + 6).toInt() and 0xffff
            val hasBad = firstBad != NO_BAD
            if ((flags and CG_TXV_SPAN_BAD) != 0 || (hasBad && (status == CG_UNSUPPORTED || status == CG_NOT_RUN)) ||
                (!hasBad && (flags and CG_TXV_REQ_HOST) != 0)) {
                stx.verifySignaturesExcept(*allowed)
            } else if (hasBad) {
                val sig = stx.sigs[firstBad]
                raiseForStatus(status.toByte(), BatchItem(sig.by, sig.bytes,
                                                          SignableData(stx.id, sig.signatureMetadata).serialize().bytes))
            } else if (nMissing != 0) {
                val first = checks.getInt(TX_CHECK_BYTES * t + 12)
                val found = needed[t].filterIndexed { r, _ -> (reqStatus.get(first + r).toInt() and 0xff) == CG_REQ_MISSING }.toSet()
                // built as getMissingSignatures builds it, so the exception lists the keys in its order
                val missing = stx.requiredSigningKeys.filter { it in found }.toSet() - allowedToBeMissing
                throw SignedTransaction.SignaturesMissingException(missing, stx.getKeyDescriptions(missing), stx.id)
            }
        }
    }
}
