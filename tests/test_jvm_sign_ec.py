"""The Kotlin binding's ECDSA sign path (jvm/.../CryptoBatch.kt signAllEcdsa) and its two JNI functions, read
as source (no JVM here; tests/test_jvm_binding.py compiles the shim against the header and checks every
external fun's parameter count): ECDSA key pairs go to the device with nonces from a SecureRandom, only
CG_NONCE_REJECTED items are redrawn, everything else falls back to Crypto.doSign, the nonce buffer is zeroed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT = open(os.path.join(ROOT, "jvm/src/main/kotlin/net/corda/core/crypto/CryptoBatch.kt")).read()
JNI = open(os.path.join(ROOT, "jvm/jni/cordagpu_jni.c")).read()
HDR = open(os.path.join(ROOT, "include/cordagpu.h")).read()


def _body(name):
    at = re.search(rf"fun {name}\(", KT).start()
    nxt = re.search(r"\n    (?:private |internal )?(?:fun|val|var|class|object|/\*\*|@|//)", KT[at + 1:])
    return KT[at:at + 1 + nxt.start()] if nxt else KT[at:]


def test_external_funs_and_jni_exports():
    for ext, calls in (("nativeLoadEcSigners", ("cg_ec_signers_load(", "cg_pool_ec_signers_load(")),
                       ("nativeEcSignTxIds", ("cg_ec_sign_tx_ids(", "cg_pool_ec_sign_tx_ids("))):
        decl = re.search(rf"external fun {ext}\((.*?)\): Int", KT, re.S).group(1)
        assert decl.replace(" ", "").replace("\n", "").startswith("ctx:Long,pool:Long,"), ext
        c = re.search(rf"Java_net_corda_core_crypto_CryptoBatch_{ext}\((.*?)\)\s*{{(.*?)\n}}", JNI, re.S)
        assert c and all(x in c.group(2) for x in calls), ext
        assert len([p for p in decl.split(",") if p.strip()]) + 2 == len(c.group(1).split(",")), ext
    assert "nonces: ByteBuffer, sigsOut: ByteBuffer, sigLenOut: ByteBuffer" in KT.replace("\n", " ").replace("  ", "")\
        or re.search(r"nonces: ByteBuffer,\s*sigsOut: ByteBuffer,\s*sigLenOut: ByteBuffer", KT)


def test_constants_match_the_header():
    assert re.search(r"#define CG_NONCE_REJECTED 9\b", HDR) and "const val CG_NONCE_REJECTED = 9" in KT
    assert re.search(r"#define CG_EC_SIG_MAX 72\b", HDR) and "const val CG_EC_SIG_MAX = 72" in KT


def test_sign_all_routes_ecdsa_pairs_to_the_device_above_min_batch():
    body = _body("signAll")
    assert "random: SecureRandom" in body
    assert re.search(r"txIds\.size >= config\.minBatch && ecdsaSchemeId\(keyPair\) != 0\)\s*return signAllEcdsa\(", body)
    assert "txIds.size < config.minBatch) return txIds.map(::onJvm)" in body  # below minBatch: the JVM, as before
    sid = _body("ecdsaSchemeId")
    assert "ECDSA_SECP256R1_SHA256" in sid and "ECDSA_SECP256K1_SHA256" in sid and "k.public" in sid


def test_redraw_fallback_and_zeroing():
    body = _body("signAllEcdsa")
    assert "random.nextBytes(draw); nonces.put(draw)" in body           # 32 bytes per attempt, drawn on the JVM
    assert "CG_NONCE_REJECTED -> again.add(i)" in body and "pending = again" in body  # only the refused ids
    assert "else -> out[i] = onJvm(txIds[i])" in body                   # a device fault (st = -1) or any other status
    assert "if (rc == CG_OK) status.get(j).toInt() and 0xFF else -1" in body
    assert re.search(r"finally \{\s*wipe\(nonces\)", body)              # zeroed whatever happened
    assert "nativeEcSignTxIds(c, p," in body and "withHandles {" in body and "signerLock.withLock" in body
    ens = _body("ensureEcSigners")
    assert "wipe(secrets)" in ens and "nativeLoadEcSigners(c, p," in ens and "contentEquals(want)" in ens
    assert "st.get(i).toInt() != 0" in ens                              # a key the device refused leaves the set
