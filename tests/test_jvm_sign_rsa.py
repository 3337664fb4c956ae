"""The Kotlin binding's RSA sign path (jvm/.../CryptoBatch.kt signAllRsa) and its two JNI functions, read as
source (no JVM here; tests/test_jvm_binding.py compiles the shim against the header and checks every external
fun's parameter count): RSA CRT key pairs go to the device with salts from a SecureRandom, one draw per
signature and no redraw, every non-zero status falls back to Crypto.doSign, the salt and key buffers are zeroed."""
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
    for ext, calls in (("nativeLoadRsaSigners", ("cg_rsa_signers_load(", "cg_pool_rsa_signers_load(")),
                       ("nativeRsaSignTxIds", ("cg_rsa_sign_tx_ids(", "cg_pool_rsa_sign_tx_ids("))):
        decl = re.search(rf"external fun {ext}\((.*?)\): Int", KT, re.S).group(1)
        assert decl.replace(" ", "").replace("\n", "").startswith("ctx:Long,pool:Long,"), ext
        c = re.search(rf"Java_net_corda_core_crypto_CryptoBatch_{ext}\((.*?)\)\s*{{(.*?)\n}}", JNI, re.S)
        assert c and all(x in c.group(2) for x in calls), ext
        assert len([p for p in decl.split(",") if p.strip()]) + 2 == len(c.group(1).split(",")), ext
    assert "(uint16_t*)ADDR(sig_len_out)" in JNI


def test_constants_match_the_header():
    assert re.search(r"#define CG_RSA_SIG_MAX 512\b", HDR) and "const val CG_RSA_SIG_MAX = 512" in KT
    assert "} cg_rsa_signer;     /* 52 bytes */" in HDR and "direct(52 * n)" in _body("ensureRsaSigners")


def test_sign_all_sends_rsa_crt_pairs_to_the_device():
    body = _body("signAll")
    assert re.search(r"txIds\.size >= config\.minBatch && isRsaCrt\(keyPair\)\)\s*return signAllRsa\(", body)
    crt = _body("isRsaCrt")
    assert "RSAPrivateCrtKey" in crt and "bitLength() <= 32" in crt and "Crypto.RSA_SHA256" in crt


def test_one_salt_per_signature_no_redraw_and_the_fallback():
    body = _body("signAllRsa")
    assert body.count("random.nextBytes(draw); salts.put(draw)") == 1 and "while (" not in body  # drawn once
    assert re.search(r"finally \{\s*wipe\(salts\)", body)  # zeroed whatever happened
    assert "nativeRsaSignTxIds(c, p," in body and "withHandles {" in body and "signerLock.withLock" in body
    assert "if (rc == CG_OK && status.get(j).toInt() == 0)" in body and "else onJvm(id)" in body
    assert "lens.getShort(2 * j).toInt() and 0xFFFF" in body  # the 16-bit length
    ens = _body("ensureRsaSigners")
    assert "wipe(secrets)" in ens and "nativeLoadRsaSigners(c, p," in ens and "st.get(i).toInt() != 0" in ens
    assert "pub.modulus != priv.modulus || pub.publicExponent != priv.publicExponent" in ens  # the key-pair check
    for part in ("modulus", "primeP", "primeQ", "primeExponentP", "primeExponentQ", "crtCoefficient"):
        assert "k." + part in ens, part
