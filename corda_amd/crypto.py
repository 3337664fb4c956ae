"""Host mirror of Corda's ``Crypto`` verification API over the MI355X engine.

Mirrors core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:
  * ``Crypto.do_verify(public_key, signature_data, clear_data)`` -- Crypto.kt:457 -> :474-484:
    unsupported scheme -> IllegalArgumentException; empty signature / clear data ->
    IllegalArgumentException; verification false -> SignatureException("Signature Verification
    failed!"); returns True.
  * ``Crypto.is_valid(...)`` -- Crypto.kt:536 -> :553-559: returns a boolean; engine exceptions
    propagate.
  * ``Crypto.do_verify_tx(tx_id, transaction_signature)`` / ``is_valid_tx`` -- Crypto.kt:499-502,
    :516-519: the clear data is SignableData(txId, metadata) (corda_amd/signable.py).
  * ``Crypto.verify_batch(items, mode)`` -- the batch overload this engine adds: one status byte
    per item (include/cordagpu.h). Ed25519 / ECDSA items run on the GPU. The schemes the GPU
    returns CG_UNSUPPORTED for are NOT errors -- Corda supports them (Crypto.kt:177-184, :891) --
    and are routed to the host, as the Kotlin binding falls back to ``Crypto.isValid``:
      - RSA_SHA256: corda_amd/hostverify.py; when the engine in use was opened with ``rsa=True`` an
        RSA item with an X.509 key joins the GPU batch first and only what comes back UNSUPPORTED
        (a key the device decode declines) goes to the host;
      - COMPOSITE: corda_amd/composite.py -- the threshold walk on the host, every leaf signature
        expanded into the same GPU batch (isValid semantics over SignableData(txId, leaf meta));
      - SPHINCS-256: no host verifier in this mirror -> UnsupportedOperationException.
    Items decided on the host with an exception the C status bytes cannot express get the
    mirror-only status HOST_EXCEPTION and their exception in ``verify_batch_ex``'s error map.
  * ``Crypto.raise_for_status`` maps a status byte back onto the exception the serial JVM call
    would have thrown, so a batch caller reproduces fail-fast semantics
    (TransactionWithSignatures.kt:58-62) exactly.

Key-decode failures (status KEY_INVALID) are the exceptions the JVM raises when it builds the key
object, before any verification [ext, recalled]: a raw Ed25519 key (Kryo.kt:330-339 ->
i2p GroupElement) -> IllegalArgumentException("not a valid point"); an X.509 key through
Crypto.decodePublicKey (Crypto.kt:349-356, the ECDSA Kryo path Kryo.kt:388-398) ->
InvalidKeySpecException("This public key cannot be decoded, ...").

Signing (Crypto.kt:395-402, :415-422) on the GPU: EDDSA_ED25519_SHA512, and with ``random=`` the two ECDSA
schemes (below):
  * ``Crypto.do_sign(private_key, clear_data)`` -- doSign(privateKey, clearData): an unsupported scheme
    -> IllegalArgumentException; empty clear data -> Exception("Signing of an empty array is not
    permitted!"); returns the 64 signature bytes i2p's EdDSAEngine.engineSign writes (RFC 8032).
  * ``Crypto.do_sign_tx(key_pair, signable_data)`` -- doSign(keyPair, signableData): a pair whose halves
    have different schemes -> IllegalArgumentException("Metadata schemeCodeName: ... is not aligned with
    the key type: ..."); returns a TransactionSignature. The mirror also refuses a pair whose public
    key is not the private key's (the Abyte ``Engine.load_signers`` returns).
  * ``Crypto.sign_all(key_pair, tx_ids, metadata)`` -- the batch form: NotaryService.sign(txId)
    (NotaryService.kt:77-80) for many ids in one call.
  A SPHINCS private key raises UnsupportedOperationException, as SPHINCS verification does, and so does an
  ECDSA or RSA key when no ``random=`` is given: the mirror has no host signer (a JVM caller keeps its own
  Crypto.doSign for those).
  * ``do_sign`` / ``do_sign_tx`` / ``sign_all`` with ``random=`` (a callable ``random(nbytes) -> bytes``, e.g.
    ``secrets.token_bytes``) sign with ECDSA_SECP256K1_SHA256 / ECDSA_SECP256R1_SHA256 keys: the host
    draws BC's BigInteger(256, random) candidates for k, the device signs (cg_ec_sign_batch /
    cg_ec_sign_tx_ids) and applies BC's refusals, and only the refused items are redrawn, one draw per
    attempt as in ECDSASigner.generateSignature. Returns BC's DER bytes.
  * With ``random=`` they also sign with RSA_SHA256 keys (``PrivateKey(RSA_SHA256, pkcs8)``, the PKCS#8 DER
    of getEncoded()): the host draws PSSSigner's 32-byte salt, ``random(32)`` exactly once per signature
    and never again (BC never refuses a salt), and the device signs (cg_rsa_sign_batch /
    cg_rsa_sign_tx_ids). Returns the k = ceil(bits(n) / 8) signature bytes. A key without CRT parts, or
    whose public exponent is 2^32 or more (the C ABI's e is 32 bits), raises UnsupportedOperationException.

Key derivation (Crypto.kt:646-771), all three curves, on the GPU:
  * ``Crypto.derive_key_pair(private_key, seed, scheme=None)`` -- deriveKeyPair: a scheme that is not
    supported -> IllegalArgumentException; RSA / SPHINCS -> UnsupportedOperationException; returns the
    KeyPair the JVM returns, byte for byte (ECDSA public keys as raw X || Y).
  * ``Crypto.derive_key_pairs(private_key, seeds)`` -- the batch form: one key pair per seed in one call
    (a confidential identity per transaction). An item the device hands back with DERIVE_HOST (more than
    4 rehashes) is finished by corda_amd/derive.py.
  * ``Crypto.derive_key_pair_from_entropy(entropy)`` -- deriveKeyPairFromEntropy (Ed25519 only).
  * ``Crypto.generate_key_pair(scheme)`` -- generateKeyPair for the three curves: the host draws the
    randomness (``secrets``), the device applies the accept rule and computes the public key; a refused
    ECDSA candidate is redrawn.

Public keys are ``PublicKey(scheme, encoded, fmt)`` (fmt: raw / SPKI / SEC1), the byte forms a JVM
caller hands over JNI; two PublicKeys are equal when their X.509 encodings are (as JVM keys are),
and ``CompositeKey`` (corda_amd/composite.py) is a PublicKey too.
"""
import threading
from dataclasses import dataclass

import numpy as np

from . import batch as B
from . import keys as K
from .engine import Engine
from .hostverify import InvalidKeySpecException, UnsupportedOperationException

RSA_SHA256 = 1
ECDSA_SECP256K1_SHA256 = B.ECDSA_SECP256K1_SHA256
ECDSA_SECP256R1_SHA256 = B.ECDSA_SECP256R1_SHA256
EDDSA_ED25519_SHA512 = B.EDDSA_ED25519_SHA512
_ECDSA_SCHEMES = (ECDSA_SECP256K1_SHA256, ECDSA_SECP256R1_SHA256)
_EC_ORDER = {ECDSA_SECP256K1_SHA256: 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
             ECDSA_SECP256R1_SHA256: 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551}  # group orders n
SPHINCS256_SHA256 = 5
COMPOSITE_KEY = 6

SCHEME_CODE_NAMES = {
    RSA_SHA256: "RSA_SHA256",
    ECDSA_SECP256K1_SHA256: "ECDSA_SECP256K1_SHA256",
    ECDSA_SECP256R1_SHA256: "ECDSA_SECP256R1_SHA256",
    EDDSA_ED25519_SHA512: "EDDSA_ED25519_SHA512",
    SPHINCS256_SHA256: "SPHINCS-256_SHA512",
    COMPOSITE_KEY: "COMPOSITE",
}
GPU_SCHEMES = (ECDSA_SECP256K1_SHA256, ECDSA_SECP256R1_SHA256, EDDSA_ED25519_SHA512)
HOST_EXCEPTION = 240  # mirror-only status: decided on the host with an exception (see verify_batch_ex)

__all__ = ["Crypto", "PublicKey", "PrivateKey", "KeyPair", "SignableData", "BatchItem", "TransactionSignature", "SignatureException", "InvalidKeyException",
           "IllegalArgumentException", "InvalidKeySpecException", "UnsupportedOperationException", "HOST_EXCEPTION"]


class SignatureException(Exception):
    """java.security.SignatureException"""


class InvalidKeyException(Exception):
    """java.security.InvalidKeyException"""


class IllegalArgumentException(ValueError):
    """java.lang.IllegalArgumentException"""


@dataclass(frozen=True, eq=False)
class PublicKey:
    scheme: int
    encoded: bytes
    fmt: int = B.KEY_RAW

    def spki(self):
        return K.canonical_spki(self.scheme, self.fmt, self.encoded)

    def __eq__(self, other):
        return isinstance(other, PublicKey) and self.scheme == other.scheme and self.spki() == other.spki()

    def __hash__(self):
        return hash((self.scheme, self.spki()))

    def __repr__(self):
        return f"PublicKey({SCHEME_CODE_NAMES.get(self.scheme, self.scheme)}, {self.spki().hex()[-16:]})"


@dataclass(frozen=True, eq=False)
class PrivateKey:
    """A private key as the node's key store holds it. EDDSA_ED25519_SHA512: ``encoded`` is the 32-byte
    seed of EdDSAPrivateKeySpec(seed). ECDSA_SECP256R1_SHA256 / ECDSA_SECP256K1_SHA256: ``encoded`` is the
    32-byte big-endian d of the BC EC private key. RSA_SHA256: ``encoded`` is the PKCS#8 DER of
    getEncoded() (a BCRSAPrivateCrtKey)."""
    scheme: int
    encoded: bytes

    def __eq__(self, other):
        return isinstance(other, PrivateKey) and self.scheme == other.scheme and self.encoded == other.encoded

    def __hash__(self):
        return hash((self.scheme, self.encoded))

    def __repr__(self):  # never the key bytes
        return f"PrivateKey({SCHEME_CODE_NAMES.get(self.scheme, self.scheme)})"


@dataclass(frozen=True)
class KeyPair:
    """java.security.KeyPair"""
    public: PublicKey
    private: PrivateKey


@dataclass(frozen=True)
class SignableData:
    """SignableData(txId, SignatureMetadata(platformVersion, schemeNumberID)) (SignableData.kt:13)."""
    tx_id: bytes
    platform_version: int = 1
    scheme_number_id: int = 4


@dataclass(frozen=True)
class TransactionSignature:
    """TransactionSignature(bytes, by, SignatureMetadata(platformVersion, schemeNumberID))
    (TransactionSignature.kt:14, SignatureMetadata.kt:15)."""
    bytes: bytes
    by: object                 # PublicKey or composite.CompositeKey
    platform_version: int = 1
    scheme_number_id: int = 4


@dataclass(frozen=True)
class BatchItem:
    public_key: object         # PublicKey or composite.CompositeKey
    signature_data: object     # bytes; composite.CompositeSignaturesWithKeys for a CompositeKey
    clear_data: bytes


def key_exception(public_key):
    """The exception the JVM raises building a key object from undecodable bytes [ext, recalled]."""
    if public_key is not None and public_key.scheme == EDDSA_ED25519_SHA512 and public_key.fmt == B.KEY_RAW:
        return IllegalArgumentException("not a valid point")
    return InvalidKeySpecException("This public key cannot be decoded, please ensure it is X509 encoded and that it "
                                   "corresponds to the input scheme's code name.")


class _Crypto:
    def __init__(self):
        self._engine = None
        self._lock = threading.Lock()
        self.last_errors = {}
        self._signers = []       # the private keys loaded into the engine, by signer index
        self._signer_pub = []    # their Abytes
        self._signer_engine = None
        self._ec_signers = []    # the ECDSA private keys loaded into the engine's ECDSA signer set
        self._ec_signer_pub = []  # their X || Y
        self._ec_signer_engine = None
        self._rsa_signers = []    # the RSA private keys loaded into the engine's RSA signer set
        self._rsa_signer_pub = []  # their (n, e)
        self._rsa_signer_engine = None

    def engine(self):
        with self._lock:
            if self._engine is None:
                self._engine = Engine(0)
            return self._engine

    def use_engine(self, engine):
        """Any object with ``verify(batch, mode)``: an Engine (one GPU) or an EnginePool."""
        with self._lock:
            self._engine = engine

    @staticmethod
    def find_signature_scheme(public_key):
        if public_key.scheme not in SCHEME_CODE_NAMES:
            raise IllegalArgumentException(f"Unsupported key/algorithm for schemeCodeName: {public_key.scheme}")
        return public_key.scheme

    @staticmethod
    def pack(items):
        b = B.BatchBuilder()
        for it in items:
            b.add_with_key(it.public_key.scheme, it.public_key.fmt, it.public_key.encoded, it.signature_data,
                           it.clear_data)
        return b.build()

    # ------------------------------------------------------------------ batch
    def verify_batch_ex(self, items, mode=B.MODE_DOVERIFY):
        """(status per item, {index: exception}) -- the exception map holds the items whose status
        is HOST_EXCEPTION (host-decided with an exception no C status expresses)."""
        from . import composite as C
        from . import hostverify
        n = len(items)
        st = np.full(n, B.NOT_RUN, dtype=np.uint8)
        errors = {}
        gpu = {B.MODE_DOVERIFY: [], B.MODE_ISVALID: []}   # (ref, BatchItem); ref = item index or (i, j) leaf
        leaves = {}                                        # composite item -> [leaf refs in order]
        host_leaf = {}                                     # (i, j) -> status / exception

        def host_scheme(scheme, pk, sig, msg, m):
            """(status, exception) of a host-verified scheme, isValid / doVerify semantics."""
            try:
                if scheme == RSA_SHA256:
                    key = hostverify.rsa_decode_key(pk.encoded)
                    if m == B.MODE_DOVERIFY and (len(sig) == 0 or len(msg) == 0):
                        return B.EMPTY, None
                    return (B.VALID if hostverify.rsa_verify(key, sig, msg) else B.INVALID), None
                if m == B.MODE_DOVERIFY and (len(sig) == 0 or len(msg) == 0):
                    return B.EMPTY, None
                hostverify.verify(scheme, pk, sig, msg)
            except Exception as e:  # noqa: BLE001 - the reference's exception, kept for the caller
                return HOST_EXCEPTION, e
            return B.NOT_RUN, None

        gpu_rsa = bool(getattr(self.engine(), "rsa", False))

        def on_gpu(pk):
            return pk.scheme in GPU_SCHEMES or (gpu_rsa and pk.scheme == RSA_SHA256 and pk.fmt == B.KEY_SPKI)

        for i, it in enumerate(items):
            pk = it.public_key
            if pk.scheme not in SCHEME_CODE_NAMES:
                st[i] = B.UNSUPPORTED
                continue
            if on_gpu(pk):
                gpu[mode].append((i, it))
                continue
            if pk.scheme != COMPOSITE_KEY:
                s, e = host_scheme(pk.scheme, pk, it.signature_data, it.clear_data, mode)
                st[i] = s
                if e is not None:
                    errors[i] = e
                continue
            # CompositeSignature engine (CompositeSignature.kt:75-84) behind doVerify / isValid
            try:
                key = pk if isinstance(pk, C.CompositeKey) else C.CompositeKey.get_instance(pk.encoded)
                sig = it.signature_data
                # doVerify's empty checks come first, signature then clear data (Crypto.kt:476-477),
                # before the engine deserialises anything
                if mode == B.MODE_DOVERIFY and not isinstance(sig, C.CompositeSignaturesWithKeys) and len(sig) == 0:
                    st[i] = B.EMPTY
                    continue
                if mode == B.MODE_DOVERIFY and len(it.clear_data) == 0:
                    st[i] = B.EMPTY
                    continue
                if not isinstance(sig, C.CompositeSignaturesWithKeys):
                    sig = C.CompositeSignaturesWithKeys.deserialize(sig)
                if not key.is_fulfilled_by([s.by for s in sig.sigs]):
                    st[i] = B.INVALID
                    continue
                if len(it.clear_data) != 32:
                    raise IllegalArgumentException("Failed requirement.")  # SecureHash.SHA256(buffer)
                refs = []
                for j, (s, msg) in enumerate(C.leaf_messages(sig, it.clear_data)):
                    ref = (i, j)
                    refs.append(ref)
                    if on_gpu(s.by):
                        gpu[B.MODE_ISVALID].append((ref, BatchItem(s.by, s.bytes, msg)))
                    else:  # RSA / SPHINCS leaves on the host; a composite leaf cannot be fulfilled
                        host_leaf[ref] = host_scheme(s.by.scheme, s.by, s.bytes, msg, B.MODE_ISVALID)
                leaves[i] = (refs, sig)
            except Exception as e:  # noqa: BLE001
                st[i] = HOST_EXCEPTION
                errors[i] = e

        leaf_st = {}
        for m, lst in gpu.items():
            if not lst:
                continue
            out = self.engine().verify(self.pack([b for _, b in lst]), m)
            for (ref, b), s in zip(lst, out):
                e = None
                if s == B.UNSUPPORTED and b.public_key.scheme == RSA_SHA256:  # a key the GPU declined
                    s, e = host_scheme(RSA_SHA256, b.public_key, b.signature_data, b.clear_data, m)
                if isinstance(ref, tuple):
                    leaf_st[ref] = (int(s), e)
                else:
                    st[ref] = s
                    if e is not None:
                        errors[ref] = e
        for ref, v in host_leaf.items():
            leaf_st[ref] = v
        # the `all { it.isValid(clearData) }` reduction: the first false or exception decides
        for i, (refs, sig) in leaves.items():
            verdict = B.VALID
            for j, ref in enumerate(refs):
                s, e = leaf_st[ref]
                if s == B.VALID:
                    continue
                if s == B.INVALID:
                    verdict = B.INVALID
                    break
                if e is None:
                    leaf = sig.sigs[j]
                    try:
                        self.raise_for_status(s, SCHEME_CODE_NAMES.get(leaf.by.scheme, ""), do_verify=False,
                                              key=leaf.by)
                    except Exception as x:  # noqa: BLE001
                        e = x
                errors[i] = e
                verdict = HOST_EXCEPTION
                break
            st[i] = verdict
        self.last_errors = errors
        return st, errors

    def verify_batch(self, items, mode=B.MODE_DOVERIFY):
        """Batch overload: list[BatchItem] -> numpy uint8 status per item (exceptions of host-decided
        items in ``last_errors``)."""
        if not items:
            self.last_errors = {}
            return np.zeros(0, dtype=np.uint8)
        return self.verify_batch_ex(items, mode)[0]

    # ------------------------------------------------------------------ status -> JVM outcome
    @staticmethod
    def raise_for_status(status, scheme_name="", do_verify=True, error=None, key=None):
        """The exception Crypto.doVerify (do_verify=True) / isValid would raise for `status`,
        or the return value (True / False)."""
        if status == B.VALID:
            return True
        if status == B.INVALID:
            if do_verify:
                raise SignatureException("Signature Verification failed!")
            return False
        if status == HOST_EXCEPTION:
            raise error if error is not None else RuntimeError("host-decided item without its exception")
        if status == B.SIG_MALFORMED:
            raise SignatureException("signature length is wrong" if scheme_name == "EDDSA_ED25519_SHA512"
                                     else "error decoding signature bytes.")
        if status == B.KEY_INVALID:
            raise key_exception(key)
        if status == B.UNSUPPORTED:
            raise IllegalArgumentException(f"Unsupported key/algorithm for schemeCodeName: {scheme_name}")
        if status == B.EMPTY:
            raise IllegalArgumentException("Signature data is empty!")
        raise RuntimeError(f"item not verified (status {status})")

    def _one(self, public_key, signature_data, clear_data, mode):
        scheme = self.find_signature_scheme(public_key)
        st, err = self.verify_batch_ex([BatchItem(public_key, signature_data, clear_data)], mode)
        s = int(st[0])
        if s == B.EMPTY:  # doVerify's own messages, signature first (Crypto.kt:476-477)
            sig_empty = isinstance(signature_data, (bytes, bytearray)) and len(signature_data) == 0
            raise IllegalArgumentException("Signature data is empty!" if sig_empty
                                           else "Clear data is empty, nothing to verify!")
        return self.raise_for_status(s, SCHEME_CODE_NAMES[scheme], do_verify=mode == B.MODE_DOVERIFY,
                                     error=err.get(0), key=public_key)

    def do_verify(self, public_key, signature_data, clear_data):
        """Crypto.doVerify(publicKey, signatureData, clearData) (Crypto.kt:457 -> :474-484)."""
        return self._one(public_key, signature_data, clear_data, B.MODE_DOVERIFY)

    def is_valid(self, public_key, signature_data, clear_data):
        """Crypto.isValid(publicKey, signatureData, clearData) (Crypto.kt:536 -> :553-559)."""
        return self._one(public_key, signature_data, clear_data, B.MODE_ISVALID)

    # ------------------------------------------------------------------ signing
    def _sign_scheme(self, private_key, clear_len, random=None):
        """doSign's checks in its order (Crypto.kt:396-398), then the mirror's own limit."""
        if private_key.scheme not in SCHEME_CODE_NAMES or private_key.scheme == COMPOSITE_KEY:
            raise IllegalArgumentException(f"Unsupported key/algorithm for schemeCodeName: {private_key.scheme}")
        if clear_len == 0:
            raise Exception("Signing of an empty array is not permitted!")
        if private_key.scheme in _ECDSA_SCHEMES and random is not None:
            if len(private_key.encoded) != 32:
                raise InvalidKeyException("an ECDSA private key is 32 bytes of d, big-endian")
            return
        if private_key.scheme == RSA_SHA256 and random is not None:
            self._rsa_parts(private_key)
            return
        if private_key.scheme != EDDSA_ED25519_SHA512:
            raise UnsupportedOperationException(
                f"no signer for scheme {SCHEME_CODE_NAMES[private_key.scheme]} in this mirror; the JVM caller keeps "
                "its own Crypto.doSign")
        if len(private_key.encoded) != 32:
            raise InvalidKeyException("an Ed25519 private key is a 32-byte seed")

    def _signer(self, private_key):
        """(signer index, Abyte) of a key in the engine's signer set, loading it when it is new."""
        eng = self.engine()
        with self._lock:
            if self._signer_engine is not eng:
                self._signers, self._signer_pub, self._signer_engine = [], [], eng
            if private_key not in self._signers:
                keys = self._signers + [private_key]
                self._signer_pub = eng.load_signers([k.encoded for k in keys])
                self._signers = keys
            i = self._signers.index(private_key)
            return i, self._signer_pub[i]

    def _ec_signer(self, private_key):
        """(signer index, X || Y) of a key in the engine's ECDSA signer set, loading it when it is new."""
        eng = self.engine()
        with self._lock:
            if self._ec_signer_engine is not eng:
                self._ec_signers, self._ec_signer_pub, self._ec_signer_engine = [], [], eng
            if private_key not in self._ec_signers:
                # the range check on the host, before anything is loaded: the device set and this list
                # never disagree (Crypto never makes a key outside [1, n - 1])
                if not 0 < int.from_bytes(private_key.encoded, "big") < _EC_ORDER[private_key.scheme]:
                    raise InvalidKeyException("the ECDSA private key is not in [1, n - 1]")
                keys = self._ec_signers + [private_key]
                pubs, st = eng.load_ec_signers([(k.scheme, k.encoded) for k in keys])
                if any(int(x) != 0 for x in st):
                    raise InvalidKeyException("the device refused an ECDSA private key")
                self._ec_signer_pub, self._ec_signers = pubs, keys
            i = self._ec_signers.index(private_key)
            return i, self._ec_signer_pub[i]

    @staticmethod
    def _rsa_parts(private_key):
        """The CRT parts of a PKCS#8 RSA key, or the mirror's refusals."""
        from . import hostverify
        key = hostverify.rsa_decode_private_key(private_key.encoded)
        if key["e"] >= 1 << 32:
            raise UnsupportedOperationException("an RSA public exponent of 2^32 or more does not fit the C ABI's "
                                                "32-bit e; the JVM caller keeps its own Crypto.doSign")
        return key

    def _rsa_signer(self, private_key):
        """(signer index, (n, e)) of a key in the engine's RSA signer set, loading it when it is new."""
        from .engine import RsaSignerKey
        eng = self.engine()
        with self._lock:
            if self._rsa_signer_engine is not eng:
                self._rsa_signers, self._rsa_signer_pub, self._rsa_signer_engine = [], [], eng
            if private_key not in self._rsa_signers:
                keys = self._rsa_signers + [private_key]
                parts = [self._rsa_parts(k) for k in keys]
                be = lambda v: v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")  # noqa: E731
                st = eng.load_rsa_signers([RsaSignerKey(be(k["n"]), k["e"], be(k["p"]), be(k["q"]), be(k["dp"]),
                                                        be(k["dq"]), be(k["qinv"])) for k in parts])
                if any(int(x) != 0 for x in st):
                    self._rsa_signers, self._rsa_signer_pub = [], []  # the device set was replaced
                    raise InvalidKeyException("the device refused an RSA private key")
                self._rsa_signer_pub, self._rsa_signers = [(k["n"], k["e"]) for k in parts], keys
            i = self._rsa_signers.index(private_key)
            return i, self._rsa_signer_pub[i]

    def _rsa_salts(self, n, random):
        """PSSSigner's random.nextBytes(salt): one 32-byte draw per signature, never redrawn."""
        salts = np.zeros(32 * n, dtype=np.uint8)
        for j in range(n):
            s = random(32)
            if len(s) != 32:
                raise ValueError("random(32) must return 32 bytes")
            salts[32 * j:32 * j + 32] = np.frombuffer(s, dtype=np.uint8)
        return salts

    def forget_signers(self):
        """Zeroes and frees the engine's signer sets (cg_signers_clear, cg_ec_signers_clear,
        cg_rsa_signers_clear)."""
        with self._lock:
            if self._signer_engine is not None:
                self._signer_engine.clear_signers()
            self._signers, self._signer_pub, self._signer_engine = [], [], None
            if self._ec_signer_engine is not None:
                self._ec_signer_engine.clear_ec_signers()
            self._ec_signers, self._ec_signer_pub, self._ec_signer_engine = [], [], None
            if self._rsa_signer_engine is not None:
                self._rsa_signer_engine.clear_rsa_signers()
            self._rsa_signers, self._rsa_signer_pub, self._rsa_signer_engine = [], [], None

    def _ec_sign_loop(self, n, random, call):
        """ECDSASigner.generateSignature's loop over a batch: every pending item gets one 32-byte draw
        (BigInteger(256, random)), ``call(pending, nonces)`` signs them, and only the items that came back
        NONCE_REJECTED are redrawn. The nonce array is zeroed by the engine call that read it."""
        out, pending = [None] * n, list(range(n))
        while pending:
            nonces = np.zeros(32 * len(pending), dtype=np.uint8)
            for j in range(len(pending)):
                k = random(32)
                if len(k) != 32:
                    raise ValueError("random(32) must return 32 bytes")
                nonces[32 * j:32 * j + 32] = np.frombuffer(k, dtype=np.uint8)
            try:
                sigs, ln, st = call(pending, nonces)
            finally:
                nonces[:] = 0
            again = []
            for j, i in enumerate(pending):
                if int(st[j]) == B.NONCE_REJECTED:
                    again.append(i)
                    continue
                self._sign_status(int(st[j]))
                out[i] = sigs[j, :int(ln[j])].tobytes()
            pending = again
        return out

    @staticmethod
    def _sign_status(status):
        if status == B.EMPTY:
            raise Exception("Signing of an empty array is not permitted!")
        if status != 0:
            raise RuntimeError(f"item not signed (status {status})")

    def do_sign(self, private_key, clear_data, random=None):
        """Crypto.doSign(privateKey, clearData) (Crypto.kt:395-402). ``random``: see the module text; without
        it an ECDSA or RSA key raises UnsupportedOperationException."""
        clear_data = bytes(clear_data)
        self._sign_scheme(private_key, len(clear_data), random)
        if private_key.scheme == RSA_SHA256:
            i, _ = self._rsa_signer(private_key)
            salts = self._rsa_salts(1, random)
            try:
                sigs, ln, st = self.engine().sign_rsa([(i, clear_data)], salts)
            finally:
                salts[:] = 0
            self._sign_status(int(st[0]))
            return sigs[0, :int(ln[0])].tobytes()
        if private_key.scheme in _ECDSA_SCHEMES:
            i, _ = self._ec_signer(private_key)
            return self._ec_sign_loop(1, random, lambda pend, k: self.engine().sign_ec([(i, clear_data)], k))[0]
        i, _ = self._signer(private_key)
        sigs, st = self.engine().sign([(i, clear_data)])
        self._sign_status(int(st[0]))
        return sigs[0].tobytes()

    def _aligned_signer(self, key_pair, random=None):
        """The key-pair check of Crypto.kt:416-419, then the signer index."""
        sig_key = self.find_signature_scheme(key_pair.private)
        sig_meta = self.find_signature_scheme(key_pair.public)
        if sig_key != sig_meta:
            raise IllegalArgumentException(f"Metadata schemeCodeName: {SCHEME_CODE_NAMES[sig_meta]} is not aligned with "
                                           f"the key type: {SCHEME_CODE_NAMES[sig_key]}.")
        self._sign_scheme(key_pair.private, 1, random)
        if key_pair.private.scheme == RSA_SHA256:
            from . import hostverify
            i, ne = self._rsa_signer(key_pair.private)
            if hostverify.rsa_decode_key(key_pair.public.encoded) != ne:
                raise IllegalArgumentException("The public key of this pair is not the private key's.")
            return i
        if key_pair.private.scheme in _ECDSA_SCHEMES:
            i, xy = self._ec_signer(key_pair.private)
            if K.canonical_spki(key_pair.private.scheme, B.KEY_RAW, xy) != key_pair.public.spki():
                raise IllegalArgumentException("The public key of this pair is not the private key's.")
            return i
        i, abyte = self._signer(key_pair.private)
        if K.canonical_spki(EDDSA_ED25519_SHA512, B.KEY_RAW, abyte) != key_pair.public.spki():
            raise IllegalArgumentException("The public key of this pair is not the private key's.")
        return i

    def do_sign_tx(self, key_pair, signable_data, random=None):
        """Crypto.doSign(keyPair, signableData) (Crypto.kt:415-422) -> TransactionSignature."""
        return self.sign_all(key_pair, [signable_data.tx_id],
                             (signable_data.platform_version, signable_data.scheme_number_id), random=random)[0]

    def sign_all(self, key_pair, tx_ids, metadata=(1, 4), random=None):
        """NotaryService.sign(txId) (NotaryService.kt:77-80) for every id in one call:
        Crypto.doSign(keyPair, SignableData(txId, SignatureMetadata(*metadata))) each. ``random``: see the
        module text; without it an ECDSA key pair raises UnsupportedOperationException."""
        from . import signable
        signer = self._aligned_signer(key_pair, random)
        if not tx_ids:
            return []
        pv, sid = metadata
        if key_pair.private.scheme == RSA_SHA256:
            b = B.SignRequestBuilder()
            t = b.template(*signable.template(pv, sid))
            for tx_id in tx_ids:
                b.add_request(signer, b.tx_id(tx_id), t)
            salts = self._rsa_salts(len(tx_ids), random)
            try:
                sigs, ln, st = self.engine().sign_rsa_tx_ids(b.build(), salts)
            finally:
                salts[:] = 0
            for s in st:
                self._sign_status(int(s))
            return [TransactionSignature(sigs[j, :int(ln[j])].tobytes(), key_pair.public, pv, sid)
                    for j in range(len(tx_ids))]
        if key_pair.private.scheme in _ECDSA_SCHEMES:
            def call(pending, nonces):
                b = B.SignRequestBuilder()
                t = b.template(*signable.template(pv, sid))
                for i in pending:
                    b.add_request(signer, b.tx_id(tx_ids[i]), t)
                return self.engine().sign_ec_tx_ids(b.build(), nonces)
            return [TransactionSignature(sig, key_pair.public, pv, sid)
                    for sig in self._ec_sign_loop(len(tx_ids), random, call)]
        b = B.SignRequestBuilder()
        t = b.template(*signable.template(pv, sid))
        for tx_id in tx_ids:
            b.add_request(signer, b.tx_id(tx_id), t)
        sigs, st = self.engine().sign_tx_ids(b.build())
        for s in st:
            self._sign_status(int(s))
        return [TransactionSignature(sigs[j].tobytes(), key_pair.public, pv, sid) for j in range(len(tx_ids))]

    # ------------------------------------------------------------------ key derivation
    @staticmethod
    def _derive_scheme(scheme):
        """deriveKeyPair's checks in its order (Crypto.kt:647-653)."""
        if scheme not in SCHEME_CODE_NAMES or scheme == COMPOSITE_KEY:
            raise IllegalArgumentException(f"Unsupported key/algorithm for schemeCodeName: {scheme}")
        if scheme not in GPU_SCHEMES:
            raise UnsupportedOperationException(
                "Although supported for signing, deterministic key derivation is not currently implemented for "
                f"{SCHEME_CODE_NAMES[scheme]}")

    @staticmethod
    def _key_pair(scheme, secret, pub):
        return KeyPair(PublicKey(scheme, pub[:32] if scheme == EDDSA_ED25519_SHA512 else pub, B.KEY_RAW),
                       PrivateKey(scheme, secret))

    def derive_key_pairs(self, private_key, seeds, scheme=None):
        """Crypto.deriveKeyPair(privateKey, seed) for every seed in one call (cg_derive_keys)."""
        from . import derive as D
        scheme = private_key.scheme if scheme is None else scheme
        self._derive_scheme(scheme)
        if len(private_key.encoded) != 32:
            raise InvalidKeyException("a private key is 32 bytes: an Ed25519 seed, or an ECDSA d big-endian")
        seeds = [bytes(s) for s in seeds]
        if not seeds:
            return []
        b = B.DeriveRequestBuilder()
        parent = b.parent(scheme, private_key.encoded)
        for s in seeds:
            b.add_request(parent, s)
        dr = b.build()
        try:
            secrets, pubs, st, _ = self.engine().derive_keys(dr)
        finally:
            dr.wipe()
        out = []
        for j, s in enumerate(seeds):
            if st[j] == 0:
                out.append(self._key_pair(scheme, secrets[j].tobytes(), pubs[j].tobytes()))
            elif st[j] == B.DERIVE_HOST:
                d, q, _ = D.derive_ecdsa(scheme, D.key_data(scheme, private_key.encoded), s)
                out.append(self._key_pair(scheme, d, q))
            else:
                raise RuntimeError(f"key not derived (status {int(st[j])})")
        return out

    def derive_key_pair(self, private_key, seed, scheme=None):
        """Crypto.deriveKeyPair(signatureScheme, privateKey, seed) (Crypto.kt:646-654)."""
        return self.derive_key_pairs(private_key, [seed], scheme)[0]

    def _public(self, scheme, secret):
        pubs, st = self.engine().public_keys(scheme, [secret])
        return int(st[0]), pubs[0].tobytes()

    def derive_key_pair_from_entropy(self, entropy, scheme=EDDSA_ED25519_SHA512):
        """Crypto.deriveKeyPairFromEntropy (Crypto.kt:738-757): the seed is entropy.toByteArray() padded
        with zeros (or cut) to 32 bytes."""
        if scheme != EDDSA_ED25519_SHA512:
            raise IllegalArgumentException("Unsupported signature scheme for fixed entropy-based key pair generation: "
                                           f"{SCHEME_CODE_NAMES.get(scheme, scheme)}")
        n = int(entropy)
        tb = n.to_bytes((n.bit_length() + 8) // 8 if n >= 0 else ((-n - 1).bit_length() + 8) // 8, "big", signed=True)
        seed = (tb + bytes(32))[:32]
        st, pub = self._public(scheme, seed)
        if st != 0:
            raise RuntimeError(f"public key not computed (status {st})")
        return self._key_pair(scheme, seed, pub)

    def generate_key_pair(self, scheme=EDDSA_ED25519_SHA512):
        """Crypto.generateKeyPair for the three curves: 32 (Ed25519) or 256 bits (BC ECKeyPairGenerator's
        BigInteger(nBitLength, random)) drawn on the host; an ECDSA candidate the accept rule refuses is
        redrawn, as BC's loop does."""
        import secrets as _secrets
        self._derive_scheme(scheme)
        while True:
            secret = _secrets.token_bytes(32)
            st, pub = self._public(scheme, secret)
            if st == 0:
                return self._key_pair(scheme, secret, pub)
            if st != B.KEY_REJECTED:
                raise RuntimeError(f"public key not computed (status {st})")

    def do_verify_tx(self, tx_id, ts):
        """Crypto.doVerify(txId, transactionSignature) (Crypto.kt:499-502)."""
        from . import signable
        pre, suf = signable.template(ts.platform_version, ts.scheme_number_id)
        return self.do_verify(ts.by, ts.bytes, pre + bytes(tx_id) + suf)

    def is_valid_tx(self, tx_id, ts):
        """Crypto.isValid(txId, transactionSignature) (Crypto.kt:516-519)."""
        from . import signable
        pre, suf = signable.template(ts.platform_version, ts.scheme_number_id)
        return self.is_valid(ts.by, ts.bytes, pre + bytes(tx_id) + suf)


Crypto = _Crypto()
