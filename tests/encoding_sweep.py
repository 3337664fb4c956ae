"""Byte-level sweeps of signature and key encodings (test helper).

Every other fixture pins the decoders in front of the arithmetic with a few hand-picked cases per
class. The sweeps here derive thousands of encodings from a few base vectors (fixed private scalars
and nonces for both curves, one Ed25519 seed), deterministically and in a fixed order:

  mut(x, full_at)   every proper prefix of x; x extended by 1, 2, 3, 4, 8, 13 and 60 zero bytes; at
                    every position each distinct value of {00 01 02 03 04 30 7f 80 81 ff, x[i] +- 1,
                    x[i] ^ 0x80, x[i] ^ 1}; at the positions `full_at` all 255 other values.

  a  ECDSA signatures   per curve a low-S base signature (33 / 32 content bytes) and a high-S one
                        (32 / 33) under the key d = n - 5: mut with full_at = bytes 0..5 and the second
                        INTEGER's tag and length; the 0x84 length probes (a 4-byte length near 2^32
                        in either INTEGER, body unchanged); well-formed long encodings (r or s a
                        positive value of 32 + e content bytes, r a negative one); one encoding of
                        exactly 65,535 bytes (the limit of cg_item.sig_len).
  b  Ed25519 signatures mut with full_at = {31, 63}: every sign / high-y pattern of R, every top
                        byte of S.
  c  Ed25519 keys       mut of RAW(32) (full_at = {31}), the 44-byte SPKI and the 46-byte
                        NULL-parameter SPKI; each verifies the one good signature.
  d  EC keys            per curve mut of RAW(64), SEC1 04 / 02|03 / 06|07 (the tag of y's parity),
                        and the SPKI around the uncompressed and the compressed point; full_at = the
                        point's tag byte and the two SPKI length bytes that depend on the point length.
  e  precedence         per scheme {decodable, undecodable (off the curve; for Ed25519 the smallest
                        y with no x: i2p reduces a y >= p), unsupported scheme id, key_idx past the
                        table} x {good, parses-but-wrong, malformed, empty signature} x {message,
                        empty message}.

The base signatures of a and b sign SignableData(id) = prefix || id || suffix of one template of
layout_util.TMPL_LENS with a prefix of more than one SHA-256 block, so the same bytes pack as a
tx-signature batch (`txsig_batch`) and, through txsig_util.to_message_batch, as a plain one.

An item is an `Item`; expected statuses are recorded in tests/golden/encoding_sweep.json as one
digit per item and mode (`DIGIT`: the status code, 9 for NOT_RUN)."""
import collections
import hashlib

import numpy as np

from corda_amd import batch as B
from oracle import corda, ecdsa_bc, ed25519_i2p as ed

Item = collections.namedtuple("Item", "note scheme fmt key sig msg past base")
Item.__new__.__defaults__ = (False, None)

# ---------------------------------------------------------------- base vectors
D_LOW = {2: 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1,
         3: 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE}
D_HIGH = {s: ecdsa_bc.CURVES[s].n - 5 for s in (2, 3)}
# the first nonce tried; the search steps by one until r and s have the content lengths wanted
K_FIRST = {2: 0x0C0FFEE0DDBA11C0FFEE0123456789ABCDEF02468ACE13579BDF0FEDCBA98765,
           3: 0x5CA1AB1E0FEDCBA98765432100123456789ABCDEF13579BDF020DDBA11C0FFEE}
ED_SEED = bytes.fromhex("4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb")
TMPL = (79, 1)  # layout_util.TMPL_LENS: the id crosses the second SHA-256 block's end
PREFIX = bytes((37 * i + 11) & 255 for i in range(TMPL[0]))
SUFFIX = b"\x5a"
BASE_NAMES = ("k1_low", "k1_high", "r1_low", "r1_high", "ed")  # base j signs id j
IDS = [hashlib.sha256(b"encoding sweep id %d" % j).digest() for j in range(len(BASE_NAMES))]
UNSUPPORTED_SCHEME = 5  # SPHINCS-256: no device scheme, and not RSA (whose keys a flag routes)

EXT = (1, 2, 3, 4, 8, 13, 60)
FIXED = (0x00, 0x01, 0x02, 0x03, 0x04, 0x30, 0x7F, 0x80, 0x81, 0xFF)
LONG_E = (1, 8, 9, 10, 11, 12, 13, 48, 49, 55, 56, 57, 100, 200, 250, 300, 1000, 30000)
WRAP_LENS = (0xFFFFFFFA, 0xFFFFFFFF, 0x80000000, 0x00010000)
FULL_TAG = " (of all 255)"  # ends the note of a mutation at a `full_at` position
DIGIT = {B.VALID: "0", B.INVALID: "1", B.SIG_MALFORMED: "2", B.KEY_INVALID: "3", B.UNSUPPORTED: "4", B.EMPTY: "5",
         B.NOT_RUN: "9"}
STATUS_OF_DIGIT = {d: s for s, d in DIGIT.items()}


def message(j):
    return PREFIX + IDS[j] + SUFFIX


def mut(x, full_at=()):
    """(note, bytes) for every mutation of x, in a fixed order; none equals x."""
    x = bytes(x)
    for n in range(len(x)):
        yield f"cut to {n}", x[:n]
    for e in EXT:
        yield f"extended by {e}", x + bytes(e)
    full = set(full_at)
    assert all(0 <= i < len(x) for i in full)
    for i, b in enumerate(x):
        if i in full:
            vals = [v for v in range(256) if v != b]
        else:
            vals = []
            for v in FIXED + ((b + 1) & 255, (b - 1) & 255, b ^ 0x80, b ^ 1):
                if v != b and v not in vals:
                    vals.append(v)
        for v in vals:
            yield f"byte {i} = {v:02x}" + (FULL_TAG if i in full else ""), x[:i] + bytes([v]) + x[i + 1:]


_BASE = None


def _ec_base(scheme, d, msg, high):
    """(k, r, s): the first nonce from K_FIRST[scheme] whose signature has 33 / 32 content bytes
    (low-S: r >= 2^255, 2^247 <= s < 2^255) or 32 / 33 (high-S: s >= 2^255)."""
    n, k = ecdsa_bc.CURVES[scheme].n, K_FIRST[scheme]
    while True:
        r, s = ecdsa_bc.sign(scheme, d, msg, k)
        s = max(s, n - s) if high else min(s, n - s)
        big, small = (s, r) if high else (r, s)
        if big >> 255 and small >> 247 and not small >> 255:
            return k, r, s
        k += 1


def base():
    """The base vectors: name -> {scheme, d / seed, k, key (raw), r, s, sig, id}."""
    global _BASE
    if _BASE is None:
        out = {}
        for j, name in enumerate(BASE_NAMES[:4]):
            scheme, high = (2 if name.startswith("k1") else 3), name.endswith("high")
            d = (D_HIGH if high else D_LOW)[scheme]
            k, r, s = _ec_base(scheme, d, message(j), high)
            sig = ecdsa_bc.der_encode_sig(r, s)
            assert len(sig) == 71 and sig[3] == (32 if high else 33)
            out[name] = {"scheme": scheme, "d": d, "k": k, "r": r, "s": s, "sig": sig, "id": j,
                         "key": ecdsa_bc.raw_key(ecdsa_bc.public_point(scheme, d))}
        out["ed"] = {"scheme": 4, "seed": ED_SEED, "key": ed.public_from_seed(ED_SEED), "sig": ed.sign(ED_SEED, message(4)),
                     "id": 4}
        _BASE = out
    return _BASE


def base_record():
    out = {}
    for name, b in base().items():
        v = {"scheme": b["scheme"], "id": b["id"], "key": b["key"].hex(), "sig": b["sig"].hex()}
        if name == "ed":
            v["seed"] = b["seed"].hex()
        else:
            v.update({f: "%064x" % b[f] for f in ("d", "k", "r", "s")})
        out[name] = v
    return out


# ---------------------------------------------------------------- a, b: signatures
def long_encodings(r, s):
    """Well-formed DER with an INTEGER of 32 + e content bytes: positive r, positive s, negative r."""
    for e in LONG_E:
        n = 32 + e
        hi, lo = 1 << (8 * n - 2), -(1 << (8 * n - 1))
        for note, sig in ((f"r positive, {n} bytes", ecdsa_bc.der_encode_sig(hi + r, s)),
                          (f"s positive, {n} bytes", ecdsa_bc.der_encode_sig(r, hi + s)),
                          (f"r negative, {n} bytes", ecdsa_bc.der_encode_sig(lo + r, s))):
            yield note, sig


def max_encoding(r, s):
    """SEQUENCE{r, s'} of exactly 65,535 bytes: s' = s under a positive pad."""
    n = B.SIG_LEN_MAX - 4 - len(ecdsa_bc.der_encode_int(r)) - 4
    sig = ecdsa_bc.der_encode_sig(r, (1 << (8 * n - 2)) + s)
    assert len(sig) == B.SIG_LEN_MAX
    return sig


def wrap_probes(sig):
    """The length byte of either INTEGER replaced by 84 xx xx xx xx (body unchanged, the SEQUENCE
    length raised by the 4 bytes added, so the parse reaches the INTEGER)."""
    for which, at in (("r", 3), ("s", 5 + sig[3])):
        for v in WRAP_LENS:
            out = bytearray(sig[:at] + b"\x84" + v.to_bytes(4, "big") + sig[at + 1:])
            out[1] += 4
            yield f"{which} length 84 {v:08x}", bytes(out)


def sweep_a():
    out = []
    for name in BASE_NAMES[:4]:
        b = base()[name]
        msg, sig = message(b["id"]), b["sig"]

        def add(note, s):
            out.append(Item(f"{name}: {note}", b["scheme"], B.KEY_RAW, b["key"], s, msg, False, name))

        add("base", sig)
        for note, s in mut(sig, full_at=(0, 1, 2, 3, 4, 5, 4 + sig[3], 5 + sig[3])):
            add(note, s)
        for note, s in wrap_probes(sig):
            add(note, s)
        for note, s in long_encodings(b["r"], b["s"]):
            add(note, s)
    b = base()["k1_low"]  # last: a relaid-out arena can end on it
    out.append(Item("k1_low: 65535 bytes", 2, B.KEY_RAW, b["key"], max_encoding(b["r"], b["s"]), message(b["id"]), False,
                    "k1_low"))
    return out


def sweep_b():
    b = base()["ed"]
    msg = message(b["id"])
    out = [Item("ed: base", 4, B.KEY_RAW, b["key"], b["sig"], msg, False, "ed")]
    out += [Item(f"ed: {note}", 4, B.KEY_RAW, b["key"], s, msg, False, "ed") for note, s in mut(b["sig"], full_at=(31, 63))]
    return out


# ---------------------------------------------------------------- c, d: keys
def ed_key_forms():
    a = base()["ed"]["key"]
    return [("ed raw", B.KEY_RAW, a, (31,)), ("ed spki", B.KEY_SPKI, corda.ED25519_SPKI_PREFIX + a, ()),
            ("ed spki-null", B.KEY_SPKI, corda.ED25519_SPKI_PREFIX_NULL + a, ())]


def ec_key_forms(scheme):
    name = "k1" if scheme == 2 else "r1"
    raw = base()[name + "_low"]["key"]
    x, odd = raw[:32], raw[63] & 1
    p65, p33 = ecdsa_bc.spki_prefix(scheme, 65), ecdsa_bc.spki_prefix(scheme, 33)
    lens = lambda pre: (1, len(pre) - 2, len(pre))  # noqa: E731  SEQUENCE length, BIT STRING length, point tag
    return [(name + " raw", B.KEY_RAW, raw, ()), (name + " sec1 04", B.KEY_SEC1, b"\x04" + raw, (0,)),
            (name + " sec1 compressed", B.KEY_SEC1, bytes([2 | odd]) + x, (0,)),
            (name + " sec1 hybrid", B.KEY_SEC1, bytes([6 | odd]) + raw, (0,)),
            (name + " spki", B.KEY_SPKI, p65 + b"\x04" + raw, lens(p65)),
            (name + " spki compressed", B.KEY_SPKI, p33 + bytes([2 | odd]) + x, lens(p33))]


def _key_sweep(scheme, forms, good):
    msg = message(good["id"])
    out = []
    for name, fmt, key, full_at in forms:
        out.append(Item(f"{name}: base", scheme, fmt, key, good["sig"], msg))
        out += [Item(f"{name}: {note}", scheme, fmt, k, good["sig"], msg) for note, k in mut(key, full_at)]
    return out


def sweep_c():
    return _key_sweep(4, ed_key_forms(), base()["ed"])


def sweep_d():
    return _key_sweep(2, ec_key_forms(2), base()["k1_low"]) + _key_sweep(3, ec_key_forms(3), base()["r1_low"])


def d_base_keys():
    """(scheme, fmt, key, sig, msg) of sweep d's undamaged encodings."""
    return [(it.scheme, it.fmt, it.key, it.sig, it.msg) for it in sweep_d() if it.note.endswith(": base")]


# ---------------------------------------------------------------- e: precedence
def _ed_decodes(key):
    try:
        ed.decode_point(key)
        return True
    except ed.KeyDecodeError:
        return False


def sweep_e():
    """key state x signature state x message state, per scheme. The good signature is good for the
    cell's message (the empty one too: VALID under isValid); parses-but-wrong is the good
    signature of the other message."""
    out = []
    for scheme, name in ((2, "k1_low"), (3, "r1_low"), (4, "ed")):
        b = base()[name]
        msg = message(b["id"])
        if scheme == 4:
            good = {msg: b["sig"], b"": ed.sign(ED_SEED, b"")}
            malformed = b["sig"][:63]
            bad_key = next(k for k in (bytes([y]) + bytes(31) for y in range(2, 256)) if not _ed_decodes(k))
        else:
            good = {msg: b["sig"], b"": ecdsa_bc.der_encode_sig(*ecdsa_bc.sign(scheme, b["d"], b"", b["k"]))}
            malformed = b["sig"][:-1]
            bad_key = b["key"][:63] + bytes([b["key"][63] ^ 1])  # off the curve
        keys = (("decodable", scheme, b["key"], False), ("undecodable", scheme, bad_key, False),
                ("unsupported scheme", UNSUPPORTED_SCHEME, b["key"], False), ("key_idx past", scheme, b["key"], True))
        for kn, ks, kb, past in keys:
            for m, mn in ((msg, "message"), (b"", "empty message")):
                sigs = (("good", good[m]), ("wrong", good[b"" if m else msg]), ("malformed", malformed), ("empty", b""))
                for sn, s in sigs:
                    out.append(Item(f"scheme {scheme}: {kn} key, {sn} signature, {mn}", ks, B.KEY_RAW, kb, s, m, past))
    return out


SWEEPS = {"a": sweep_a, "b": sweep_b, "c": sweep_c, "d": sweep_d, "e": sweep_e}
_CACHE = {}


def sweep(name):
    if name not in _CACHE:
        _CACHE[name] = SWEEPS[name]()
    return _CACHE[name]


# ---------------------------------------------------------------- packing
def txsig_batch(items):
    """Items of sweeps a / b as one TxSigBatch: the five raw keys, the five ids, the one template."""
    bld = B.TxSigBuilder()
    tmpl = bld.template(PREFIX, SUFFIX)
    keys = {n: bld.key(base()[n]["scheme"], B.KEY_RAW, base()[n]["key"]) for n in BASE_NAMES}
    ids = [bld.tx_id(i) for i in IDS]
    for it in items:
        assert it.base is not None and it.msg == message(base()[it.base]["id"]) and len(it.sig) <= B.SIG_LEN_MAX
        bld.add_signature(keys[it.base], ids[base()[it.base]["id"]], tmpl, it.sig)
    return bld.build()


def key_batch(items, extra=()):
    """Items as a plain Batch, one key-table entry per distinct (scheme, fmt, key bytes); an item
    with `past` points behind the key table. `extra`: (scheme, fmt, key, sig, msg, count) items
    appended after them."""
    bld = B.BatchBuilder()
    for it in items:
        bld.add_with_key(it.scheme, it.fmt, it.key, it.sig, it.msg)
    for scheme, fmt, key, sig, msg, count in extra:
        k = bld.key(scheme, fmt, key)
        for _ in range(count):
            bld.add(k, sig, msg)
    b = bld.build()
    for j, it in enumerate(items):
        if it.past:
            b.items["key_idx"][j] = len(b.keys) + j
    return b


def status_array(digits):
    return np.array([STATUS_OF_DIGIT[c] for c in digits], dtype=np.uint8)


def digits_of(statuses):
    return "".join(DIGIT[int(s)] for s in statuses)
