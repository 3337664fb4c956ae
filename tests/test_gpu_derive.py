"""GPU tests of key derivation (cg_derive_keys, cg_public_keys and their device and pool forms):
Crypto.deriveKeyPair (Crypto.kt:646-771) byte for byte. The yardsticks: tests/golden/derive_keys.json
(tests/derive_ref.py cross-checked against OpenSSL) and tests/derive_ref.py itself. Sizes are the
smallest that reach each edge: one inversion run is 64 lanes x 16 items = 1,024 requests."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import derive_ref as R
import layout_util as LU
from corda_amd import _lib
from corda_amd import batch as B
from oracle import ecdsa_bc, ed25519_i2p as ed

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RUN = 64 * 16  # requests of one inversion run (derive_keys.hip DERIVE_RUN_K)


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def fixture_requests(fx):
    b = B.DeriveRequestBuilder()
    for p in fx["parents"]:
        b.parent_key_data(p["scheme"], bytes.fromhex(p["key_data"]))
    for r in fx["records"]:
        b.add_request(r["parent"], bytes.fromhex(r["seed"]))
    return b.build()


def check_fixture(fx, secrets, pubs, st, tries):
    assert not st.any() and not tries.any()
    for j, r in enumerate(fx["records"]):
        assert secrets[j].tobytes().hex() == r["secret"], (j, r["note"])
        assert pubs[j].tobytes().hex() == r["pub"], (j, r["note"])


PARENTS7 = [(R.ED, ed.entropy_seed(20)), (R.R1, (2 ** 255 + 12345).to_bytes(32, "big")), (R.K1, (0x80).to_bytes(32, "big")),
            (R.ED, bytes(range(32))), (R.K1, hashlib.sha256(b"k1 parent").digest()), (R.R1, (1).to_bytes(32, "big")),
            (R.ED, hashlib.sha256(b"ed parent").digest())]


def key_data(scheme, private):
    return R.key_data_ed(private) if scheme == R.ED else R.key_data_ec(int.from_bytes(private, "big"))


def mixed(n, salt=0):
    """n requests over the 7 parents, the schemes interleaved, seeds of 0..40 bytes."""
    b = B.DeriveRequestBuilder()
    for scheme, private in PARENTS7:
        b.parent(scheme, private)
    rows = []
    for j in range(n):
        seed = hashlib.sha256(b"%d/%d" % (salt, j)).digest() * 2
        seed = seed[:(j * 7 + salt) % 41]
        b.add_request(j % 7, seed)
        rows.append((j % 7, seed))
    return b.build(), rows


@pytest.fixture(scope="module")
def mixed4099():
    """4,099 mixed requests and, computed once, what derive_ref gives for a sample of them: every
    request of the first 130 (two waves), of both sides of every inversion-run boundary and of the tail."""
    dr, rows = mixed(4099)
    sample = sorted(set(range(130)) | {j for e in (RUN, 2 * RUN, 3 * RUN, 4 * RUN) for j in range(e - 3, e + 3)} |
                    set(range(4090, 4099)) | set(range(0, 4099, 97)))
    want = {}
    for j in sample:
        p, seed = rows[j]
        scheme, private = PARENTS7[p]
        want[j] = R.derive(scheme, key_data(scheme, private), seed)
    return dr, rows, want


def check_sample(want, secrets, pubs, st, tries, limit=None):
    assert not st.any() and not tries.any()
    for j, (secret, pub, _) in want.items():
        if limit is None or j < limit:
            assert secrets[j].tobytes() == secret and pubs[j].tobytes() == pub, j


# 1 ---------------------------------------------------------------- the fixture, three forms
def test_fixture_host_form(engine, fx):
    check_fixture(fx, *engine.derive_keys(fixture_requests(fx)))


def _device_derive(engine, dr, lead=0, stream=None):
    import torch
    dev = torch.device("cuda", 0)
    n = dr.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev)  # noqa: E731
    room = (dr.arena.size + 3) // 4 * 4
    arena = np.full(room, 0xFF, np.uint8)
    arena[:dr.arena.size] = dr.arena
    d = dict(parents=up(dr.parents), reqs=up(dr.reqs), arena=up(arena),
             secrets=torch.full((32 * n,), 0xA5, dtype=torch.uint8, device=dev),
             pubs=torch.full((64 * n,), 0xA5, dtype=torch.uint8, device=dev),
             st=torch.full((n,), 0xA5, dtype=torch.uint8, device=dev),
             tries=torch.full((n,), 0xA5, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    engine.derive_keys_device(d["parents"].data_ptr(), len(dr.parents), d["reqs"].data_ptr(), n, d["arena"].data_ptr(),
                              dr.arena.size, d["secrets"].data_ptr(), d["pubs"].data_ptr(), d["st"].data_ptr(),
                              d["tries"].data_ptr(), stream=stream or 0)
    return d


def _down(d):
    import torch
    torch.cuda.synchronize()
    return (d["secrets"].cpu().numpy().reshape(-1, 32), d["pubs"].cpu().numpy().reshape(-1, 64), d["st"].cpu().numpy(),
            d["tries"].cpu().numpy())


def test_fixture_device_form(engine, fx):
    check_fixture(fx, *_down(_device_derive(engine, fixture_requests(fx))))


def test_fixture_pool_form_and_failover(fx):
    from corda_amd.engine import EnginePool
    dr = fixture_requests(fx)
    with EnginePool([0, 0]) as ep:
        check_fixture(fx, *ep.derive_keys(dr))
        assert ep.last_stats["reruns"] == 0
        ep.inject_fault(0)
        check_fixture(fx, *ep.derive_keys(dr))
        assert ep.last_stats["reruns"] == 1 and ep.last_stats["failed_slots"] == 1 and ep.healthy() == [False, True]
        ep.inject_fault(1)
        secrets, pubs, st, tries = ep.derive_keys(dr, allow_partial=True)
        assert (st == B.NOT_RUN).all() and not secrets.any() and not pubs.any() and ep.last_stats["not_run"] == dr.n
        ep.inject_fault(0, False)
        ep.inject_fault(1, False)
        check_fixture(fx, *ep.derive_keys(dr))
        # the pool form of cg_public_keys: the same bytes, and it fails over too
        secrets = [bytes.fromhex(r["secret"]) for r in fx["records"] if fx["parents"][r["parent"]]["scheme"] == R.R1][:40]
        want = [r["pub"] for r in fx["records"] if fx["parents"][r["parent"]]["scheme"] == R.R1][:40]
        ep.inject_fault(0)
        pubs, st = ep.public_keys(R.R1, secrets)
        assert not st.any() and [q.tobytes().hex() for q in pubs] == want and ep.last_stats["reruns"] == 1
        ep.inject_fault(0, False)


@pytest.mark.parametrize("bits", [24, 22])
def test_smaller_tables_derive_the_same_bytes(fx, bits):
    from corda_amd.engine import Engine
    with Engine(0, table_bytes_max=_lib.lib().cg_table_bytes(bits)) as eng:
        assert eng.info()["fixed_base_bits"] == bits
        check_fixture(fx, *eng.derive_keys(fixture_requests(fx)))


# 2 ---------------------------------------------------------------- counts
def test_4099_mixed_requests(engine, mixed4099):
    """Every request: the secret against hmac (no request rehashes: secret = mac[0..32)), the public key
    against the second GPU form (cg_public_keys over the derived secrets, its own prep kernel) and the
    device form; the sample of ~250 also against derive_ref, whose pure-Python point arithmetic takes
    milliseconds per ECDSA key."""
    import hmac
    dr, rows, want = mixed4099
    secrets, pubs, st, tries = engine.derive_keys(dr)
    check_sample(want, secrets, pubs, st, tries)
    keys = [key_data(scheme, private) for scheme, private in PARENTS7]
    for j, (p, seed) in enumerate(rows):
        assert secrets[j].tobytes() == hmac.new(keys[p], seed, hashlib.sha512).digest()[:32], j
    for scheme in (R.K1, R.R1, R.ED):
        idx = [j for j, (p, _) in enumerate(rows) if PARENTS7[p][0] == scheme]
        again, st2 = engine.public_keys(scheme, [secrets[j].tobytes() for j in idx])
        assert not st2.any() and np.array_equal(again, pubs[idx]), scheme
    for a, b in zip(_down(_device_derive(engine, dr)), (secrets, pubs, st, tries)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [63, 64, 65, RUN - 1, RUN, RUN + 1])
def test_counts_around_a_wave_and_an_inversion_run(engine, mixed4099, n):
    dr, rows, want = mixed4099
    sub = B.DeriveRequests(dr.parents, np.ascontiguousarray(dr.reqs[:n]), dr.arena)
    secrets, pubs, st, tries = engine.derive_keys(sub)
    assert len(st) == n
    check_sample(want, secrets, pubs, st, tries, limit=n)


def test_chunked_context(mixed4099):
    from corda_amd.engine import Engine
    dr, _, want = mixed4099
    n = 3 * 1024 + 1
    sub = B.DeriveRequests(dr.parents, np.ascontiguousarray(dr.reqs[:n]), dr.arena)
    with Engine(0, chunk_items=1024) as eng:
        check_sample(want, *eng.derive_keys(sub), limit=n)


# 3 ---------------------------------------------------------------- layouts
@pytest.mark.parametrize("rem", [0, 1, 2, 3])
def test_seeds_at_every_byte_phase_arena_ending_on_a_seed(engine, rem):
    """Every seed and key moved to a byte phase (mod 8 for the seeds), poison between them, the arena
    ending on a seed's last byte with arena_len % 4 == rem; the device buffer holds 0xFF to the
    rounded end and nothing behind it."""
    dr, rows = mixed(260, salt=rem + 1)
    parents, reqs = dr.parents.copy(), dr.reqs.copy()
    phases = {"seed": np.array([j % 8 if rows[j][1] else -1 for j in range(dr.n)])}
    last = max(j for j in range(dr.n) if rows[j][1])  # the field the arena ends on takes the phase rem asks for
    phases["seed"][last] = -1
    arena = LU._relayout(dr.arena, [[LU._Spec("key", parents, "key_off", parents["key_len"])],
                                    [LU._Spec("seed", reqs, "seed_off", reqs["seed_len"], mod=8)]],
                         "seed", 40 + rem, 3, 0xFF, rem, phases)
    assert arena.size % 4 == rem
    moved = B.DeriveRequests(parents, reqs, arena)
    got = _down(_device_derive(engine, moved))
    base = engine.derive_keys(dr)
    for a, b in zip(got, base):
        assert np.array_equal(a, b)
    assert not base[2].any()
    for j in range(0, dr.n, 9):
        scheme, private = PARENTS7[rows[j][0]]
        secret, pub, _ = R.derive(scheme, key_data(scheme, private), rows[j][1])
        assert base[0][j].tobytes() == secret and base[1][j].tobytes() == pub


# 4 ---------------------------------------------------------------- cg_public_keys
def crafted_d(scheme):
    n = ecdsa_bc.CURVES[scheme].n
    return [0, 1, 2, n - 1, n, n + 1, 2 ** 256 - 1, 2 ** 255, sum(1 << (4 * i) for i in range(63)),
            sum(1 << (4 * i) for i in range(64)), int.from_bytes(hashlib.sha256(b"d").digest(), "big") >> 1]


@pytest.mark.parametrize("scheme", [R.K1, R.R1])
def test_public_keys_accept_rule_and_q(engine, scheme):
    ds = crafted_d(scheme)
    pubs, st = engine.public_keys(scheme, [d.to_bytes(32, "big") for d in ds])
    want = [R.public_key(scheme, d.to_bytes(32, "big")) for d in ds]
    assert [int(s) for s in st] == [w[0] for w in want]
    assert [p.tobytes() for p in pubs] == [w[1] for w in want]
    assert [w[0] for w in want].count(R.KEY_REJECTED) >= 7 and [w[0] for w in want].count(0) >= 2


@pytest.mark.parametrize("scheme", [R.K1, R.R1, R.ED])
def test_public_keys_device_form(engine, scheme):
    """cg_public_keys_device over the crafted list (Ed25519: the same 32 bytes as seeds), on a caller
    stream, at an odd 4-byte offset of its buffers: the refused candidates keep their input bytes."""
    import torch
    dev = torch.device("cuda", 0)
    ds = [d % 2 ** 256 for d in crafted_d(R.K1 if scheme == R.ED else scheme)]
    raw = b"".join(d.to_bytes(32, "big") for d in ds)
    n = len(ds)
    d_sec = torch.from_numpy(np.frombuffer(bytes(4) + raw, np.uint8).copy()).to(dev)
    d_pub = torch.full((4 + 64 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    engine.public_keys_device(scheme, d_sec.data_ptr() + 4, n, d_pub.data_ptr() + 4, d_st.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    want = [R.public_key(scheme, d.to_bytes(32, "big")) for d in ds]
    assert [int(x) for x in d_st.cpu().numpy()] == [w[0] for w in want]
    assert d_pub.cpu().numpy()[4:].tobytes() == b"".join(w[1] for w in want)
    assert d_pub.cpu().numpy()[:4].tobytes() == b"\xa5" * 4 and d_sec.cpu().numpy()[4:].tobytes() == raw
    host = engine.public_keys(scheme, [d.to_bytes(32, "big") for d in ds])
    assert host[0].tobytes() == b"".join(w[1] for w in want) and list(host[1]) == [w[0] for w in want]


def test_public_keys_entropy_seeds(engine):
    seeds = [ed.entropy_seed(e) for e in (20, 70, 80)] + [bytes(32), bytes([255]) * 32]
    pubs, st = engine.public_keys(R.ED, seeds)
    assert not st.any()
    assert [p.tobytes() for p in pubs] == [ed.public_from_seed(s) + bytes(32) for s in seeds]
    rc = _lib.lib().cg_public_keys(engine._h, 1, None, 0, None, None)
    assert rc == -1  # RSA: no key derivation


# 5 ---------------------------------------------------------------- the retry path (test hook)
def _probe(k):
    env = dict(os.environ, CG_TEST_DERIVE_FORCE_RETRIES=str(k))
    out = subprocess.run([sys.executable, os.path.join(HERE, "derive_hook_probe.py")], env=env, check=True,
                         stdout=subprocess.PIPE, timeout=600).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


@pytest.mark.parametrize("k", [1, 2, 5])
def test_forced_retries(k):
    import derive_hook_probe as P
    got = _probe(k)
    assert len(got["items"]) == 9
    for it in got["items"]:
        scheme = it["scheme"]
        seed = next(s for s in P.SEEDS if len(s) == it["seed_len"])
        st, secret, pub, tries = R.device_expect(scheme, key_data(scheme, P.PRIVATE[scheme]), seed, k)
        assert (it["status"], it["secret"], it["pub"], it["retries"]) == (st, secret.hex(), pub.hex(), tries), it
        assert st == (R.DERIVE_HOST if k == 5 and scheme != R.ED else 0)
    # the Python mirror finishes a DERIVE_HOST item on the host: the key the JVM returns, hook or not
    secret, pub, _ = R.derive(R.R1, key_data(R.R1, P.PRIVATE[R.R1]), b"seed-1", k if k <= R.MAX_RETRIES else 0)
    assert (got["mirror"]["secret"], got["mirror"]["pub"]) == (secret.hex(), pub.hex())


# 6 ---------------------------------------------------------------- closing the loop
def test_ed25519_children_sign_and_verify(engine):
    from corda_amd import signable
    parent = ed.entropy_seed(70)
    b = B.DeriveRequestBuilder()
    p = b.parent(R.ED, parent)
    for j in range(5):
        b.add_request(p, b"tx-%d" % j)
    secrets, pubs, st, _ = engine.derive_keys(b.build())
    assert not st.any()
    seeds = [s.tobytes() for s in secrets]
    loaded = engine.load_signers(seeds)
    assert loaded == [q.tobytes()[:32] for q in pubs]
    pre, suf = signable.template(1, 4)
    ids = [hashlib.sha256(bytes([k])).digest() for k in range(5)]
    sb = B.SignRequestBuilder()
    for k, i in enumerate(ids):
        sb.add_request(k, sb.tx_id(i), sb.template(pre, suf))
    sigs, sst = engine.sign_tx_ids(sb.build())
    engine.clear_signers()
    assert not sst.any()
    tb = B.TxSigBuilder()
    for k, i in enumerate(ids):
        key = tb.key(B.EDDSA_ED25519_SHA512, B.KEY_RAW, loaded[k])
        tb.add_signature(key, tb.tx_id(i), tb.template(pre, suf), sigs[k].tobytes())
    assert np.array_equal(engine.verify_tx_signatures_packed(tb.build().packed()), np.zeros(5, np.uint8))


@pytest.mark.parametrize("scheme", [R.K1, R.R1])
def test_ecdsa_child_verifies_a_signature(engine, scheme):
    b = B.DeriveRequestBuilder()
    b.add_request(b.parent(scheme, hashlib.sha256(b"ec parent").digest()), b"seed-1")
    secrets, pubs, st, _ = engine.derive_keys(b.build())
    assert not st.any()
    d = int.from_bytes(secrets[0].tobytes(), "big")
    msg = b"a message the child key signs"
    sig = ecdsa_bc.der_encode_sig(*ecdsa_bc.sign(scheme, d, msg, 0x1234567 + scheme))
    vb = B.BatchBuilder()
    vb.add_with_key(scheme, B.KEY_RAW, pubs[0].tobytes(), sig, msg)
    vb.add_with_key(scheme, B.KEY_RAW, pubs[0].tobytes(), sig, msg + b"!")
    assert list(engine.verify(vb.build(), B.MODE_DOVERIFY)) == [B.VALID, B.INVALID]


# 7 ---------------------------------------------------------------- two caller streams
def test_derive_between_two_verifies_on_two_streams(engine, mixed4099):
    import torch

    import golden_io
    dev = torch.device("cuda", 0)
    vb, exp, _ = golden_io.sig_batch(golden_io.load("ed25519.json")[:256])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev)  # noqa: E731
    arena = np.zeros((vb.arena.size + 3) // 4 * 4 + 16, np.uint8)
    arena[:vb.arena.size] = vb.arena
    v = dict(keys=up(vb.keys), items=up(vb.items), arena=up(arena))
    vst = [torch.full((vb.n,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    dr, _, want = mixed4099
    torch.cuda.synchronize()

    def verify_on(k):
        engine.verify_device(v["keys"].data_ptr(), len(vb.keys), v["items"].data_ptr(), vb.n, v["arena"].data_ptr(),
                             vb.arena.size, vst[k].data_ptr(), B.MODE_DOVERIFY, stream=streams[k].cuda_stream)
    verify_on(0)
    d = _device_derive(engine, dr, stream=streams[1].cuda_stream)
    verify_on(1)
    check_sample(want, *_down(d))
    for k in range(2):
        assert np.array_equal(vst[k].cpu().numpy(), exp), f"verify call {k}"


# 8 ---------------------------------------------------------------- bad inputs beside good ones
def test_bad_inputs_beside_good_items(engine):
    b = B.DeriveRequestBuilder()
    good = [b.parent(s, p) for s, p in PARENTS7[:3]]
    empty = b.parent_key_data(R.R1, b"")                 # SecretKeySpec throws
    long = b.parent_key_data(R.ED, bytes(129))           # would need a pre-hash
    edge = b.parent_key_data(R.K1, bytes(range(128)))    # 128 bytes: the longest legal key
    rsa = b.parent_key_data(1, bytes(32))
    sphincs = b.parent_key_data(5, bytes(32))
    plan = [(good[0], b"a"), (empty, b"a"), (good[1], b""), (long, b"a"), (edge, b"a"), (rsa, b"a"), (good[2], b"abc"),
            (sphincs, b"a"), (good[0], b"tail"), (good[1], b"x"), (good[2], b"y"), (good[0], b"z")]
    for p, s in plan:
        b.add_request(p, s)
    dr = b.build()
    dr.reqs["parent"][9] = len(dr.parents)            # parent index out of range
    dr.reqs["seed_off"][10] = dr.arena.size - 1       # seed runs past the arena
    dr.reqs["seed_len"][10] = 2
    dr.reqs["seed_off"][11] = 2 ** 63                 # offset far outside
    secrets, pubs, st, tries = engine.derive_keys(dr)
    assert list(st) == [0, B.DERIVE_BAD_PARENT, 0, B.DERIVE_BAD_PARENT, 0, B.UNSUPPORTED, 0, B.UNSUPPORTED, 0,
                        B.NOT_RUN, B.NOT_RUN, B.NOT_RUN]
    for j, (p, s) in enumerate(plan):
        if st[j]:
            assert not secrets[j].any() and not pubs[j].any() and tries[j] == 0
    for j in (0, 2, 6, 8):
        scheme, private = PARENTS7[plan[j][0]]
        assert (secrets[j].tobytes(), pubs[j].tobytes()) == R.derive(scheme, key_data(scheme, private), plan[j][1])[:2]
    assert (secrets[4].tobytes(), pubs[4].tobytes()) == R.derive(R.K1, bytes(range(128)), b"a")[:2]
    # a parent whose key bytes lie outside the arena: its requests are NOT_RUN, the others derive
    dr.parents["key_off"][good[1]] = dr.arena.size
    st2 = engine.derive_keys(dr)[2]
    assert st2[2] == B.NOT_RUN and st2[0] == 0 and st2[6] == 0
    # n == 0 is a no-op, a NULL ctx an argument error
    L = _lib.lib()
    assert L.cg_derive_keys(engine._h, None, 0, None, 0, None, 0, None, None, None, None) == 0
    assert L.cg_derive_keys(None, None, 0, None, 0, None, 0, None, None, None, None) == -1


def test_crypto_mirror(engine):
    from corda_amd.crypto import Crypto, PrivateKey, UnsupportedOperationException
    Crypto.use_engine(engine)
    for scheme, private in PARENTS7[:3]:
        kps = Crypto.derive_key_pairs(PrivateKey(scheme, private), [b"seed-1", b"seed-2"])
        for kp, seed in zip(kps, (b"seed-1", b"seed-2")):
            secret, pub, _ = R.derive(scheme, key_data(scheme, private), seed)
            assert kp.private.encoded == secret and kp.public.encoded == (pub[:32] if scheme == R.ED else pub)
        assert kps[0].public != kps[1].public
        kp = Crypto.generate_key_pair(scheme)
        assert R.public_key(scheme, kp.private.encoded) == (0, kp.public.encoded + (bytes(32) if scheme == R.ED else b""))
    kp = Crypto.derive_key_pair_from_entropy(20)
    assert kp.private.encoded == ed.entropy_seed(20) and kp.public.encoded == ed.public_from_seed(ed.entropy_seed(20))
    with pytest.raises(UnsupportedOperationException):
        Crypto.derive_key_pair(PrivateKey(1, bytes(32)), b"seed-1")
