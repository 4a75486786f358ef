"""The packing key on the device (rs_pack_keygen_dev, rs_pack_expand_dev, rs_audit_pack_key_dev): whole
small keys against numpy word for word under the directed ring secrets of tests/test_pack_key_cpu.py, every invalid argument, the
default-128 key at its full size used for packing, and the first real packing key of a large ring (redsec_medium, 15,360 rows)."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import client, keygen
from test_pack_key_cpu import RING_SET, SECRETS, SHAPES, STDEV, lwe_secret, pack_gauss, ring_secret

pytestmark = pytest.mark.gpu

MASK_SEED = bytes(range(150, 182))
NOISE_SEED = bytes(range(31, 63))
KEY_SEED = bytes(range(9, 41))
GUARD = 0x5A5A5A5A

_BACKENDS = {}


def _backend(N, n):
    """One context per (ring, n) for the whole module: the calls need no key, only the context's N and n."""
    import redsec_amd
    if (N, n) not in _BACKENDS:
        _BACKENDS[N, n] = redsec_amd.Backend(redsec_amd.params(RING_SET[N], n=n), device=0)
    return _BACKENDS[N, n]


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    import torch
    for be in _BACKENDS.values():
        be.close()
    _BACKENDS.clear()
    torch.cuda.empty_cache()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _guarded(be, *shape):
    """A tensor of `shape` between two guard rows of its own row size -> (whole, view)."""
    rows, row = shape[0], int(np.prod(shape[1:]))
    whole = be.empty(rows + 2, row).fill_(GUARD)
    return whole, whole[1:rows + 1].view(*shape)


def _guards_ok(whole):
    return bool((whole[0] == GUARD).all()) and bool((whole[-1] == GUARD).all())


@pytest.mark.parametrize("kind", SECRETS)
@pytest.mark.parametrize("N,n,basebit,t", SHAPES)
def test_whole_small_keys_equal_numpy(N, n, basebit, t, kind):
    import torch
    be, name = _backend(N, n), RING_SET[N]
    lwe, S = lwe_secret(n), ring_secret(kind, N)
    rows = np.arange(n * t)
    mask = keygen.pack_key_mask(MASK_SEED, N, rows).reshape(n, t, N)
    g_body, body = _guarded(be, n, t, N)
    g_full, full = _guarded(be, n, t, 2, N)
    for stdev in (0.0, STDEV):
        want = keygen.pack_key(name, lwe, S, MASK_SEED, NOISE_SEED, basebit, t, stdev)
        noise = pack_gauss(NOISE_SEED, rows, N, stdev).reshape(n, t, N)
        limit = keygen.pack_noise_limit(stdev) if stdev else 0
        for again in range(2):                                               # a second call into the same buffers: the same words
            got = be.pack_keygen(lwe, S, MASK_SEED, NOISE_SEED, basebit, t, stdev, out=body)
            assert got.data_ptr() == body.data_ptr()
            h = body.cpu().numpy()
            assert np.array_equal(h, want), (stdev, again, np.argwhere(h != want)[:4].tolist())
            exp = be.expand_packing_key(MASK_SEED, body, t, out=full)
            assert exp.data_ptr() == full.data_ptr()
            h = full.cpu().numpy()
            assert np.array_equal(h[:, :, 0], mask) and np.array_equal(h[:, :, 1], want), (stdev, again)
        assert _guards_ok(g_body) and _guards_ok(g_full)
        for rep in (be.audit_packing_key(lwe, S, full, basebit, t, limit=limit, noise=True),
                    be.audit_packing_key(lwe, S, body, basebit, t, mask_seed=MASK_SEED, limit=limit, noise=True)):
            assert np.array_equal(rep["noise"].cpu().numpy(), noise)
            assert (rep["over"], rep["words"], rep["max_abs"]) == (0, n * t * N, int(np.abs(noise.astype(np.int64)).max()))
        if stdev:                                                             # a limit below the largest word counts what exceeds it
            low = int(np.abs(noise.astype(np.int64)).max()) // 2
            rep = be.audit_packing_key(lwe, S, body, basebit, t, mask_seed=MASK_SEED, limit=low)
            assert rep["over"] == int((np.abs(noise.astype(np.int64)) > low).sum()) > 0 and "noise" not in rep
    if (N, n, basebit, t) == SHAPES[0] and kind == "random":
        # expansion on a side stream with a dependent consumer; the words of the bodies as a server gets them
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        fresh = be.empty(n, t, 2, N).fill_(GUARD)
        with torch.cuda.stream(s):
            out = be.expand_packing_key(MASK_SEED, body, t, out=fresh)
            twice = out * 2
        s.synchronize()
        assert np.array_equal(twice.cpu().numpy().view(np.uint32), full.cpu().numpy().view(np.uint32) * np.uint32(2))
        key = client.PackingKey(name, n, basebit, t, MASK_SEED, body.cpu().numpy())
        assert np.array_equal(be.upload_packing_key(key).cpu().numpy(), key.expand())


def test_invalid_arguments_leave_the_next_call_working():
    import redsec_amd
    import torch
    N, n, basebit, t = 1024, 2, 4, 5
    be = _backend(N, n)
    L, vp = be.L, C.c_void_p
    lwe, S = lwe_secret(n), ring_secret("random", N)
    want = keygen.pack_key(RING_SET[N], lwe, S, MASK_SEED, NOISE_SEED, basebit, t, STDEV)
    body, full, noise = be.empty(n, t, N), be.empty(n, t, 2, N), be.empty(n, t, N)
    i32p = C.POINTER(C.c_int32)
    P = lambda x: vp(x.data_ptr())
    H = lambda a: a.ctypes.data_as(i32p)
    bad_lwe, bad_S = lwe.copy(), S.copy()
    bad_lwe[1], bad_S[N - 1] = 2, -1
    rep = redsec_amd.backend.RsPackKeyAudit()

    def gen(o=P(body), k=H(lwe), K=H(S), ms=MASK_SEED, ns=NOISE_SEED, basebit=basebit, t=t, stdev=STDEV):
        return L.rs_pack_keygen_dev(be.h, o, k, K, ms, ns, basebit, t, stdev)

    def expand(o=P(full), ms=MASK_SEED, b=P(body), t=t):
        return L.rs_pack_expand_dev(be.h, o, ms, b, t, None)

    def audit(r=C.byref(rep), e=P(noise), key=P(body), ms=MASK_SEED, k=H(lwe), K=H(S), basebit=basebit, t=t, limit=keygen.pack_noise_limit(STDEV)):
        return L.rs_audit_pack_key_dev(be.h, r, e, key, ms, k, K, basebit, t, limit)

    def still_works():
        body.zero_(); full.zero_(); noise.zero_()
        assert gen() == 0 and expand() == 0 and audit() == 0
        torch.cuda.synchronize()
        assert np.array_equal(body.cpu().numpy(), want) and np.array_equal(full.cpu().numpy()[:, :, 1], want)
        assert (rep.over, rep.words) == (0, n * t * N) and rep.max_abs == int(np.abs(noise.cpu().numpy().astype(np.int64)).max()) > 0

    still_works()
    cases = [
        (lambda: gen(o=None), b"null pointer"), (lambda: gen(k=None), b"null pointer"), (lambda: gen(K=None), b"null pointer"),
        (lambda: gen(ms=None), b"null pointer"), (lambda: gen(ns=None), b"null pointer"),
        (lambda: gen(k=H(bad_lwe)), b"lwe_key[1] = 2"), (lambda: gen(K=H(bad_S)), b"tlwe_key[1023] = -1"),
        (lambda: gen(ns=MASK_SEED), b"equal"),
        (lambda: gen(basebit=0, t=1), b"outside 1 .. 8"), (lambda: gen(basebit=9, t=1), b"outside 1 .. 8"), (lambda: gen(basebit=-1, t=1), b"outside 1 .. 8"),
        (lambda: gen(t=0), b"below 1"), (lambda: gen(t=-3), b"below 1"),
        (lambda: gen(basebit=8, t=5), b"passes 32 bits"), (lambda: gen(basebit=1, t=33), b"passes 32 bits"), (lambda: gen(basebit=3, t=11), b"passes 32 bits"),
        (lambda: gen(stdev=-1e-9), b"finite and non-negative"), (lambda: gen(stdev=float("nan")), b"finite and non-negative"),
        (lambda: gen(stdev=float("inf")), b"finite and non-negative"),
        (lambda: expand(o=None), b"null pointer"), (lambda: expand(ms=None), b"null pointer"), (lambda: expand(b=None), b"null pointer"),
        (lambda: expand(t=0), b"below 1"), (lambda: expand(t=-1), b"below 1"), (lambda: expand(t=(1 << 31) - 1), b"too large"),
        (lambda: expand(t=1 << 25), b"too large"),
        (lambda: audit(r=None), b"null pointer"), (lambda: audit(key=None), b"null pointer"), (lambda: audit(k=None), b"null pointer"),
        (lambda: audit(K=None), b"null pointer"), (lambda: audit(k=H(bad_lwe)), b"lwe_key[1] = 2"), (lambda: audit(K=H(bad_S)), b"tlwe_key[1023] = -1"),
        (lambda: audit(basebit=0, t=1), b"outside 1 .. 8"), (lambda: audit(t=0), b"below 1"), (lambda: audit(basebit=8, t=5), b"passes 32 bits"),
    ]
    for k, (call, text) in enumerate(cases):
        assert call() == -1 and text in L.rs_last_error(), (k, L.rs_last_error())
        still_works()
    # the Python layer: a secret or a key of another set or another n is refused
    sk = client.SecretKeySet.from_secret("default128", *keygen.secret_keys("default128", KEY_SEED, n))
    with pytest.raises(ValueError, match="default128"):
        sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED, backend=be)
    sk = client.SecretKeySet.from_secret("redsec_small_v2", *keygen.secret_keys("redsec_small_v2", KEY_SEED, n + 1))
    with pytest.raises(ValueError, match="n = 3"):
        sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED, backend=be)
    sk = client.SecretKeySet.from_secret("redsec_small_v2", lwe, S)
    with pytest.raises(ValueError, match="equal"):
        sk.packing_key(mask_seed=MASK_SEED, noise_seed=MASK_SEED, backend=be)
    with pytest.raises(ValueError):
        sk.packing_key(4, 9, MASK_SEED, NOISE_SEED, backend=be)
    key = sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED, backend=be)      # the set's default deviation and digits
    assert np.array_equal(key.body, sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED).body) and (key.basebit, key.t) == (4, 5)
    rep2 = sk.audit_packing_key(key, be)
    assert (rep2["over"], rep2["words"]) == (0, n * 5 * N) and 0 < rep2["max_abs"] <= keygen.pack_noise_limit(keygen.rlwe_default_stdev("redsec_small_v2"))


def test_default128_at_full_size_generated_expanded_used_and_audited():
    """n = 630, (4, 4): 2,520 rows. The device's bodies equal keygen.pack_key and SecretKeySet.packing_key(backend=) gives the same
    PackingKey; expanded on the device, the key packs 1,025 NAND results of a device-generated evaluation key and every bit decrypts;
    the audit passes, and counts exactly the one body word corrupted on the device."""
    import redsec_amd
    import torch
    be = redsec_amd.Backend(redsec_amd.params("default128"), device=0)
    try:
        sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
        del bk, ksk
        host = sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
        assert (host.basebit, host.t, host.body.shape) == (4, 4, (630, 4, 1024))
        stdev = keygen.rlwe_default_stdev("default128")
        body = be.pack_keygen(sk.lwe_key, sk.tlwe_key, MASK_SEED, NOISE_SEED, 4, 4, stdev)
        h = body.cpu().numpy()
        assert np.array_equal(h, host.body), np.argwhere(h != host.body)[:4].tolist()
        dev = sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED, backend=be)
        assert (dev.name, dev.n, dev.basebit, dev.t, dev.mask_seed) == (host.name, host.n, host.basebit, host.t, host.mask_seed)
        assert np.array_equal(dev.body, host.body) and dev.body.dtype == np.int32
        d_key = be.expand_packing_key(MASK_SEED, body, 4)
        rng = np.random.default_rng(23)
        count = 1025
        x, y = rng.integers(0, 2, count), rng.integers(0, 2, count)
        ct = _dev(sk.encrypt_bits(np.concatenate([x, y]), seed=6))
        nand = be.gate("NAND", ct[:count].contiguous(), ct[count:].contiguous())
        packed = be.pack(nand, d_key, 4, 4)
        assert tuple(packed.shape) == (2, 2, 1024)
        assert np.array_equal(sk.decrypt_packed_bits(packed, count, backend=be), 1 - (x & y))
        assert np.array_equal(be.pack(nand, dev).cpu().numpy(), packed.cpu().numpy())          # the PackingKey: uploaded and expanded by the call
        rep = sk.audit_packing_key(dev, be)
        assert (rep["over"], rep["words"]) == (0, 2520 * 1024) and 0 < rep["max_abs"] <= keygen.pack_noise_limit(stdev)
        rep = be.audit_packing_key(sk.lwe_key, sk.tlwe_key, d_key, 4, 4)
        assert (rep["over"], rep["words"]) == (0, 2520 * 1024)
        body[317, 2, 600] += 1 << 20
        for k, seed in ((body, MASK_SEED), (be.expand_packing_key(MASK_SEED, body, 4), None)):
            rep = be.audit_packing_key(sk.lwe_key, sk.tlwe_key, k, 4, 4, mask_seed=seed)
            assert rep["over"] == 1 and (1 << 20) - keygen.pack_noise_limit(stdev) <= rep["max_abs"] <= (1 << 20) + keygen.pack_noise_limit(stdev)
    finally:
        be.close()
        torch.cuda.empty_cache()


def test_redsec_medium_at_full_size_the_first_real_key_of_a_large_ring():
    """n = 3072, N = 4096, (4, 5): 15,360 rows, stdev 2^-30 (the set's own truncates to zero). 16 sampled rows, rows 0 and 15,359 among
    them, equal keygen.pack_key; the seeded audit passes over all 62.9 M words and returns the domain-15 words; the expanded masks
    are pack_key_mask's; 64 fresh +-1/8 bits pack and decrypt on the device."""
    import redsec_amd
    import torch
    name, stdev, (basebit, t) = "redsec_medium", 2.0 ** -30, keygen.pack_default("redsec_medium")
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    try:
        n, N = be.p.n, be.p.N
        assert (n, N, basebit, t) == (3072, 4096, 4, 5)
        sk = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, KEY_SEED))
        rows = np.unique(np.concatenate([[0, 1, t - 1, t, n * t - 1], np.random.default_rng(5).integers(0, n * t, 11)]))[:16]
        assert len(rows) == 16 and rows[0] == 0 and rows[-1] == n * t - 1 == 15359
        want = keygen.pack_key(name, sk.lwe_key, sk.tlwe_key, MASK_SEED, NOISE_SEED, basebit, t, stdev, rows=rows)
        body = be.pack_keygen(sk.lwe_key, sk.tlwe_key, MASK_SEED, NOISE_SEED, basebit, t, stdev)
        d_rows = torch.from_numpy(rows).cuda()
        h = body.view(n * t, N)[d_rows].cpu().numpy()
        assert np.array_equal(h, want), np.argwhere(h != want)[:4].tolist()
        limit = keygen.pack_noise_limit(stdev)
        rep = be.audit_packing_key(sk.lwe_key, sk.tlwe_key, body, basebit, t, mask_seed=MASK_SEED, limit=limit, noise=True)
        assert (rep["over"], rep["words"]) == (0, 15360 * 4096) and 0 < rep["max_abs"] <= limit
        assert np.array_equal(rep["noise"].view(n * t, N)[d_rows].cpu().numpy(), pack_gauss(NOISE_SEED, rows, N, stdev))
        del rep
        d_key = be.expand_packing_key(MASK_SEED, body, t)
        got = d_key.view(n * t, 2, N)[d_rows].cpu().numpy()
        assert np.array_equal(got[:, 0], keygen.pack_key_mask(MASK_SEED, N, rows)) and np.array_equal(got[:, 1], want)
        bits = np.random.default_rng(24).integers(0, 2, 64)
        packed = be.pack(_dev(sk.encrypt_bits(bits, seed=7)), d_key, basebit, t)
        assert tuple(packed.shape) == (1, 2, N)
        assert np.array_equal(sk.decrypt_packed_bits(packed, 64, backend=be), bits)
    finally:
        be.close()
        torch.cuda.empty_cache()
