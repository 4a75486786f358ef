"""Ring re-keying on the device (rs_ring_rekey_dev): word-for-word equality with the numpy restatement on
every ring, ciphertext count and digit shape at which the kernels take another path, guard words, invalid arguments, and the end to
end uses: packed NAND results of a default-128 secret ring-re-keyed to a second secret under both key forms, and the packed logits
of an MNIST image on redsec_small_v2 delivered under a second secret's ring key."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

MASK_SEED = bytes(range(150, 182))
NOISE_SEED = bytes(range(31, 63))
RAND_SEED = bytes(range(200, 232))
PACK_MASK_SEED = bytes(range(60, 92))
PACK_NOISE_SEED = bytes(range(120, 152))
KEY_SEED = bytes(range(9, 41))
OTHER_SEED = bytes(range(90, 122))
GUARD = 0x5A5A5A5A
RING_SETS = {1024: "redsec_small_v2", 2048: None, 4096: "redsec_medium", 8192: "redsec_large"}

_BACKENDS = {}


def _backend(N):
    """One small-n context per ring: the call needs no loaded key, and the ring is the context's."""
    import redsec_amd
    if N not in _BACKENDS:
        p = redsec_amd.params(RING_SETS[N] or "default128", n=16)
        # N = 2048 is a ring no shipped set has: rs_create takes any N in {1024, 2048, 4096, 8192} with k = 1 whatever the gadget
        # and keyswitch shape beside it (tests/oracle_lib.py builds its N = 2048 context the same way), and rs_ring_rekey_dev reads
        # nothing of a context but its N. For the other rings the line changes nothing
        p.N = N
        _BACKENDS[N] = redsec_amd.Backend(p, device=0)
        assert _BACKENDS[N].p.N == N
    return _BACKENDS[N]


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


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _extreme(rng, R, N, basebit, t):
    """Random ciphertexts whose first and last mask coefficients are the extreme words and 2^32 - off, which wraps abar to 0."""
    rl = _words(rng, R, 2, N)
    off = 1 << (31 - t * basebit)
    ext = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, (1 << 32) - off, (1 << 32) - off - 1, off], np.uint64).astype(np.uint32)
    rl[:, 0, :ext.size] = ext.view(np.int32)
    rl[0, 0, -ext.size:] = ext.view(np.int32)
    return rl


def _check_ring_rekey(N, R, basebit, t, side_stream=False):
    """Random words for the key (equality of the sums needs no real key); a ciphertext of guard words on either side of the output."""
    import torch
    be = _backend(N)
    rng = np.random.default_rng(N + 7 * R + 100 * basebit + t)
    rl, key = _extreme(rng, R, N, basebit, t), _words(rng, t + 1, 2, N)
    want = keygen.ring_rekey(rl, key, basebit, t)
    guard = be.empty(R + 2, 2, N).fill_(GUARD)
    out = guard[1:R + 1]
    d_rl, d_key = _dev(rl), _dev(key)
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                           # a non-default stream, the consumer ordered behind it
            got = be.ring_rekey(d_rl, d_key, basebit, t, out=out)
            twice = got * 2
        s.synchronize()
        assert np.array_equal(_u32(twice.cpu().numpy()), _u32(want) * np.uint32(2))
    else:
        got = be.ring_rekey(d_rl, d_key, basebit, t, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (R, 2, N)
    h = got.cpu().numpy()
    assert np.array_equal(h, want), (N, R, basebit, t, np.argwhere(h != want)[:4].tolist())
    be.ring_rekey(d_rl, d_key, basebit, t, out=out)                          # a second call initialises again: the same words
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((guard[0] == GUARD).all()) and bool((guard[R + 1] == GUARD).all())
    assert np.array_equal(d_rl.cpu().numpy(), rl) and np.array_equal(d_key.cpu().numpy(), key)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_ring_rekey_words_equal_numpy_at_n_1024(R):
    """(4, 5): 20 workgroups a ciphertext; R = 3 also on a side stream with a dependent consumer."""
    _check_ring_rekey(1024, R, 4, 5)
    if R == 3:
        _check_ring_rekey(1024, R, 4, 5, side_stream=True)


def test_ring_rekey_words_equal_numpy_with_two_source_blocks():
    """N = 2048: the first ring whose source coefficients fall into two blocks and whose windows start inside (-p, p)."""
    _check_ring_rekey(2048, 1, 2, 8)


def test_ring_rekey_words_equal_numpy_on_the_large_ring():
    """N = 8192 with one digit of eight bits: 16 tiles x 2 polynomials x 8 source blocks."""
    _check_ring_rekey(8192, 1, 8, 1)


def test_ring_rekey_words_equal_numpy_at_n_4096():
    """redsec_medium's ring at its default (4, 6): 8 tiles x 2 polynomials x 4 source blocks x 6 digits."""
    _check_ring_rekey(4096, 1, 4, 6)


@pytest.mark.parametrize("basebit,t", [(1, 1), (8, 3), (4, 5), (2, 8), (5, 6), (1, 31)])
def test_ring_rekey_words_equal_numpy_for_every_digit_shape(basebit, t):
    _check_ring_rekey(1024, 2, basebit, t)


def test_ring_rekey_invalid_arguments_and_the_empty_batch():
    import torch
    N, R = 1024, 2
    be = _backend(N)
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    key, rl = _dev(_words(rng, 6, 2, N)), _dev(_words(rng, R, 2, N))
    out = be.empty(R, 2, N).fill_(7)
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())

    def call(o=P(out), c=P(rl), r=R, k=P(key), basebit=4, t=5):
        return L.rs_ring_rekey_dev(be.h, o, c, r, k, basebit, t, None)
    assert call(o=None) == -1 and call(c=None) == -1 and call(k=None) == -1 and b"null pointer" in L.rs_last_error()
    for bad in (0, 9, -1):
        assert call(basebit=bad, t=1) == -1 and b"outside 1 .. 8" in L.rs_last_error()
    for bad in (0, -3):
        assert call(t=bad) == -1 and b"below 1" in L.rs_last_error()
    for basebit, t in ((4, 9), (8, 5), (1, 33)):
        assert call(basebit=basebit, t=t) == -1 and b"passes 32 bits" in L.rs_last_error()
    for basebit, t in ((4, 8), (8, 4), (1, 32), (2, 16)):
        assert call(basebit=basebit, t=t) == -1 and b"passes 31 bits" in L.rs_last_error()
    assert call(r=1 << 62) == -1 and b"too large" in L.rs_last_error()
    assert call(r=(1 << 64) - 1) == -1 and b"too large" in L.rs_last_error()
    assert call(r=1 << 40) == -1 and b"too large for one launch" in L.rs_last_error()    # fits the address space, not one launch
    # an out that shares a byte with an input is refused: the kernels add into it with atomics after an init kernel has set it, so
    # there is no re-keying in place. Every range named below lies inside one allocation of four ciphertexts or inside the key (six)
    arena = _dev(_words(rng, 4, 2, N))
    held, held_key = arena.cpu().numpy(), key.cpu().numpy()
    A, K, ct = arena.data_ptr(), key.data_ptr(), 8 * N
    for o in (A, A + ct, A + 2 * ct - 4):                                     # out == rlwe, one ciphertext into it, on its last word
        assert call(o=vp(o), c=vp(A)) == -1 and b"out overlaps rlwe" in L.rs_last_error()
    assert call(o=vp(A), c=vp(A + 2 * ct - 4)) == -1 and b"out overlaps rlwe" in L.rs_last_error()    # out's last word is rlwe's first
    for o in (K, K + ct, K + 4 * ct):                                         # out on the key's first and second row and its last two
        assert call(o=vp(o)) == -1 and b"out overlaps ring_key" in L.rs_last_error()
    with pytest.raises(ValueError, match="out overlaps rlwe"):
        be.ring_rekey(arena[:2], key, 4, 5, out=arena[:2])
    with pytest.raises(ValueError, match="out overlaps rlwe"):
        be.ring_rekey(arena[:2], key, 4, 5, out=arena[1:3])
    with pytest.raises(ValueError, match="out overlaps ring_key"):
        be.ring_rekey(rl, key, 4, 5, out=key[4:])
    # nothing above launched anything; R = 0 is a no-op
    assert call(r=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert np.array_equal(arena.cpu().numpy(), held) and np.array_equal(key.cpu().numpy(), held_key)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), keygen.ring_rekey(rl.cpu().numpy(), key.cpu().numpy(), 4, 5))
    with pytest.raises(ValueError, match="explicit basebit"):
        be.ring_rekey(rl, key)
    with pytest.raises(ValueError):
        be.ring_rekey(rl, key, 4, 8)
    other = client.SecretKeySet.from_secret("redsec_medium", *keygen.secret_keys("redsec_medium", KEY_SEED))
    big = other.ring_rekey_to(other, 4, 2, MASK_SEED, NOISE_SEED, stdev=2.0 ** -31)
    with pytest.raises(ValueError, match="N = 4096"):
        be.ring_rekey(rl, big)


@pytest.fixture(scope="module")
def default128():
    import redsec_amd
    import torch
    be = redsec_amd.Backend(redsec_amd.params("default128"), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    yield be, sk
    be.close()
    torch.cuda.empty_cache()


def test_default128_packed_nand_results_ring_rekeyed_under_both_key_forms(default128):
    """1,024 NAND results packed under the owner's packing key, ring-re-keyed with (a) a seeded key to a second secret and (b) a key
    made from the second secret's RLWE public key alone, decrypted by the second secret on the device: every bit, and
    every phase within 8 ring_rekey_sigma of the packed phase under the owner's key."""
    be, sk = default128
    other = client.SecretKeySet.from_secret("default128", *keygen.secret_keys("default128", OTHER_SEED))
    assert not np.array_equal(sk.tlwe_key, other.tlwe_key)
    pack_key = sk.packing_key(mask_seed=PACK_MASK_SEED, noise_seed=PACK_NOISE_SEED, backend=be)
    rng = np.random.default_rng(31)
    x, y = rng.integers(0, 2, 1024), rng.integers(0, 2, 1024)
    ct = _dev(sk.encrypt_bits(np.concatenate([x, y]), seed=3))
    nand = be.gate("NAND", ct[:1024].contiguous(), ct[1024:].contiguous())
    want = 1 - (x & y)
    packed = be.pack(nand, pack_key)
    assert tuple(packed.shape) == (1, 2, 1024) and np.array_equal(sk.decrypt_packed_bits(packed, 1024, backend=be), want)
    before = sk.packed_phase(packed, 1024, backend=be)
    stdev = client.PARAM_SETS["default128"][8]
    seeded = sk.ring_rekey_to(other, mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    rlwe = sk.ring_rekey_for(other.rlwe_public_key(MASK_SEED, NOISE_SEED), rand_seed=RAND_SEED, backend=be)
    host = sk.ring_rekey_for(other.rlwe_public_key(MASK_SEED, NOISE_SEED), rand_seed=RAND_SEED)
    assert np.abs(host.rlwe.astype(np.int64) - rlwe.rlwe.astype(np.int64)).max() <= 1   # numpy's log / cos: the last bit of a noise word
    for key, sigma_row in ((seeded, stdev), (rlwe, stdev * np.sqrt(1025.0))):
        assert (key.basebit, key.t) == (2, 8) and key.expand().shape == (9, 2, 1024)
        out = be.ring_rekey(packed, key)
        assert np.array_equal(out.cpu().numpy(), keygen.ring_rekey(packed.cpu().numpy(), key.expand(), 2, 8))
        assert np.array_equal(other.decrypt_packed_bits(out, 1024, backend=be), want), key.form
        after = other.packed_phase(out, 1024, backend=be)
        assert np.array_equal(after, other.packed_phase(out.cpu().numpy(), 1024))
        sigma = keygen.ring_rekey_sigma(1024, 2, 8, sigma_row)
        err = (_u32(after) - _u32(before)).view(np.int32) / 2.0 ** 32
        print("default-128 %s key: largest ring re-keying error %.3g = %.2f sigma (ring_rekey_sigma %.3g), rms %.3g"
              % (key.form, np.abs(err).max(), np.abs(err).max() / sigma, sigma, np.sqrt(np.mean(err * err))))
        assert np.abs(err).max() < 8 * sigma < 1 / 8
        assert (sk.decrypt_packed_bits(out, 1024, backend=be) != want).any()   # the owner's key no longer opens them


def test_mnist_logits_packed_ring_rekeyed_and_decrypted_on_redsec_small_v2():
    """The ten logits of one golden image on redsec_small_v2, packed, ring-re-keyed to a second secret and decrypted there on the
    device: the integers of the direct decryption, for both key forms (their documented margins are 19.5 and 16.5 sigma),
    and every phase within 8 ring_rekey_sigma of the packed phase under the owner's key."""
    import plain_model as pm
    import redsec_amd
    import torch
    from redsec_amd import nets
    name = "redsec_small_v2"
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    other = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, OTHER_SEED))
    labels, pixels = pm.load_images()
    logits = nets.EncryptedMnist(be, pm.load_net("sign1024x1")).run(_dev(sk.encrypt_image(np.asarray(pixels[0]).ravel())))
    direct = sk.decrypt_ints(logits.cpu().numpy())
    packed = be.pack(logits.contiguous(), sk.packing_key(mask_seed=PACK_MASK_SEED, noise_seed=PACK_NOISE_SEED))
    before = sk.packed_phase(packed, 10, backend=be)
    stdev = client.PARAM_SETS[name][8]
    keys = [(sk.ring_rekey_to(other, mask_seed=MASK_SEED, noise_seed=NOISE_SEED), (4, 5), stdev),
            (sk.ring_rekey_for(other.rlwe_public_key(MASK_SEED, NOISE_SEED), rand_seed=RAND_SEED, backend=be), (2, 12), stdev * np.sqrt(1025.0))]
    for key, shape, sigma_row in keys:
        assert (key.basebit, key.t) == shape == keygen.ring_rekey_default(name, key.form)
        sigma = keygen.ring_rekey_sigma(1024, key.basebit, key.t, sigma_row)
        assert 8 * sigma <= 1 / 8192                                         # the documented margin of this form
        out = be.ring_rekey(packed, key)
        after = other.packed_phase(out, 10, backend=be)
        err = (_u32(after) - _u32(before)).view(np.int32) / 2.0 ** 32
        print("redsec_small_v2 %s key: largest ring re-keying error %.3g = %.2f sigma (ring_rekey_sigma %.3g)"
              % (key.form, np.abs(err).max(), np.abs(err).max() / sigma, sigma))
        assert np.abs(err).max() < 8 * sigma
        assert np.array_equal(other.decrypt_packed_ints(out, 10, backend=be), direct), key.form
    be.close()
    torch.cuda.empty_cache()
