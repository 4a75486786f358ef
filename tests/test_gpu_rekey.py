"""Re-keying on the device (rs_rekey_dev): word-for-word equality with the numpy restatement over every
batch size, width and digit shape at which the kernel takes another path, invalid arguments, and the end to end uses: NAND results
of one default-128 secret re-keyed to another and used again there, the ten logits of an MNIST image on redsec_small_v2 re-keyed to
the ring key behind a second secret's RLWE public key, and bits crossing from redsec_small_v2 to default-128."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

MASK_SEED = bytes(range(150, 182))
NOISE_SEED = bytes(range(31, 63))
RAND_SEED = bytes(range(200, 232))
KEY_SEED = bytes(range(9, 41))
OTHER_SEED = bytes(range(90, 122))
GUARD = 0x5A5A5A5A

_BACKENDS = {}
_REF = {}


def _backend():
    """One context for the whole module: the call needs no key and takes both dimensions as arguments, so a context of any set
    serves every shape below."""
    import redsec_amd
    if "any" not in _BACKENDS:
        _BACKENDS["any"] = redsec_amd.Backend(redsec_amd.params("redsec_small_v2", n=16), device=0)
    return _BACKENDS["any"]


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    import torch
    for be in _BACKENDS.values():
        be.close()
    _BACKENDS.clear()
    _REF.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def pair128():
    """Two default-128 contexts at full size, each under a key generated on the device from a seed of its own."""
    import redsec_amd
    import torch
    out = []
    for seed in (KEY_SEED, OTHER_SEED):
        be = redsec_amd.Backend(redsec_amd.params("default128"), device=0)
        sk, bk, ksk = keygen.generate(be, seed=seed)
        del bk, ksk
        out.append((be, sk))
    assert not np.array_equal(out[0][1].lwe_key, out[1][1].lwe_key)
    yield out
    for be, _ in out:
        be.close()
    torch.cuda.empty_cache()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _inputs(n_src, n_dst, basebit, t, most):
    """Random words for key and samples (equality of the sums needs no real key, and random words exercise every bit of every
    word), made once per shape with the restatement of all `most` samples; a smaller batch takes the first rows of both."""
    k = (n_src, n_dst, basebit, t)
    if k not in _REF:
        rng = np.random.default_rng(n_src + 5 * n_dst + 100 * basebit + t)
        key, ct = _words(rng, n_src, t, n_dst + 1), _words(rng, most, n_src + 1)
        _REF[k] = (key, ct, keygen.rekey(ct, key, basebit, t))
    key, ct, want = _REF[k]
    assert ct.shape[0] >= most
    return key, ct, want


def _check_rekey(n_src, n_dst, B, basebit, t, most=None, side_stream=False):
    import torch
    be = _backend()
    key, ct, want = _inputs(n_src, n_dst, basebit, t, most or B)
    ct, want = ct[:B], want[:B]
    guard = be.empty(B + 2, n_dst + 1).fill_(GUARD)                         # a row on either side of the output stays untouched
    out = guard[1:B + 1]
    d_key, d_ct = _dev(key), _dev(ct)
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                          # a non-default stream, the consumer ordered behind it
            got = be.rekey(d_ct, d_key, basebit, t, out=out)
            twice = got * 2
        s.synchronize()
        assert np.array_equal(twice.cpu().numpy().view(np.uint32), want.view(np.uint32) * np.uint32(2))
    else:
        got = be.rekey(d_ct, d_key, basebit, t, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (B, n_dst + 1)
    h = got.cpu().numpy()
    assert np.array_equal(h, want), (n_src, n_dst, B, basebit, t, np.argwhere(h != want)[:4].tolist())
    # a second call into the same buffer starts from (0, b) again: the same words, not twice the sums
    be.rekey(d_ct, d_key, basebit, t, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((guard[0] == GUARD).all()) and bool((guard[B + 1] == GUARD).all())


@pytest.mark.parametrize("B", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 1000])
def test_rekey_words_equal_numpy_at_every_batch_edge(B):
    """n_src = 37 (five index chunks, the last of 5 indices), n_dst = 350 (six word tiles, the last of 31 words) at (4, 5): the
    edges of a wave's 32 ciphertexts and of a workgroup's 128, a ragged third tile, eight tiles. The ragged count also runs on a
    side stream with a dependent consumer."""
    _check_rekey(37, 350, B, 4, 5, most=1000)
    if B == 257:
        _check_rekey(37, 350, B, 4, 5, most=1000, side_stream=True)


@pytest.mark.parametrize("n_dst", [1, 63, 64, 255, 256, 630, 1024, 8192])
def test_rekey_words_equal_numpy_at_every_destination_width(n_dst):
    """n_src = 5, B = 33: two output words; one word tile exactly (n_dst + 1 = 64) and one word more; four tiles exactly and one
    word more; default-128's width, a ring key's, the largest ring's."""
    _check_rekey(5, n_dst, 33, 4, 5)


@pytest.mark.parametrize("n_src", [1, 7, 8, 9, 630])
def test_rekey_words_equal_numpy_at_every_source_width(n_src):
    """n_dst = 16, B = 5, (2, 8): one index; one short of, exactly and one past the index chunk; default-128's 79 chunks."""
    _check_rekey(n_src, 16, 5, 2, 8)


@pytest.mark.parametrize("basebit,t", [(2, 8), (8, 4), (3, 5), (1, 32), (4, 4)])
def test_rekey_words_equal_numpy_for_every_digit_shape(basebit, t):
    """n_src = 16, n_dst = 37, B = 65: 16 and 32 bits in narrow and wide digits, a basebit that does not divide 32 with an odd t,
    offset 0 at 32 bits."""
    _check_rekey(16, 37, 65, basebit, t)


def test_rekey_words_equal_numpy_at_the_real_size():
    """default-128 to default-128 at rekey_default: n_src = n_dst = 630, (2, 8), B = 1,024 (four chunks a workgroup, 20 splits)."""
    assert keygen.rekey_default("default128") == (2, 8)
    _check_rekey(630, 630, 1024, 2, 8)


def test_default128_nand_results_rekeyed_decrypted_and_used_again(pair128):
    """128 bits under the first secret, a NAND, the 64 results re-keyed with a rekey_to key whose bodies were made on the device:
    they decrypt under the second secret, every phase lies within 8 rekey_sigma of its source phase, and they feed a NAND on the
    second context, which holds the second secret's evaluation key."""
    (be1, sk1), (be2, sk2) = pair128
    key = sk1.rekey_to(sk2, mask_seed=MASK_SEED, noise_seed=NOISE_SEED, backend=be2)
    assert (key.basebit, key.t, key.n_src, key.n_dst, key.nbytes) == (2, 8, 630, 630, 32 + 4 * 630 * 8)
    d_key = be1.upload_rekey_key(key)
    assert tuple(d_key.shape) == (630, 8, 631)
    rng = np.random.default_rng(21)
    x, y = rng.integers(0, 2, 64), rng.integers(0, 2, 64)
    ct = _dev(sk1.encrypt_bits(np.concatenate([x, y]), seed=3))
    nand = be1.gate("NAND", ct[:64].contiguous(), ct[64:].contiguous())
    want = 1 - (x & y)
    out = be1.rekey(nand, d_key, key.basebit, key.t)
    assert tuple(out.shape) == (64, 631)
    assert np.array_equal(sk2.decrypt_bits(out.cpu().numpy()), want)
    assert np.array_equal(sk2.decrypt_bits(out, backend=be2), want)
    sigma = keygen.rekey_sigma(630, key.basebit, key.t, client.PARAM_SETS["default128"][7])
    err = (_u32(sk2.phase(out.cpu().numpy())) - _u32(sk1.phase(nand.cpu().numpy()))).view(np.int32) / 2.0 ** 32
    print("default-128, 64 results: largest re-keying error %.3g = %.2f sigma (rekey_sigma %.3g), rms %.3g"
          % (np.abs(err).max(), np.abs(err).max() / sigma, sigma, np.sqrt(np.mean(err * err))))
    assert np.abs(err).max() < 8 * sigma < 1 / 16
    nand2 = be2.gate("NAND", out[:32].contiguous(), out[32:].contiguous())
    assert np.array_equal(sk2.decrypt_bits(nand2.cpu().numpy()), 1 - (want[:32] & want[32:]))
    # the same key as a RekeyKey, expanded and uploaded by the call, and the host-made key: the same words
    assert np.array_equal(be1.rekey(nand, key).cpu().numpy(), out.cpu().numpy())
    host = sk1.rekey_to(sk2, mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    assert np.abs(host.body.astype(np.int64) - key.body.astype(np.int64)).max() <= 1     # numpy's log / cos: the last bit of a noise word
    assert np.array_equal(keygen.rekey(nand.cpu().numpy(), key.expand(), key.basebit, key.t), out.cpu().numpy())


def test_bits_cross_from_redsec_small_v2_to_default128(pair128):
    """Bits encrypted under a redsec_small_v2 secret (n = 350) are re-keyed to the second default-128 secret (n = 630): they decrypt
    there and feed a default-128 gate."""
    _, (be2, sk2) = pair128
    src = client.SecretKeySet.from_secret("redsec_small_v2", *keygen.secret_keys("redsec_small_v2", KEY_SEED))
    key = src.rekey_to(sk2, mask_seed=MASK_SEED, noise_seed=NOISE_SEED, backend=be2)
    assert (key.src_name, key.dst_name, key.n_src, key.n_dst, key.basebit, key.t) == ("redsec_small_v2", "default128", 350, 630, 2, 8)
    rng = np.random.default_rng(23)
    x, y = rng.integers(0, 2, 32), rng.integers(0, 2, 32)
    ct = _dev(src.encrypt_bits(np.concatenate([x, y]), seed=8))
    out = be2.rekey(ct, key)
    assert tuple(out.shape) == (64, 631)
    assert np.array_equal(sk2.decrypt_bits(out.cpu().numpy()), np.concatenate([x, y]))
    sigma = keygen.rekey_sigma(350, 2, 8, client.PARAM_SETS["default128"][7])
    err = (_u32(sk2.phase(out.cpu().numpy())) - _u32(src.phase(ct.cpu().numpy()))).view(np.int32) / 2.0 ** 32
    assert np.abs(err).max() < 8 * sigma < 1 / 16
    gate = be2.gate("XOR", out[:32].contiguous(), out[32:].contiguous())
    assert np.array_equal(sk2.decrypt_bits(gate.cpu().numpy()), x ^ y)


def test_mnist_logits_rekeyed_to_a_ring_key_on_redsec_small_v2():
    """The ten logit ciphertexts of nets.EncryptedMnist for one golden image, re-keyed with a rekey_for key made from a second
    secret's RLWE public key alone: each phase under that ring key lies within 8 rekey_sigma of the logit's phase under the first
    secret (phases, not rounded integers: a logit near a rounding boundary proves nothing about the re-keying), and the device and
    numpy decryptions agree word for word."""
    import plain_model as pm
    import redsec_amd
    import torch
    from redsec_amd import nets
    name = "redsec_small_v2"
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    other = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, OTHER_SEED))
    pk = other.rlwe_public_key(MASK_SEED, NOISE_SEED)
    key = sk.rekey_for(pk, rand_seed=RAND_SEED, backend=be)
    assert (key.form, key.basebit, key.t, key.n_src, key.n_dst) == ("rlwe", 4, 5, 350, 1024) and key.rlwe.shape == (2, 2, 1024)
    labels, pixels = pm.load_images()
    logits = nets.EncryptedMnist(be, pm.load_net("sign1024x1")).run(_dev(sk.encrypt_image(np.asarray(pixels[0]).ravel())))
    assert tuple(logits.shape) == (10, be.W)
    out = be.rekey(logits.contiguous(), key)
    assert tuple(out.shape) == (10, 1025)
    stdev = client.PARAM_SETS[name][8]
    sigma = keygen.rekey_sigma(350, 4, 5, stdev * np.sqrt(1025.0))
    plain = sk.phase(logits.cpu().numpy())
    there = other.phase(out.cpu().numpy(), ring=True)
    err = (_u32(there) - _u32(plain)).view(np.int32) / 2.0 ** 32
    print("redsec_small_v2, 10 logits: largest re-keying error %.3g = %.2f sigma (rekey_sigma %.3g)" % (np.abs(err).max(), np.abs(err).max() / sigma, sigma))
    assert 1.0e-5 < sigma < 1.2e-5 and np.abs(err).max() < 8 * sigma
    assert np.array_equal(other.phase(out, backend=be, ring=True), there)
    assert np.array_equal(keygen.rekey(logits.cpu().numpy(), key.expand(), 4, 5), out.cpu().numpy())
    be.close()
    torch.cuda.empty_cache()


def test_invalid_arguments_and_the_empty_batch():
    import torch
    n_src, n_dst, B = 9, 16, 5
    be = _backend()
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    key, ct = _dev(_words(rng, n_src, 5, n_dst + 1)), _dev(_words(rng, B, n_src + 1))
    out = be.empty(B, n_dst + 1).fill_(7)
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())

    def rekey(o=P(out), c=P(ct), b=B, ns=n_src, k=P(key), nd=n_dst, basebit=4, t=5):
        return L.rs_rekey_dev(be.h, o, c, b, ns, k, nd, basebit, t, None)
    assert rekey(o=None) == -1 and rekey(c=None) == -1 and rekey(k=None) == -1 and b"null pointer" in L.rs_last_error()
    for bad in (0, -1, 65537):
        assert rekey(ns=bad) == -1 and b"n_src" in L.rs_last_error() and b"outside 1 .. 65536" in L.rs_last_error()
        assert rekey(nd=bad) == -1 and b"n_dst" in L.rs_last_error() and b"outside 1 .. 65536" in L.rs_last_error()
    for bad in (0, 9, -1):
        assert rekey(basebit=bad, t=1) == -1 and b"outside 1 .. 8" in L.rs_last_error()
    for bad in (0, -3):
        assert rekey(t=bad) == -1 and b"below 1" in L.rs_last_error()
    for basebit, t in ((4, 9), (8, 5), (1, 33), (3, 11)):
        assert rekey(basebit=basebit, t=t) == -1 and b"passes 32 bits" in L.rs_last_error()
    assert rekey(b=1 << 62) == -1 and b"too large" in L.rs_last_error()
    assert rekey(b=(1 << 64) - 1) == -1 and b"too large" in L.rs_last_error()
    assert rekey(b=1 << 44) == -1 and b"too large for one launch" in L.rs_last_error()   # fits the address space, not one launch
    # an out that shares a byte with an input is refused: the kernels add into it with atomics after an init kernel has set it.
    # Every range named below lies inside one allocation of 512 words or inside the key (765 words, out is 85)
    arena = _dev(_words(rng, 512))
    held, held_key = arena.cpu().numpy(), key.cpu().numpy()
    A, K, row = arena.data_ptr(), key.data_ptr(), 4 * (n_src + 1)
    for o in (A, A + row, A + B * row - 4):                                   # out == ct, one sample into ct, on its last word
        assert rekey(o=vp(o), c=vp(A)) == -1 and b"out overlaps ct" in L.rs_last_error()
    assert rekey(o=vp(A), c=vp(A + 4 * B * (n_dst + 1) - 4)) == -1 and b"out overlaps ct" in L.rs_last_error()   # out's last word is ct's first
    for o in (K, K + 4 * (n_dst + 1), K + 4 * (key.numel() - B * (n_dst + 1))):   # out on the key's first and second row and its end
        assert rekey(o=vp(o)) == -1 and b"out overlaps rekey_key" in L.rs_last_error()
    with pytest.raises(ValueError, match="out overlaps ct"):
        be.rekey(arena[:B * (n_src + 1)].view(B, n_src + 1), key, 4, 5, out=arena[:B * (n_dst + 1)])
    with pytest.raises(ValueError, match="out overlaps rekey_key"):
        be.rekey(ct, key, 4, 5, out=key.view(-1)[:B * (n_dst + 1)])
    # nothing above launched anything; B = 0 is a no-op
    assert rekey(b=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert np.array_equal(arena.cpu().numpy(), held) and np.array_equal(key.cpu().numpy(), held_key)
    assert rekey() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), keygen.rekey(ct.cpu().numpy(), key.cpu().numpy(), 4, 5))


def test_python_refusals():
    """A key of another destination is refused, by its n for the seeded form and by its ring for the RLWE form; a bare tensor needs
    its digit shape, and the shape it has."""
    be = _backend()                                                          # redsec_small_v2 with n = 16
    secret = lambda name, n, seed: client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, seed, n))
    src = secret("default128", 9, KEY_SEED)
    ct = _dev(src.encrypt_bits(np.ones(4, np.int64), seed=2))
    with pytest.raises(ValueError, match="n = 17"):
        be.rekey(ct, src.rekey_to(secret("redsec_small_v2", 17, OTHER_SEED), mask_seed=MASK_SEED, noise_seed=NOISE_SEED))
    big = client.RlwePublicKey("redsec_medium", MASK_SEED, np.zeros(4096, np.int32))
    with pytest.raises(ValueError, match="N = 4096"):
        be.rekey(ct, src.rekey_for(big, rand_seed=RAND_SEED, stdev=2.0 ** -31))
    good = src.rekey_to(secret("default128", 16, OTHER_SEED), mask_seed=MASK_SEED, noise_seed=NOISE_SEED)   # n matches, the set need not
    d_key = be.upload_rekey_key(good)
    assert tuple(be.rekey(ct, good).shape) == (4, 17)
    with pytest.raises(ValueError, match="explicit basebit"):
        be.rekey(ct, d_key)
    with pytest.raises(ValueError):
        be.rekey(ct, d_key, 4, 9)
    with pytest.raises(ValueError, match="n_src"):
        be.rekey(ct, d_key, 4, 4)                                            # the key has t = 8
