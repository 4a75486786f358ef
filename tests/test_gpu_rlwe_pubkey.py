"""Compact RLWE public keys on the device (rs_rlwe_pk_encrypt_dev, rs_rlwe_extract_dev): word-for-word
equality with the numpy restatement on every ring and over every shape at which a kernel takes another path, the phase identity
through rs_phase_dev, rlwe_unpack against the keyswitch of the extracted rows, invalid arguments, and the end to end use: an MNIST
image encrypted under the public key runs through sign1024x1 with the layer-wise assertions of a secret-key image, and 64 bits under
a default-128 public key go through a NAND."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

RAND_SEED = bytes(range(60, 92))
MASK_SEED = bytes(range(130, 162))
NOISE_SEED = bytes(range(21, 53))
KEY_SEED = bytes(range(9, 41))
E8 = 1 << 29
GUARD = 0x5A5A5A5A
RING_SET = {1024: "redsec_small_v2", 4096: "redsec_medium", 8192: "redsec_large"}

_BACKENDS = {}


def _backend(N):
    """One context per ring for the whole module (a reduced n: neither call needs a key, and the LWE dimension does not enter)."""
    import redsec_amd
    if N not in _BACKENDS:
        _BACKENDS[N] = redsec_amd.Backend(redsec_amd.params(RING_SET[N], n=16), device=0)
    return _BACKENDS[N]


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    import torch
    for be in _BACKENDS.values():
        be.close()
    _BACKENDS.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def small_v2():
    """redsec_small_v2 at full size under a key generated on the device, and its RLWE public key as an encryptor holds it."""
    import redsec_amd
    import torch
    be = redsec_amd.Backend(redsec_amd.params("redsec_small_v2"), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    pk = sk.rlwe_public_key(MASK_SEED, NOISE_SEED)
    yield be, sk, pk
    be.close()
    torch.cuda.empty_cache()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _check_encrypt(N, count, first, stdev, side_stream=False):
    """Random words for the key: equality of the sums needs no real key, and random words exercise every bit of every word."""
    import torch
    be = _backend(N)
    rng = np.random.default_rng(N + 7 * count)
    pk, mu = _words(rng, 2, N), _words(rng, count)
    want = keygen.rlwe_pk_encrypt(pk, mu, RAND_SEED, first, stdev=stdev)
    R = -(-count // N)
    guard = be.empty(R + 2, 2, N).fill_(GUARD)                               # a ciphertext on either side of the output stays untouched
    out = guard[1:R + 1]
    d_pk, d_mu = _dev(pk), _dev(mu)
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                          # a non-default stream, the consumer ordered behind it
            got = be.rlwe_pk_encrypt(d_pk, d_mu, RAND_SEED, first, stdev, out=out)
            twice = got * 2
        s.synchronize()
        assert np.array_equal(twice.cpu().numpy().view(np.uint32), want.view(np.uint32) * np.uint32(2))
    else:
        got = be.rlwe_pk_encrypt(d_pk, d_mu, RAND_SEED, first, stdev, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (R, 2, N)
    h = got.cpu().numpy()
    assert np.array_equal(h, want), (N, count, first, stdev, np.argwhere(h != want)[:4].tolist())
    assert bool((guard[0] == GUARD).all()) and bool((guard[R + 1] == GUARD).all())
    return want


@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, 2 * 1024 + 5])
def test_encrypt_words_equal_numpy_at_n_1024(count):
    """One slot, one short of a ciphertext, exactly one, one over, two and a ragged third; without noise and with 2^-25; rows
    2^32 - 1, 2^32, 2^32 + 1 (the row counter crosses its low word) and rows from 0."""
    for stdev in (0.0, 2.0 ** -25):
        _check_encrypt(1024, count, (1 << 32) - 1, stdev)
    _check_encrypt(1024, count, 0, 2.0 ** -25, side_stream=True)


def test_encrypt_words_equal_numpy_at_the_last_rows():
    _check_encrypt(1024, 1025, (1 << 64) - 2, 2.0 ** -25)


@pytest.mark.parametrize("N", [4096, 8192])
def test_encrypt_words_equal_numpy_on_the_large_rings(N):
    """count = N + 1: two ciphertexts, the second nearly empty; every coefficient-tile boundary of both polynomials is crossed."""
    _check_encrypt(N, N + 1, (1 << 32) - 1, 2.0 ** -25)


@pytest.mark.parametrize("N,count", [(1024, 1), (1024, 1025), (1024, 2 * 1024 + 5), (4096, 4097)])
def test_extract_words_equal_numpy(N, count):
    be = _backend(N)
    R = -(-count // N)
    rlwe = _words(np.random.default_rng(N + count), R, 2, N)
    want = keygen.rlwe_extract(rlwe, count)
    guard = be.empty(count + 2, N + 1).fill_(GUARD)
    got = be.rlwe_extract(_dev(rlwe), count, out=guard[1:count + 1])
    h = got.cpu().numpy()
    assert h.shape == (count, N + 1)
    assert np.array_equal(h, want), (N, count, np.argwhere(h != want)[:4].tolist())
    assert bool((guard[0] == GUARD).all()) and bool((guard[count + 1] == GUARD).all())


def test_phase_of_the_extracted_rows_is_mu_plus_the_numpy_noise_words(small_v2):
    """rs_phase_dev(dim = N) of the extracted rows, minus mu, equals the noise words of the restatement exactly."""
    be, sk, pk = small_v2
    N, count, alpha = 1024, 2 * 1024 + 5, 2.0 ** -30
    mu = _words(np.random.default_rng(12), count)
    want_ct = keygen.rlwe_pk_encrypt(pk.expand(), mu, RAND_SEED, 9, stdev=alpha)
    noise = keygen.rlwe_phase(want_ct, sk.tlwe_key).ravel()[:count].view(np.uint32) - mu.view(np.uint32)
    ct = be.rlwe_pk_encrypt(pk, _dev(mu), RAND_SEED, 9, alpha)              # the RlwePublicKey itself: expanded by the call
    assert np.array_equal(ct.cpu().numpy(), want_ct)
    rows = be.rlwe_extract(ct, count)
    ph = be.phase(rows, sk.tlwe_key).cpu().numpy()
    assert np.array_equal(ph.view(np.uint32) - mu.view(np.uint32), noise)
    assert 0 < np.abs(noise.view(np.int32)).max() < 8 * alpha * np.sqrt(N + 1) * 2.0 ** 32


def test_unpack_equals_the_keyswitch_of_the_extracted_rows(small_v2):
    be, sk, pk = small_v2
    count = 1024 + 3
    mu = _words(np.random.default_rng(13), count)
    ct = be.rlwe_pk_encrypt(pk, _dev(mu), RAND_SEED, 40)
    got = be.rlwe_unpack(ct, count)
    want = be.keyswitch(be.rlwe_extract(ct, count))
    assert tuple(got.shape) == (count, be.W)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    # and the Python default is a fresh rand seed per call
    a, b = be.rlwe_pk_encrypt(pk, _dev(mu[:4])), be.rlwe_pk_encrypt(pk, _dev(mu[:4]))
    assert not np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def _unpack_sigma(p, alpha, ks_stdev):
    """Deviation of an unpacked input: alpha^2 (N + 1) of the encryption, N t (1 - 2^-basebit) sigma_ks^2 of the keyswitch samples added
    (a digit is zero once in 2^basebit), (N / 2) 2^(-2 t basebit) / 12 of the digits' rounding."""
    N, t, basebit = p.N, p.ks_t, p.ks_basebit
    return np.sqrt(alpha ** 2 * (N + 1) + N * t * (1 - 2.0 ** -basebit) * ks_stdev ** 2 + (N / 2) * 2.0 ** (-2 * t * basebit) / 12)


def _w(s, z):
    return np.where(z == 1, 0, np.where(s == 1, 1, -1)).astype(np.int64)


def test_mnist_image_under_the_public_key_runs_through_sign1024x1(small_v2):
    """An MNIST image of the golden set through rlwe_pk_encrypt_image -> rlwe_unpack: all 784 inputs decrypt to 2 pixel - 255, their
    largest phase error is below 8 sigma (sigma from the formula and the set's constants: 2.7e-6, against a half step of 1.2e-4),
    and the ciphertexts run through nets.EncryptedMnist with the layer-wise assertions of
    test_gpu_keygen.py::test_mnist_sign1024x1_under_a_device_generated_key."""
    import plain_model as pm
    from redsec_amd import nets
    be, sk, pk = small_v2
    p = be.p
    (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS["redsec_small_v2"]
    labels, pixels = pm.load_images()
    px = np.asarray(pixels[0]).ravel()
    assert px.size == 784
    rlwe = be.rlwe_pk_encrypt_image(pk, px)                                   # what the sensor sends: one ciphertext, 8 KB
    assert tuple(rlwe.shape) == (1, 2, 1024)
    ct = be.rlwe_unpack(rlwe, 784)                                            # what the server feeds the network
    assert tuple(ct.shape) == (784, be.W)
    h = ct.cpu().numpy()
    v = 2 * px.astype(np.int64) - 255
    assert np.array_equal(sk.decrypt_ints(h), v)
    err = (sk.phase(h).view(np.uint32) - (v * (1 << 20)).astype(np.int32).view(np.uint32)).view(np.int32) / 2.0 ** 32
    sigma = _unpack_sigma(p, bk_stdev, ks_stdev)
    print("largest phase error %.3g = %.2f sigma (sigma %.3g), deviation %.3g" % (np.abs(err).max(), np.abs(err).max() / sigma, sigma, err.std()))
    assert 2.6e-6 < sigma < 2.8e-6
    assert np.abs(err).max() < 8 * sigma

    ks_round = np.sqrt(p.N / 24.0) * 2.0 ** -(p.ks_t * p.ks_basebit) * 4096   # std per bootstrapped output, in 1/4096
    net = pm.load_net("sign1024x1")
    enc = nets.EncryptedMnist(be, net)
    taps, ptaps = {}, {}
    out = enc.run(ct, taps)
    pm.forward(net, pixels[0], ptaps)
    assert out.shape == (10, be.W)
    pre0 = sk.decrypt_ints(taps["pre0"].cpu().numpy())
    assert np.abs(pre0 - ptaps["pre0"]).max() <= 2
    bits0 = np.where(sk.phase(taps["bits0"].cpu().numpy()) > 0, 1, -1)
    strong = np.abs(ptaps["pre0"]) >= 32
    assert np.array_equal(bits0[strong], ptaps["bits0"][strong])
    s, z, b = net.fc[0]
    W1 = _w(s, z)
    expect1 = bits0 @ W1 + b
    pre1 = sk.decrypt_ints(taps["pre1"].cpu().numpy())
    assert np.abs(pre1 - expect1).max() <= 2 + 6 * ks_round * np.sqrt(np.abs(W1).sum(axis=0).max())
    bits1 = np.where(sk.phase(taps["bits1"].cpu().numpy()) > 0, 1, -1)
    strong = np.abs(expect1) >= 32
    assert np.array_equal(bits1[strong], np.where(expect1 >= 0, 1, -1)[strong])
    ph = sk.phase(taps["bits1"].cpu().numpy()).astype(np.float64) / (1 << 20)
    assert np.all(np.abs(np.abs(ph) - 1.0) < max(0.25, 6 * ks_round))
    s, z, b = net.final
    W2 = _w(s, z)
    logits = sk.decrypt_ints(out.cpu().numpy())
    assert np.abs(logits - (bits1 @ W2 + b)).max() <= 3 + 6 * ks_round * np.sqrt(np.abs(W2).sum(axis=0).max())


def test_default128_bits_under_the_public_key_go_through_a_nand():
    """64 bits in the +-1/8 encoding under a default-128 RLWE public key, unpacked: they decrypt, and so does their NAND."""
    import redsec_amd
    import torch
    name = "default128"
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    pk = sk.rlwe_public_key(MASK_SEED, NOISE_SEED)
    assert pk.nbytes == 32 + 4096
    rng = np.random.default_rng(11)
    x, y = rng.integers(0, 2, 64), rng.integers(0, 2, 64)
    mu = np.where(np.concatenate([x, y]) != 0, E8, -E8).astype(np.int32)
    ct = be.rlwe_unpack(be.rlwe_pk_encrypt(pk, _dev(mu), RAND_SEED), 128)
    a, b = ct[:64].contiguous(), ct[64:].contiguous()
    assert np.array_equal(sk.decrypt_bits(a.cpu().numpy()), x) and np.array_equal(sk.decrypt_bits(b.cpu().numpy()), y)
    (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    err = (sk.phase(ct.cpu().numpy()).view(np.uint32) - mu.view(np.uint32)).view(np.int32) / 2.0 ** 32
    assert np.abs(err).max() < 8 * _unpack_sigma(be.p, bk_stdev, ks_stdev) < 1 / 16
    nand = be.gate("NAND", a, b)
    assert np.array_equal(sk.decrypt_bits(nand.cpu().numpy()), 1 - (x & y))
    be.close()
    torch.cuda.empty_cache()


def test_invalid_arguments_and_the_empty_batch():
    import torch
    N, count = 1024, 5
    be = _backend(N)
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    pk, mu = _dev(_words(rng, 2, N)), _dev(_words(rng, count))
    ct = be.empty(1, 2, N).fill_(7)
    rows = be.empty(count, N + 1).fill_(7)
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())

    def enc(c=P(ct), k=P(pk), u=P(mu), n=count, seed=RAND_SEED, first=0, stdev=0.0):
        return L.rs_rlwe_pk_encrypt_dev(be.h, c, k, u, n, seed, first, stdev, None)

    def ext(u=P(rows), c=P(ct), n=count):
        return L.rs_rlwe_extract_dev(be.h, u, c, n, None)
    assert enc(c=None) == -1 and enc(k=None) == -1 and enc(u=None) == -1 and enc(seed=None) == -1
    assert b"null pointer" in L.rs_last_error()
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert enc(stdev=bad) == -1 and b"finite and non-negative" in L.rs_last_error()
    assert enc(first=(1 << 64) - 1, n=N + 1) == -1 and b"2^64" in L.rs_last_error()      # two ciphertexts from the last row
    assert enc(n=1 << 62) == -1 and b"too large" in L.rs_last_error()                     # R 2 N 4 bytes passes the address space
    assert enc(n=(1 << 64) - 1) == -1
    assert ext(u=None) == -1 and ext(c=None) == -1 and b"null pointer" in L.rs_last_error()
    assert ext(n=1 << 62) == -1 and b"too large" in L.rs_last_error()
    # nothing above launched anything; count = 0 is a no-op wherever `first` is
    assert enc(n=0) == 0 and enc(n=0, first=(1 << 64) - 1) == 0 and ext(n=0) == 0
    torch.cuda.synchronize()
    assert bool((ct == 7).all()) and bool((rows == 7).all())
    assert enc(first=(1 << 64) - 1) == 0                                                  # one ciphertext AT the last row
    assert ext() == 0
    torch.cuda.synchronize()
    want = keygen.rlwe_pk_encrypt(pk.cpu().numpy(), mu.cpu().numpy(), RAND_SEED, (1 << 64) - 1, stdev=0.0)
    assert np.array_equal(ct.cpu().numpy(), want)
    assert np.array_equal(rows.cpu().numpy(), keygen.rlwe_extract(want, count))
    # the Python layer: a key of another set is refused (default-128 and the REDsec set share N = 1024, not the deviation)
    other = client.SecretKeySet.from_secret("default128", *keygen.secret_keys("default128", KEY_SEED)).rlwe_public_key(MASK_SEED, NOISE_SEED)
    with pytest.raises(ValueError, match="default128"):
        be.rlwe_pk_encrypt(other, mu)
    # ... and no silent noise-free ciphertexts on the large rings
    with pytest.raises(ValueError, match="explicit stdev"):
        _backend(4096).rlwe_pk_encrypt(_dev(np.zeros((2, 4096), np.int32)), _dev(np.zeros(3, np.int32)))
