"""Packed results on the device (rs_pack_dev): word-for-word equality with the numpy restatement on every
ring, over every count at which the kernel takes another path and every digit shape, decryption through the device and through
numpy, invalid arguments, and the end to end uses: NAND results of a default-128 key packed, decrypted, unpacked and used again,
the ten logits of an MNIST image on redsec_small_v2, and the output bits of a compiled adder."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

MASK_SEED = bytes(range(150, 182))
NOISE_SEED = bytes(range(31, 63))
KEY_SEED = bytes(range(9, 41))
GUARD = 0x5A5A5A5A
RING_SET = {1024: "redsec_small_v2", 4096: "redsec_medium", 8192: "redsec_large"}

_BACKENDS = {}
_REF = {}


def _backend(N, n):
    """One context per (ring, n) for the whole module: the call needs no key, only the context's N and n."""
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
    _REF.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def default128():
    """default-128 at full size under a key generated on the device, and a packing key of pack_default as a server holds it."""
    import redsec_amd
    import torch
    be = redsec_amd.Backend(redsec_amd.params("default128"), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    key = sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    assert (key.basebit, key.t) == keygen.pack_default("default128") == (4, 4) and key.nbytes == 32 + 4 * 630 * 4 * 1024
    yield be, sk, key, be.upload_packing_key(key)
    be.close()
    torch.cuda.empty_cache()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _inputs(N, n, basebit, t, most):
    """Random words for key and samples (equality of the sums needs no real key, and random words exercise every bit of every
    word), made once per shape; a smaller count takes the first samples."""
    k = (N, n, basebit, t)
    if k not in _REF:
        rng = np.random.default_rng(N + 5 * n + 100 * basebit + t)
        _REF[k] = (_words(rng, n, t, 2, N), _words(rng, most, n + 1))
    key, ct = _REF[k]
    assert ct.shape[0] >= most
    return key, ct


def _check_pack(N, n, count, basebit, t, most=None, side_stream=False):
    import torch
    be = _backend(N, n)
    key, ct = _inputs(N, n, basebit, t, most or count)
    ct = ct[:count]
    want = keygen.pack(ct, key, basebit, t)
    R = -(-count // N)
    guard = be.empty(R + 2, 2, N).fill_(GUARD)                               # a ciphertext on either side of the output stays untouched
    out = guard[1:R + 1]
    d_key, d_ct = _dev(key), _dev(ct)
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                          # a non-default stream, the consumer ordered behind it
            got = be.pack(d_ct, d_key, basebit, t, out=out)
            twice = got * 2
        s.synchronize()
        assert np.array_equal(twice.cpu().numpy().view(np.uint32), want.view(np.uint32) * np.uint32(2))
    else:
        got = be.pack(d_ct, d_key, basebit, t, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (R, 2, N)
    h = got.cpu().numpy()
    assert np.array_equal(h, want), (N, n, count, basebit, t, np.argwhere(h != want)[:4].tolist())
    # a second call into the same buffer starts from (0, sum b X^c) again: the same words, not twice the sums
    be.pack(d_ct, d_key, basebit, t, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((guard[0] == GUARD).all()) and bool((guard[R + 1] == GUARD).all())
    return want


@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, 2 * 1024 + 5, 5 * 1024])
def test_pack_words_equal_numpy_at_n_1024(count):
    """n = 37 (five index chunks, the last of 5 indices) at (4, 5): one slot, one short of a ciphertext, exactly one, one over (the
    second with a single slot), two and a ragged third, five full ones. The ragged count also runs on a side stream with a
    dependent consumer."""
    _check_pack(1024, 37, count, 4, 5, most=5 * 1024)
    if count == 2 * 1024 + 5:
        _check_pack(1024, 37, count, 4, 5, most=5 * 1024, side_stream=True)


@pytest.mark.parametrize("basebit,t", [(2, 8), (8, 4), (3, 5), (1, 32)])
def test_pack_words_equal_numpy_for_every_digit_shape(basebit, t):
    """n = 16, 1,025 slots: 16 and 32 bits in narrow and wide digits, a basebit that does not divide 32, offset 0 at 32 bits."""
    _check_pack(1024, 16, 1025, basebit, t)


@pytest.mark.parametrize("N,n", [(4096, 8), (8192, 5)])
def test_pack_words_equal_numpy_on_the_large_rings(N, n):
    """count = N + 1: four and eight slot blocks, every coefficient tile of both polynomials, the second ciphertext with one slot."""
    _check_pack(N, n, N + 1, 4, 5)


def test_packed_phases_through_the_device_and_through_numpy():
    """rs_rlwe_extract_dev + rs_phase_dev(dim = N) of a packed ciphertext equals keygen.rlwe_phase of it, and both equal the sample
    phases plus the error words of the restatement, exactly."""
    N, n, count, (basebit, t) = 1024, 16, 1024 + 9, (4, 5)
    be = _backend(N, n)
    sk = client.SecretKeySet.from_secret("redsec_small_v2", *keygen.secret_keys("redsec_small_v2", KEY_SEED, n))
    key = sk.packing_key(basebit, t, MASK_SEED, NOISE_SEED)
    v = np.random.default_rng(2).integers(-2048, 2048, count)
    ct = sk.encrypt_torus(v * (1 << 20), 2.0 ** -25, 5)
    want = keygen.pack(ct, key.expand(), basebit, t)
    err = sk.packed_phase(want, count).view(np.uint32) - sk.phase(ct).view(np.uint32)
    packed = be.pack(_dev(ct), key)                                          # the PackingKey itself: expanded and uploaded by the call
    assert np.array_equal(packed.cpu().numpy(), want)
    on_device = sk.packed_phase(packed, count, backend=be)
    assert np.array_equal(on_device, keygen.rlwe_phase(packed.cpu().numpy(), sk.tlwe_key).ravel()[:count])
    assert np.array_equal(on_device.view(np.uint32), sk.phase(ct).view(np.uint32) + err)
    sigma = keygen.pack_sigma(n, N, basebit, t, count, 2.0 ** -30)
    assert 0 < np.abs(err.view(np.int32)).max() < 8 * sigma * 2.0 ** 32
    assert np.array_equal(sk.decrypt_packed_ints(packed, count, backend=be), v)


def test_default128_nand_results_packed_decrypted_and_used_again(default128):
    """128 bits, a NAND, the 64 results packed under the default key (4, 4): they decrypt from the packed ciphertext, every packed
    phase lies within 8 pack_sigma of the unpacked result's, and rlwe_unpack of the packed ciphertext feeds another NAND."""
    be, sk, key, d_key = default128
    rng = np.random.default_rng(21)
    x, y = rng.integers(0, 2, 64), rng.integers(0, 2, 64)
    ct = _dev(sk.encrypt_bits(np.concatenate([x, y]), seed=3))
    nand = be.gate("NAND", ct[:64].contiguous(), ct[64:].contiguous())
    want = 1 - (x & y)
    packed = be.pack(nand, d_key, key.basebit, key.t)
    assert tuple(packed.shape) == (1, 2, 1024)
    assert np.array_equal(sk.decrypt_packed_bits(packed.cpu().numpy(), 64), want)
    assert np.array_equal(sk.decrypt_packed_bits(packed, 64, backend=be), want)
    sigma = keygen.pack_sigma(630, 1024, key.basebit, key.t, 64, client.PARAM_SETS["default128"][8])
    err = (sk.packed_phase(packed.cpu().numpy(), 64).view(np.uint32) - sk.phase(nand.cpu().numpy()).view(np.uint32)).view(np.int32) / 2.0 ** 32
    print("default-128, 64 slots: largest packing error %.3g = %.2f sigma (pack_sigma %.3g), rms %.3g" % (np.abs(err).max(), np.abs(err).max() / sigma, sigma, np.sqrt(np.mean(err * err))))
    assert np.abs(err).max() < 8 * sigma < 1 / 16
    again = be.rlwe_unpack(packed, 64)
    assert np.array_equal(sk.decrypt_bits(again.cpu().numpy()), want)
    nand2 = be.gate("NAND", again[:32].contiguous(), again[32:].contiguous())
    assert np.array_equal(sk.decrypt_bits(nand2.cpu().numpy()), 1 - (want[:32] & want[32:]))
    # the same key as a PackingKey, expanded and uploaded by the call: the same words
    assert np.array_equal(be.pack(nand, key).cpu().numpy(), packed.cpu().numpy())


def test_adder_outputs_of_a_circuit_packed_in_one_call(default128):
    """circuit.adder(4) over 64 lanes: the 5 x 64 output bits go into one packed ciphertext of 320 slots, and the sums decrypt."""
    from redsec_amd import circuit
    be, sk, key, d_key = default128
    rng = np.random.default_rng(22)
    xa, xb = rng.integers(0, 16, 64), rng.integers(0, 16, 64)
    bits = np.stack([(x >> i) & 1 for x in (xa, xb) for i in range(4)])
    inputs = _dev(sk.encrypt_bits(bits.ravel(), seed=4).reshape(8, 64, be.W))
    bound = circuit.adder(4).compile().bind(be)
    outs = bound.run(inputs)
    assert tuple(outs.shape) == (5, 64, be.W)
    packed = be.pack(outs.reshape(320, be.W).contiguous(), d_key, key.basebit, key.t)
    got = sk.decrypt_packed_bits(packed.cpu().numpy(), 320).reshape(5, 64)
    assert np.array_equal(sum(got[i] << i for i in range(5)), xa + xb)
    bound.close()


def test_mnist_logits_packed_on_redsec_small_v2():
    """The ten logit ciphertexts of nets.EncryptedMnist for one golden image, packed with (4, 5): each packed phase lies within
    8 pack_sigma(count = 10) of the unpacked logit's phase (phases, not rounded integers: a logit near a rounding boundary proves
    nothing about the packing)."""
    import plain_model as pm
    import redsec_amd
    import torch
    from redsec_amd import nets
    name = "redsec_small_v2"
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    key = sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    assert (key.basebit, key.t) == (4, 5)
    labels, pixels = pm.load_images()
    logits = nets.EncryptedMnist(be, pm.load_net("sign1024x1")).run(_dev(sk.encrypt_image(np.asarray(pixels[0]).ravel())))
    assert tuple(logits.shape) == (10, be.W)
    packed = be.pack(logits.contiguous(), key)
    assert tuple(packed.shape) == (1, 2, 1024)
    sigma = keygen.pack_sigma(be.p.n, 1024, 4, 5, 10, client.PARAM_SETS[name][8])
    plain = sk.phase(logits.cpu().numpy())
    err = (sk.packed_phase(packed.cpu().numpy(), 10).view(np.uint32) - plain.view(np.uint32)).view(np.int32) / 2.0 ** 32
    print("redsec_small_v2, 10 logits: largest packing error %.3g = %.2f sigma (pack_sigma %.3g)" % (np.abs(err).max(), np.abs(err).max() / sigma, sigma))
    assert 3e-6 < sigma < 5e-6 and np.abs(err).max() < 8 * sigma
    assert np.array_equal(sk.packed_phase(packed, 10, backend=be), sk.packed_phase(packed.cpu().numpy(), 10))
    be.close()
    torch.cuda.empty_cache()


def test_invalid_arguments_and_the_empty_batch():
    import torch
    N, n, count = 1024, 16, 5
    be = _backend(N, n)
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    key, ct = _dev(_words(rng, n, 5, 2, N)), _dev(_words(rng, count, n + 1))
    out = be.empty(1, 2, N).fill_(7)
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())

    def pack(o=P(out), c=P(ct), cnt=count, k=P(key), basebit=4, t=5):
        return L.rs_pack_dev(be.h, o, c, cnt, k, basebit, t, None)
    assert pack(o=None) == -1 and pack(c=None) == -1 and pack(k=None) == -1 and b"null pointer" in L.rs_last_error()
    for bad in (0, 9, -1):
        assert pack(basebit=bad, t=1) == -1 and b"outside 1 .. 8" in L.rs_last_error()
    for bad in (0, -3):
        assert pack(t=bad) == -1 and b"below 1" in L.rs_last_error()
    for basebit, t in ((4, 9), (8, 5), (1, 33), (3, 11)):
        assert pack(basebit=basebit, t=t) == -1 and b"passes 32 bits" in L.rs_last_error()
    assert pack(cnt=1 << 62) == -1 and b"too large" in L.rs_last_error()
    assert pack(cnt=(1 << 64) - 1) == -1 and b"too large" in L.rs_last_error()
    assert pack(cnt=1 << 44) == -1 and b"too large" in L.rs_last_error()          # fits the address space, not one launch
    # an rlwe that shares a byte with an input is refused: the kernels add into it with atomics after an init kernel has set it.
    # Every range named below lies inside one allocation of four ciphertexts (ct at its start or behind its first ciphertext) or
    # inside the key
    arena = _dev(_words(rng, 4 * 2 * N))
    held, held_key = arena.cpu().numpy(), key.cpu().numpy()
    A, K, row = arena.data_ptr(), key.data_ptr(), 4 * (n + 1)
    for o in (A, A + row, A + count * row - 4):                               # rlwe == ct, one sample into ct, on its last word
        assert pack(o=vp(o), c=vp(A)) == -1 and b"rlwe overlaps ct" in L.rs_last_error()
    assert pack(o=vp(A), c=vp(A + 8 * N - 4)) == -1 and b"rlwe overlaps ct" in L.rs_last_error()   # the last word of rlwe is ct's first
    for o in (K, K + 8 * N, K + 4 * key.numel() - 8 * N):                     # rlwe on the key's first, second and last sample
        assert pack(o=vp(o)) == -1 and b"rlwe overlaps pack_key" in L.rs_last_error()
    with pytest.raises(ValueError, match="rlwe overlaps ct"):
        be.pack(arena[:count * (n + 1)].view(count, n + 1), key, 4, 5, out=arena[:2 * N])
    with pytest.raises(ValueError, match="rlwe overlaps pack_key"):
        be.pack(ct, key, 4, 5, out=key[n - 1, 4])
    # nothing above launched anything; count = 0 is a no-op
    assert pack(cnt=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert np.array_equal(arena.cpu().numpy(), held) and np.array_equal(key.cpu().numpy(), held_key)
    assert pack() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), keygen.pack(ct.cpu().numpy(), key.cpu().numpy(), 4, 5))
    # the Python layer: a key of another set or another n is refused, and a bare tensor needs its digit shape
    sk = client.SecretKeySet.from_secret("default128", *keygen.secret_keys("default128", KEY_SEED, n))
    with pytest.raises(ValueError, match="default128"):
        be.pack(ct, sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED))
    sk = client.SecretKeySet.from_secret("redsec_small_v2", *keygen.secret_keys("redsec_small_v2", KEY_SEED, n + 1))
    with pytest.raises(ValueError, match="n = 17"):
        be.pack(ct, sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED))
    with pytest.raises(ValueError, match="explicit basebit"):
        be.pack(ct, key)
    with pytest.raises(ValueError):
        be.pack(ct, key, 4, 9)
