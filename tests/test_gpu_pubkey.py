"""Public-key encryption on the device (rs_pk_encrypt_dev): word-for-word equality with the numpy
restatement over every shape at which the kernel takes another path, the phase identity through rs_phase_dev, a second path made of
kernels that existed before (linear_fc fed the same bits as byte masks, lincomb for mu), invalid arguments, and the end to end use:
operands encrypted under a public key added by arith.add, a NAND against the CPU oracle, a gate output re-randomised in place."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
from redsec_amd import arith, client, keygen

pytestmark = pytest.mark.gpu

RAND_SEED = bytes(range(60, 92))
MASK_SEED = bytes(range(130, 162))
NOISE_SEED = bytes(range(21, 53))
KEY_SEED = bytes(range(9, 41))
E8 = 1 << 29


def _tile():
    L = emu_lib.lib()
    L.rs_emu_pk_tile.argtypes = []
    return L.rs_emu_pk_tile()


_BACKENDS = {}


def _backend(n):
    """One context per LWE dimension for the whole module (the ring and the gadget do not matter here: the call needs no key)."""
    import redsec_amd
    if n not in _BACKENDS:
        _BACKENDS[n] = redsec_amd.Backend(redsec_amd.params("default128" if n == 630 else "redsec_small_v2", n=n), device=0)
    return _BACKENDS[n]


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


def _inputs(n, m, B):
    """Random words: equality of the sums needs no real encryptions, and random rows exercise every bit of every word."""
    rng = np.random.default_rng(1000 * n + 10 * m + B)
    draw = lambda *shape: rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)
    return draw(m, n + 1), draw(B), draw(B, n + 1)


def _check(n, m, B, first, use_mu=True, use_base=False, alias=False):
    import torch
    be = _backend(n)
    pk, mu, base = _inputs(n, m, B)
    want = keygen.pk_encrypt(pk, mu if use_mu else None, RAND_SEED, first, base if use_base else None, B=B)
    d_pk, d_mu, d_base = _dev(pk), _dev(mu) if use_mu else None, _dev(base) if use_base else None
    guard = be.empty(B + 2, n + 1).fill_(0x5A5A5A5A)                       # a row on either side of the output must stay untouched
    out = d_base if alias else guard[1:B + 1]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                              # a non-default stream, the consumer ordered behind it
        got = be.pk_encrypt(d_pk, d_mu, RAND_SEED, first, d_base, out=out)
        twice = be.lincomb(got, 2)
    s.synchronize()
    assert got.data_ptr() == out.data_ptr()
    h = got.cpu().numpy()
    assert np.array_equal(h, want), (n, m, B, first, use_mu, use_base, alias, np.argwhere(h != want)[:4].tolist())
    assert np.array_equal(twice.cpu().numpy().view(np.uint32), want.view(np.uint32) * np.uint32(2))
    assert bool((guard[0] == 0x5A5A5A5A).all()) and bool((guard[B + 1] == 0x5A5A5A5A).all())


@pytest.mark.parametrize("n", [63, 64, 350, 630])
def test_words_equal_numpy_over_the_row_widths(n):
    """W = 64, 65, 351, 631: a full wave, one word over, and ragged last tiles of one and three word tiles."""
    _check(n, 513, 65, 0)


@pytest.mark.parametrize("m", [1, 33, 512, 513, 1100])
def test_words_equal_numpy_over_the_row_counts(m):
    """One row, a ragged group, exactly one chunk, one row over, and two chunks with a ragged third."""
    _check(350, m, 65, 0)


def test_words_equal_numpy_over_the_batch_sizes():
    T = _tile()
    for B in (1, 65, 257, T - 1, T, T + 1, 3 * T + 5):
        _check(350, 513, B, 0)


def test_words_equal_numpy_across_2_to_the_32_in_first():
    for first in (0, (1 << 32) - 3):
        _check(350, 513, 65, first)
    _check(64, 33, 3, (1 << 64) - 3)                                        # the last rows there are


def test_words_equal_numpy_with_and_without_mu_and_base():
    for use_mu, use_base, alias in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 0), (1, 1, 1), (0, 1, 1)):
        _check(350, 513, 65, 0, bool(use_mu), bool(use_base), bool(alias))


def test_words_equal_numpy_in_the_combined_ragged_case():
    _check(630, 1100, 3 * _tile() + 5, (1 << 32) - 3, True, True, True)


def test_phase_identity_through_the_device_phase():
    """Real rows: phase(ct_i) = mu_i + phase(base_i) + the sum of the phases of the selected rows, every phase taken by rs_phase_dev."""
    n, m, B = 350, 1100, 65
    be = _backend(n)
    lwe, tlwe = keygen.secret_keys("redsec_small_v2", KEY_SEED, n)
    sk = client.SecretKeySet.from_secret("redsec_small_v2", lwe, tlwe)
    pk_s = sk.public_key(m, mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    rng = np.random.default_rng(5)
    mu = rng.integers(-(1 << 31), 1 << 31, B, dtype=np.int64)
    base = _dev(sk.encrypt_torus(rng.integers(-(1 << 31), 1 << 31, B, dtype=np.int64), seed=8))
    d_pk = be.expand_ciphertexts(MASK_SEED, _dev(pk_s.body), pk_s.first)
    ct = be.pk_encrypt(pk_s, _dev(mu), RAND_SEED, 7, base)                  # the seeded form of the key is expanded by the call
    assert np.array_equal(ct.cpu().numpy(), be.pk_encrypt(d_pk, _dev(mu), RAND_SEED, 7, base).cpu().numpy())
    ph = lambda x: sk.phase(x, backend=be).astype(np.int64)
    sel = keygen.pk_selection(RAND_SEED, m, 7, B).astype(np.int64)
    want = (sel @ ph(d_pk) + mu + ph(base)) & 0xFFFFFFFF
    assert np.array_equal(ph(ct) & 0xFFFFFFFF, want)
    assert np.abs(ph(d_pk)).max() < 8 * client.SECALPHA * 2 ** 32


def test_words_equal_the_composition_of_earlier_kernels():
    """B = 64, m = 1100: linear_fc with sign = 1 and zero = 1 - bit (a zero tap adds zero_tap_b = 0), then lincomb for mu on the body
    word, gives the same words."""
    import torch
    n, m, B = 350, 1100, 64
    be = _backend(n)
    pk, mu, _ = _inputs(n, m, B)
    sel = keygen.pk_selection(RAND_SEED, m, 5, B)                           # [B][m]
    zero = torch.from_numpy(np.ascontiguousarray(1 - sel.T)).cuda()         # uint8 [K = m][M = B]
    sign = torch.ones_like(zero)
    sums = be.linear_fc(_dev(pk), sign, zero)
    trivial = np.zeros((B, n + 1), np.int32)
    trivial[:, n] = mu
    second = be.lincomb(sums, 1, _dev(trivial), 1)
    got = be.pk_encrypt(_dev(pk), _dev(mu), RAND_SEED, 5)
    assert np.array_equal(got.cpu().numpy(), second.cpu().numpy())


def test_invalid_arguments_and_the_empty_batch():
    import torch
    n, m, B = 64, 40, 5
    be = _backend(n)
    L, vp = be.L, C.c_void_p
    pk, mu, base = (_dev(a) for a in _inputs(n, m, B))
    ct = be.empty(B, n + 1).fill_(7)
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())

    def call(c=P(ct), k=P(pk), rows=m, u=P(mu), b=P(base), count=B, seed=RAND_SEED, first=0):
        return L.rs_pk_encrypt_dev(be.h, c, k, rows, u, b, count, seed, first, None)
    assert call(c=None) == -1 and call(k=None) == -1 and call(seed=None) == -1
    assert b"null pointer" in L.rs_last_error()
    assert call(rows=0) == -1 and call(rows=1 << 31) == -1 and b"2^31" in L.rs_last_error()
    assert call(first=(1 << 64) - B + 1) == -1 and b"2^64" in L.rs_last_error()
    assert call(count=1 << 62) == -1 and b"too large" in L.rs_last_error()  # B (n + 1) 4 bytes passes the address space
    assert call(count=(1 << 64) - 1, first=0) == -1
    # nothing above launched anything; B = 0 is a no-op wherever `first` is
    assert call(count=0) == 0 and call(count=0, first=(1 << 64) - 1) == 0
    torch.cuda.synchronize()
    assert bool((ct == 7).all())
    assert call(first=(1 << 64) - B) == 0 and call(u=None) == 0 and call(b=None) == 0 and call(rows=(1 << 31) - 1, count=0) == 0
    torch.cuda.synchronize()
    want = keygen.pk_encrypt(pk.cpu().numpy(), mu.cpu().numpy(), RAND_SEED, 0)
    assert np.array_equal(ct.cpu().numpy(), want)
    # the Python default is a fresh rand seed per call
    a, b = be.pk_encrypt(pk, mu), be.pk_encrypt(pk, mu)
    assert not np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_end_to_end_adder_nand_and_rerandomisation_under_a_public_key():
    """default-128, key generated on the device. Two 4-bit operands x 8 lanes encrypted under the public key add up (arith.add); a
    NAND of two public-key-encrypted bits equals the CPU oracle's NAND of the same input words; a gate output re-randomised in place
    decrypts as before while its mask words change."""
    import torch
    import oracle_lib as ol
    import redsec_amd
    name = "default128"
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    pk_s = sk.public_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    assert len(pk_s) == keygen.pk_rows(630)
    pk = be.expand_ciphertexts(pk_s.mask_seed, _dev(pk_s.body), pk_s.first)  # what a party without the secret holds
    bits, lanes = 4, 8
    rng = np.random.default_rng(11)
    x, y = rng.integers(0, 1 << bits, lanes), rng.integers(0, 1 << bits, lanes)
    slices = lambda v: np.array([(v >> i) & 1 for i in range(bits)]).ravel()                     # [bits][lanes], LSB first
    a = be.pk_encrypt_bits(pk, slices(x), RAND_SEED, 0).view(bits, lanes, be.W)
    b = be.pk_encrypt_bits(pk, slices(y), RAND_SEED, bits * lanes).view(bits, lanes, be.W)
    assert np.array_equal(sk.decrypt_bits(a.cpu().numpy()), slices(x))
    total = arith.add(be, a, b)
    got = sk.decrypt_bits(total.reshape(-1, be.W).cpu().numpy()).reshape(bits + 1, lanes)
    assert np.array_equal((got << np.arange(bits + 1)[:, None]).sum(axis=0), x + y)

    fa, fb = a.reshape(-1, be.W).contiguous(), b.reshape(-1, be.W).contiguous()
    nand = be.gate("NAND", fa, fb)

    class K:
        pass
    ks = K()
    ks.p, ks.bk, ks.ksk = ol.params(name), bk.cpu().numpy().ravel(), ksk.cpu().numpy().ravel()
    ctx = ol.Ctx(ks)
    ref = ctx.gate_batch("NAND", fa.cpu().numpy(), fb.cpu().numpy())
    ctx.close()
    before = nand.cpu().numpy()
    assert np.array_equal(before, ref)
    assert np.array_equal(sk.decrypt_bits(before), 1 - (slices(x) & slices(y)))

    again = be.pk_encrypt(pk, None, RAND_SEED, 2 * bits * lanes, base=nand, out=nand)           # in place
    after = again.cpu().numpy()
    assert again.data_ptr() == nand.data_ptr()
    assert np.array_equal(sk.decrypt_bits(after), sk.decrypt_bits(before))
    assert np.mean(after[:, :630] == before[:, :630]) < 0.01
    del bk, ksk, pk, a, b, total, nand, again
    be.close()
    torch.cuda.empty_cache()
