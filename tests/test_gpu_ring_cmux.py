"""Encrypted selection on the device (rs_ring_cmux_dev, rs_ring_lookup_dev): word-for-word equality with
the numpy restatement on every ring, ciphertext count, digit shape, stride and null d1 at which the kernels take another path, guard
words, invalid arguments, and the end to end uses: a row of a plaintext table on redsec_small_v2 under an encrypted index, and one
of two packed NAND results of a default-128 secret under an encrypted bit."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

MASK_SEED = bytes(range(160, 192))
NOISE_SEED = bytes(range(41, 73))
PACK_MASK_SEED = bytes(range(60, 92))
PACK_NOISE_SEED = bytes(range(120, 152))
KEY_SEED = bytes(range(9, 41))
GUARD = 0x5A5A5A5A
RING_SETS = {1024: "redsec_small_v2", 2048: None, 4096: "redsec_medium", 8192: "redsec_large"}
SHAPES = [(1, 1), (8, 3), (4, 6), (2, 12), (5, 6), (1, 31)]

_BACKENDS = {}


def _backend(N):
    """One small-n context per ring: the calls need no loaded key, and the ring is the context's."""
    import redsec_amd
    if N not in _BACKENDS:
        p = redsec_amd.params(RING_SETS[N] or "default128", n=16)
        # N = 2048 is a ring no shipped set has: rs_create takes any N in {1024, 2048, 4096, 8192} with k = 1 whatever the gadget
        # and keyswitch shape beside it (tests/test_gpu_ring_rekey.py builds its N = 2048 context the same way), and the calls read
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


def _seeds(k):
    return [bytes((b + 43 * k + 17 * q) & 0xFF for b in range(32)) for q in range(2)]


def _extreme(rng, R, N, basebit, l):
    """Random ciphertext pairs whose first and last differences d1 - d0 are the extreme words and 2^32 - off, which wraps x + off to 0."""
    d0, d1 = _words(rng, R, 2, N), _words(rng, R, 2, N)
    off = keygen.ring_cmux_offset(basebit, l)
    ext = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, (1 << 32) - off, ((1 << 32) - off - 1) & 0xFFFFFFFF, off], np.uint64).astype(np.uint32)
    for poly in range(2):
        d1[:, poly, :ext.size] = (_u32(d0[:, poly, :ext.size]) + ext).view(np.int32)
        d1[0, poly, -ext.size:] = (_u32(d0[0, poly, -ext.size:]) + ext).view(np.int32)
    return d1, d0


def _check_ring_cmux(N, R, basebit, l, stride=1, null_d1=False, side_stream=False):
    """Random words for the selector (equality of the sums needs no real one); a ciphertext of guard words on either side of the
    output; a second call into the same buffer."""
    import torch
    be = _backend(N)
    rng = np.random.default_rng(N + 7 * R + 100 * basebit + l + 1000 * stride + null_d1)
    rows = (R - 1) * stride + 1
    d1, d0 = _extreme(rng, rows, N, basebit, l)
    sel = _words(rng, 2 * l, 2, N)
    want = keygen.ring_cmux(None if null_d1 else d1[::stride], d0[::stride], sel, basebit, l)
    guard = be.empty(R + 2, 2, N).fill_(GUARD)
    out = guard[1:R + 1]
    t1, t0, tsel = None if null_d1 else _dev(d1), _dev(d0), _dev(sel)
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                           # a non-default stream, the consumer ordered behind it
            got = be.ring_cmux(t1, t0, tsel, basebit, l, stride=stride, out=out)
            twice = got * 2
        s.synchronize()
        assert np.array_equal(_u32(twice.cpu().numpy()), _u32(want) * np.uint32(2))
    else:
        got = be.ring_cmux(t1, t0, tsel, basebit, l, stride=stride, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (R, 2, N)
    h = got.cpu().numpy()
    assert np.array_equal(h, want), (N, R, basebit, l, stride, null_d1, np.argwhere(h != want)[:4].tolist())
    be.ring_cmux(t1, t0, tsel, basebit, l, stride=stride, out=out)           # a second call initialises again: the same words
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((guard[0] == GUARD).all()) and bool((guard[R + 1] == GUARD).all())
    assert np.array_equal(t0.cpu().numpy(), d0) and np.array_equal(tsel.cpu().numpy(), sel)
    assert null_d1 or np.array_equal(t1.cpu().numpy(), d1)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_ring_cmux_words_equal_numpy_at_n_1024(R):
    """(4, 6): 48 workgroups a ciphertext; R = 3 also on a side stream with a dependent consumer."""
    _check_ring_cmux(1024, R, 4, 6)
    if R == 3:
        _check_ring_cmux(1024, R, 4, 6, side_stream=True)


@pytest.mark.parametrize("N", [2048, 4096, 8192])
def test_ring_cmux_words_equal_numpy_on_the_larger_rings(N):
    """(8, 3) at R = 1: N = 2048 is the first ring whose source coefficients fall into two blocks and whose windows start inside
    (-p, p); N = 8192 has 16 tiles x 2 polynomials x 8 source blocks x 6 rows."""
    _check_ring_cmux(N, 1, 8, 3)


@pytest.mark.parametrize("basebit,l", SHAPES)
def test_ring_cmux_words_equal_numpy_for_every_digit_shape(basebit, l):
    _check_ring_cmux(1024, 1, basebit, l)


def test_ring_cmux_words_equal_numpy_with_a_null_d1():
    _check_ring_cmux(1024, 2, 4, 6, null_d1=True)
    _check_ring_cmux(2048, 1, 8, 3, null_d1=True)


def test_ring_cmux_words_equal_numpy_at_stride_two():
    """Rows 0, 2, 4 of five; and the even and odd entries of one table, d1 = d0 + one row."""
    _check_ring_cmux(1024, 3, 4, 6, stride=2)
    _check_ring_cmux(1024, 2, 4, 6, stride=2, null_d1=True)
    be = _backend(1024)
    rng = np.random.default_rng(77)
    table, sel = _words(rng, 6, 2, 1024), _words(rng, 6, 2, 1024)
    dev = _dev(table)
    got = be.ring_cmux(dev[1:], dev, _dev(sel), 8, 3, stride=2)
    assert np.array_equal(got.cpu().numpy(), keygen.ring_cmux(table[1::2], table[0::2], sel, 8, 3))


@pytest.mark.parametrize("entries", [5, 8])
def test_ring_lookup_words_equal_numpy(entries):
    """Depth 3 with random words for table and selectors: 5 entries take the unpaired launch at levels 0 and 1 and one row against
    zero; 8 entries are the full tree. Guard words behind out."""
    N, basebit, l = 1024, 4, 6
    be = _backend(N)
    rng = np.random.default_rng(entries)
    table, sel = _words(rng, entries, 2, N), _words(rng, 3, 2 * l, 2, N)
    guard = be.empty(3, 2, N).fill_(GUARD)
    got = be.ring_lookup(_dev(table), _dev(sel), basebit, l, out=guard[1])
    assert np.array_equal(got.cpu().numpy(), keygen.ring_lookup(table, sel, basebit, l))
    assert bool((guard[0] == GUARD).all()) and bool((guard[2] == GUARD).all())


def test_ring_cmux_invalid_arguments_and_the_empty_batch():
    import torch
    N, R = 1024, 2
    be = _backend(N)
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    sel, d0, d1 = _dev(_words(rng, 3, 12, 2, N)), _dev(_words(rng, R, 2, N)), _dev(_words(rng, R, 2, N))
    out = be.empty(R, 2, N).fill_(7)
    scratch = be.empty(2, 2, N)
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())

    def call(o=P(out), a=P(d1), b=P(d0), r=R, stride=1, s=P(sel), basebit=4, l=6):
        return L.rs_ring_cmux_dev(be.h, o, a, b, r, stride, s, basebit, l, None)

    def look(o=P(out), tb=P(d0), entries=2, s=P(sel), depth=2, basebit=4, l=6, sc=P(scratch)):
        return L.rs_ring_lookup_dev(be.h, o, tb, entries, s, depth, basebit, l, sc, None)
    assert call(o=None) == -1 and call(b=None) == -1 and call(s=None) == -1 and b"null pointer" in L.rs_last_error()
    assert look(o=None) == -1 and look(tb=None) == -1 and look(s=None) == -1 and b"null pointer" in L.rs_last_error()
    for f in (call, look):
        for bad in (0, 9, -1):
            assert f(basebit=bad, l=1) == -1 and b"outside 1 .. 8" in L.rs_last_error()
        for bad in (0, -3):
            assert f(l=bad) == -1 and b"below 1" in L.rs_last_error()
        for basebit, l in ((4, 8), (8, 4), (1, 32), (2, 16), (8, 5)):
            assert f(basebit=basebit, l=l) == -1 and b"passes 31 bits" in L.rs_last_error()
    assert call(stride=0) == -1 and b"stride = 0" in L.rs_last_error()
    assert call(r=1 << 62) == -1 and b"too large" in L.rs_last_error()
    assert call(r=(1 << 64) - 1) == -1 and b"too large" in L.rs_last_error()
    assert call(r=2, stride=(1 << 63)) == -1 and b"too large" in L.rs_last_error()
    assert call(r=1 << 40) == -1 and b"too large for one launch" in L.rs_last_error()    # fits the address space, not one launch
    for bad in (0, -1, 31):
        assert look(depth=bad) == -1 and b"depth" in L.rs_last_error() and b"outside 1 .. 30" in L.rs_last_error()
    for entries, depth in ((0, 2), (5, 2), (3, 1), ((1 << 64) - 1, 30)):
        assert look(entries=entries, depth=depth) == -1 and b"entries" in L.rs_last_error()
    assert look(sc=None) == -1 and b"null scratch" in L.rs_last_error()
    assert look(entries=1 << 30, depth=30) == -1 and b"too large for one launch" in L.rs_last_error()
    # an out that shares a byte with an input is refused: the kernels add into it with atomics after an init kernel has set it to
    # d0, so out = d0 is not offered. Every range named below lies inside one allocation of eight ciphertexts, the selectors (36)
    # or the scratch
    arena = _dev(_words(rng, 8, 2, N))
    held, held_sel = arena.cpu().numpy(), sel.cpu().numpy()
    A, S, ct = arena.data_ptr(), sel.data_ptr(), 8 * N
    for o in (A, A + ct, A + 2 * ct - 4):                                     # out == d0, one ciphertext into it, on its last word
        assert call(o=vp(o), b=vp(A)) == -1 and b"out overlaps d0" in L.rs_last_error()
        assert call(o=vp(o), a=vp(A)) == -1 and b"out overlaps d1" in L.rs_last_error()
        assert call(o=vp(o), a=None, b=vp(A)) == -1 and b"out overlaps d0" in L.rs_last_error()
    assert call(o=vp(A), b=vp(A + 2 * ct - 4)) == -1 and b"out overlaps d0" in L.rs_last_error()      # out's last word is d0's first
    # rows 0 and 2 at stride 2 are read from three ciphertexts, d0 from the arena's rows 0 .. 2 and d1 from its rows 3 .. 5: an out
    # that touches only the third of either is refused (an out behind it is accepted: below)
    assert call(o=vp(A + 2 * ct), b=vp(A), a=vp(A + 4 * ct), stride=2) == -1 and b"out overlaps d0" in L.rs_last_error()
    assert call(o=vp(A + 5 * ct), b=vp(A), a=vp(A + 3 * ct), stride=2) == -1 and b"out overlaps d1" in L.rs_last_error()
    for o in (S, S + 11 * ct, S + 12 * ct - 4):                               # out on the first and the last row of the selector
        assert call(o=vp(o)) == -1 and b"out overlaps sel" in L.rs_last_error()
    assert look(o=vp(A), tb=vp(A)) == -1 and b"out overlaps table" in L.rs_last_error()
    assert look(o=vp(A + ct), tb=vp(A)) == -1 and b"out overlaps table" in L.rs_last_error()
    assert look(o=vp(S + 23 * ct)) == -1 and b"out overlaps sel" in L.rs_last_error()               # the last row of selector 1
    assert look(o=P(scratch)) == -1 and b"out overlaps scratch" in L.rs_last_error()
    assert look(o=vp(scratch.data_ptr() + ct)) == -1 and b"out overlaps scratch" in L.rs_last_error()
    assert look(sc=vp(A + ct), tb=vp(A)) == -1 and b"scratch overlaps table" in L.rs_last_error()
    assert look(sc=vp(S + 22 * ct)) == -1 and b"scratch overlaps sel" in L.rs_last_error()
    with pytest.raises(ValueError, match="out overlaps d0"):
        be.ring_cmux(d1, arena[:2], sel[0], 4, 6, out=arena[:2])
    with pytest.raises(ValueError, match="out overlaps d0"):
        be.ring_cmux(d1, arena[:2], sel[0], 4, 6, out=arena[1:3])
    with pytest.raises(ValueError, match="out overlaps d1"):
        be.ring_cmux(arena[:2], d0, sel[0], 4, 6, out=arena[1:3])
    with pytest.raises(ValueError, match="out overlaps sel"):
        be.ring_cmux(d1, d0, sel[0], 4, 6, out=sel[0, 10:])
    with pytest.raises(ValueError, match="out overlaps table"):
        be.ring_lookup(arena[:4], sel[:2], 4, 6, out=arena[3])
    with pytest.raises(ValueError, match="out overlaps sel"):
        be.ring_lookup(arena[:4], sel[:2], 4, 6, out=sel[1, 11])
    # nothing above launched anything; R = 0 is a no-op
    assert call(r=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert np.array_equal(arena.cpu().numpy(), held) and np.array_equal(sel.cpu().numpy(), held_sel)
    # inputs may overlap each other, and an out that begins where the strided rows end is accepted: rows 0 and 2 of the arena
    # against rows 1 and 3, into rows 4 and 5
    assert call(o=vp(A + 4 * ct), a=vp(A + ct), b=vp(A), stride=2) == 0
    torch.cuda.synchronize()
    assert np.array_equal(arena[4:6].cpu().numpy(), keygen.ring_cmux(held[1:4:2], held[0:4:2], held_sel[0], 4, 6))
    assert np.array_equal(arena[:4].cpu().numpy(), held[:4]) and np.array_equal(arena[6:].cpu().numpy(), held[6:])
    assert call() == 0
    torch.cuda.synchronize()
    h_sel = sel.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), keygen.ring_cmux(d1.cpu().numpy(), d0.cpu().numpy(), h_sel[0], 4, 6))
    assert look(depth=1, sc=None) == 0                                        # depth 1 needs no scratch
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), keygen.ring_lookup(d0.cpu().numpy(), h_sel[:1], 4, 6))
    with pytest.raises(ValueError, match="explicit basebit"):
        be.ring_cmux(d1, d0, sel[0])
    with pytest.raises(ValueError):
        be.ring_cmux(d1, d0, sel[0], 4, 8)
    with pytest.raises(ValueError, match="stride"):
        be.ring_cmux(d1, d0, sel[0], 4, 6, stride=0)
    with pytest.raises(ValueError, match="entries"):
        be.ring_lookup(_dev(_words(rng, 3, 2, N)), sel[:1].contiguous(), 4, 6)
    other = client.SecretKeySet.from_secret("redsec_medium", *keygen.secret_keys("redsec_medium", KEY_SEED))
    big = other.ring_selector(1, 1, 8, 1, MASK_SEED, NOISE_SEED, stdev=2.0 ** -31)
    with pytest.raises(ValueError, match="N = 4096"):
        be.ring_cmux(d1, d0, big)
    with pytest.raises(ValueError, match="N = 4096"):
        be.upload_ring_selector(big)


def test_a_table_row_under_an_encrypted_index_on_redsec_small_v2():
    """Eight trivial rows of random 1/4096-scale integers and a real seeded selector (the set's default shape and deviation) for
    each index 0 .. 7: the words of the numpy restatement, and decrypt_packed_ints returns that row's N values, every error inside
    8 ring_cmux_sigma."""
    import redsec_amd
    import torch
    name, N, depth = "redsec_small_v2", 1024, 3
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    sk = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, KEY_SEED))
    basebit, l = keygen.ring_cmux_default(name, depth)
    sigma = keygen.ring_cmux_sigma(N, basebit, l, keygen.rlwe_default_stdev(name), depth)
    assert 8 * sigma <= 1 / 8192
    values = np.random.default_rng(8).integers(-2047, 2048, (8, N))
    table = keygen.ring_trivial((values << 20).astype(np.int32))
    dev = _dev(table)
    for index in range(8):
        s = _seeds(index)
        sel = sk.ring_selector(index, depth, mask_seed=s[0], noise_seed=s[1])
        assert (sel.basebit, sel.l) == (basebit, l)
        out = be.ring_lookup(dev, sel)
        assert tuple(out.shape) == (2, N)
        if index in (0, 5):
            assert np.array_equal(out.cpu().numpy(), keygen.ring_lookup(table, sel.expand(), basebit, l))
        assert np.array_equal(sk.decrypt_packed_ints(out.reshape(1, 2, N), N, backend=be), values[index]), index
        err = (_u32(sk.packed_phase(out.reshape(1, 2, N), N, backend=be)) - _u32(table[index, 1])).view(np.int32) / 2.0 ** 32
        assert np.abs(err).max() < 8 * sigma, (index, np.abs(err).max() / sigma)
    be.close()
    torch.cuda.empty_cache()


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


def test_default128_one_of_two_packed_nand_results_under_an_encrypted_bit(default128):
    """Two packed ciphertexts of 1,024 NAND results each from Backend.pack, ring_cmux under a real selector of 0 and of 1:
    decrypt_packed_bits gives the chosen one, every phase within 8 ring_cmux_sigma of the chosen ciphertext's."""
    be, sk = default128
    pack_key = sk.packing_key(mask_seed=PACK_MASK_SEED, noise_seed=PACK_NOISE_SEED, backend=be)
    rng = np.random.default_rng(31)
    x, y = rng.integers(0, 2, 2048), rng.integers(0, 2, 2048)
    ct = _dev(sk.encrypt_bits(np.concatenate([x, y]), seed=3))
    nand = be.gate("NAND", ct[:2048].contiguous(), ct[2048:].contiguous())
    want = (1 - (x & y)).reshape(2, 1024)
    packed = be.pack(nand, pack_key)
    assert tuple(packed.shape) == (2, 2, 1024) and not np.array_equal(want[0], want[1])
    before = sk.packed_phase(packed, 2048, backend=be).reshape(2, 1024)
    basebit, l = keygen.ring_cmux_default("default128")
    sigma = keygen.ring_cmux_sigma(1024, basebit, l, keygen.rlwe_default_stdev("default128"))
    for bit in (0, 1):
        s = _seeds(bit)
        sel = sk.ring_selector(bit, 1, mask_seed=s[0], noise_seed=s[1])
        assert (sel.basebit, sel.l) == (basebit, l)
        out = be.ring_cmux(packed[1:], packed[:1], sel)
        assert np.array_equal(out.cpu().numpy(), keygen.ring_cmux(packed[1:].cpu().numpy(), packed[:1].cpu().numpy(), sel.expand()[0], basebit, l))
        assert np.array_equal(sk.decrypt_packed_bits(out, 1024, backend=be), want[bit]), bit
        err = (_u32(sk.packed_phase(out, 1024, backend=be)) - _u32(before[bit])).view(np.int32) / 2.0 ** 32
        print("default-128 selector of %d: largest CMUX error %.3g = %.2f sigma (ring_cmux_sigma %.3g)" % (bit, np.abs(err).max(), np.abs(err).max() / sigma, sigma))
        assert np.abs(err).max() < 8 * sigma < 1 / 8192
