"""Circuit bootstrapping on the device (rs_ring_selector_dev, rs_circuit_bootstrap_dev): word-for-word
equality of the selector keyswitch with the numpy restatement on every ring, source dimension, row count and digit shape at which
the kernel takes another path, guard rows, invalid arguments, and the end to end uses on redsec_small_v2 with keys generated on the
device: table[a + b] for two encrypted integers, and one of two packed results under a bit the server computed with a gate."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import arith, client, keygen

pytestmark = pytest.mark.gpu

MASK_SEED = bytes(range(170, 202))
NOISE_SEED = bytes(range(51, 83))
PACK_MASK_SEED = bytes(range(60, 92))
PACK_NOISE_SEED = bytes(range(120, 152))
KEY_SEED = bytes(range(19, 51))
GUARD = 0x5A5A5A5A
RING_SETS = {1024: "redsec_small_v2", 2048: None, 4096: "redsec_medium", 8192: "redsec_large"}
KS_SHAPES = [(8, 4), (1, 1), (4, 6), (2, 12)]                  # (ks_basebit, ks_t); (8, 4) has off = 0
NAME = "redsec_small_v2"

_BACKENDS = {}


def _backend(N):
    """One small-n context per ring: the keyswitch needs no loaded key, the ring is the context's and n_src is an argument."""
    import redsec_amd
    if N not in _BACKENDS:
        p = redsec_amd.params(RING_SETS[N] or "default128", n=16)
        p.N = N                                                  # N = 2048 is a ring no shipped set has (tests/test_gpu_ring_cmux.py)
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


def _extreme(rng, rows, n_src, basebit, l, ks_basebit, ks_t):
    """Random samples whose first and last coordinates x_i (the b word before its half step is added) are the extreme words and
    2^32 - off, which wraps x + off to 0."""
    ct = _words(rng, rows, n_src + 1)
    off = 0 if ks_basebit * ks_t >= 32 else 1 << (31 - ks_basebit * ks_t)
    ext = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, ((1 << 32) - off) & 0xFFFFFFFF], np.uint64).astype(np.uint32)
    for r in range(rows):
        half = 1 << (31 - (r % l + 1) * basebit)
        ct[r, 0] = ext[r % ext.size].view(np.int32)
        ct[r, n_src] = np.uint32((int(ext[(r + 2) % ext.size]) - half) & 0xFFFFFFFF).view(np.int32)
    return ct


def _check(N, n_src, depth, basebit, l, ks_basebit, ks_t, side_stream=False):
    """Random words for the key (equality of the sums needs no real one); a selector of guard words on either side of the output; a
    second call into the same buffer."""
    import torch
    be = _backend(N)
    rng = np.random.default_rng(N + 7 * n_src + 100 * depth + l + 1000 * ks_t)
    rows = depth * l
    ct = _extreme(rng, rows, n_src, basebit, l, ks_basebit, ks_t)
    key = _words(rng, 2, n_src + 1, ks_t, 2, N)
    want = keygen.ring_selector_switch(ct, basebit, l, key, ks_basebit, ks_t)
    guard = be.empty(depth + 2, 2 * l, 2, N).fill_(GUARD)
    out = guard[1:depth + 1]
    tct, tkey = _dev(ct), _dev(key)
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                           # a non-default stream, the consumer ordered behind it
            got = be.ring_selector(tct, basebit, l, tkey, ks_basebit, ks_t, out=out)
            twice = got * 2
        s.synchronize()
        assert np.array_equal(_u32(twice.cpu().numpy()), _u32(want) * np.uint32(2))
    else:
        got = be.ring_selector(tct, basebit, l, tkey, ks_basebit, ks_t, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (depth, 2 * l, 2, N)
    h = got.cpu().numpy()
    assert np.array_equal(h, want), (N, n_src, depth, basebit, l, ks_basebit, ks_t, np.argwhere(h != want)[:4].tolist())
    be.ring_selector(tct, basebit, l, tkey, ks_basebit, ks_t, out=out)       # a second call initialises again: the same words
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((guard[0] == GUARD).all()) and bool((guard[depth + 1] == GUARD).all())
    assert np.array_equal(tct.cpu().numpy(), ct) and np.array_equal(tkey.cpu().numpy(), key)


@pytest.mark.parametrize("n_src", [6, 7, 8, 21])
def test_selector_words_equal_numpy_around_the_coordinate_chunk(n_src):
    """n_src + 1 coordinates one below, at and one past the chunk of eight, and 22 = two chunks and six; nine rows = one register
    block and one row of the next. n_src = 8 also on a side stream with a dependent consumer."""
    _check(1024, n_src, 3, 3, 3, 4, 6)
    if n_src == 8:
        _check(1024, n_src, 3, 3, 3, 4, 6, side_stream=True)


@pytest.mark.parametrize("depth,l", [(1, 1), (4, 2), (3, 3), (2, 9)])
def test_selector_words_equal_numpy_around_the_register_block(depth, l):
    """rows = depth l: 1, one register block of eight, one block + 1, and 18 = two blocks and two"""
    _check(1024, 13, depth, 3, l, 4, 6)


@pytest.mark.parametrize("N", [2048, 4096, 8192])
def test_selector_words_equal_numpy_on_the_larger_rings(N):
    """four to sixteen tiles a polynomial, both families and polynomials, two chunks, nine rows"""
    _check(N, 9, 3, 3, 3, 8, 4)


@pytest.mark.parametrize("ks_basebit,ks_t", KS_SHAPES)
def test_selector_words_equal_numpy_for_every_digit_shape(ks_basebit, ks_t):
    _check(1024, 10, 2, 1, 31, ks_basebit, ks_t)
    _check(1024, 10, 1, 8, 3, ks_basebit, ks_t)


def test_selector_invalid_arguments_and_the_empty_call():
    import torch
    N, n_src, depth, l, ks_t = 1024, 10, 2, 3, 6
    be = _backend(N)
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    ct, key = _dev(_words(rng, depth * l, n_src + 1)), _dev(_words(rng, 2, n_src + 1, ks_t, 2, N))
    bits = _dev(_words(rng, depth, be.W))
    out = be.empty(depth, 2 * l, 2, N).fill_(7)
    scratch = be.empty(l * N + depth * l * (2 * be.W + 1))
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())

    def call(o=P(out), c=P(ct), d=depth, basebit=4, l=l, n=n_src, k=P(key), kb=4, kt=ks_t):
        return L.rs_ring_selector_dev(be.h, o, c, d, basebit, l, n, k, kb, kt, None)

    def boot(o=P(out), c=P(bits), d=depth, basebit=4, l=l, k=P(key), kb=4, kt=ks_t, sc=P(scratch)):
        return L.rs_circuit_bootstrap_dev(be.h, o, c, d, basebit, l, k, kb, kt, sc, None)
    assert boot() == -4 and b"rs_load_keys" in L.rs_last_error()             # RS_ERR_STATE: this context has no evaluation key
    assert call(o=None) == -1 and call(c=None) == -1 and call(k=None) == -1 and b"null pointer" in L.rs_last_error()
    for bad in (0, 9, -1):
        assert call(basebit=bad, l=1) == -1 and b"basebit" in L.rs_last_error() and b"outside 1 .. 8" in L.rs_last_error()
        assert call(kb=bad, kt=1) == -1 and b"ks_basebit" in L.rs_last_error() and b"outside 1 .. 8" in L.rs_last_error()
    for bad in (0, -3):
        assert call(l=bad) == -1 and b"l = " in L.rs_last_error() and b"below 1" in L.rs_last_error()
        assert call(kt=bad) == -1 and b"ks_t = " in L.rs_last_error() and b"below 1" in L.rs_last_error()
    for basebit, ll in ((4, 8), (8, 4), (1, 32)):
        assert call(basebit=basebit, l=ll) == -1 and b"passes 31 bits" in L.rs_last_error()
    for kb, kt in ((4, 9), (8, 5), (1, 33)):
        assert call(kb=kb, kt=kt) == -1 and b"passes 32 bits" in L.rs_last_error()
    for bad in (-1, 31):
        assert call(d=bad) == -1 and b"depth" in L.rs_last_error() and b"outside 0 .. 30" in L.rs_last_error()
    for bad in (0, -1, 65537):
        assert call(n=bad) == -1 and b"n_src" in L.rs_last_error() and b"outside 1 .. 65536" in L.rs_last_error()
    assert call(k=vp(key.data_ptr() + 4)) == -1 and b"16-byte aligned" in L.rs_last_error()
    # a sel that shares a byte with an input is refused: the kernels add into it with atomics after an init kernel has zeroed it.
    # Every range named below lies inside one allocation of sixteen ring samples (sel is twelve) or inside the key (132)
    arena = _dev(_words(rng, 16, 2, N))
    held, held_key = arena.cpu().numpy(), key.cpu().numpy()
    A, K, row, ring = arena.data_ptr(), key.data_ptr(), 4 * (n_src + 1), 8 * N
    for o in (A, A + row, A + depth * l * row - 4):                           # sel == ct, one sample into ct, on its last word
        assert call(o=vp(o), c=vp(A)) == -1 and b"sel overlaps ct" in L.rs_last_error()
    assert call(o=vp(A), c=vp(A + 12 * ring - 4)) == -1 and b"sel overlaps ct" in L.rs_last_error()   # sel's last word is ct's first
    for o in (K, K + ring, K + 120 * ring):                                   # sel on the key's first, second and last twelve samples
        assert call(o=vp(o)) == -1 and b"sel overlaps sel_key" in L.rs_last_error()
    with pytest.raises(ValueError, match="sel overlaps ct"):
        be.ring_selector(arena.view(-1)[:depth * l * (n_src + 1)].view(depth * l, n_src + 1), 4, l, key, 4, ks_t, out=arena[:12])
    with pytest.raises(ValueError, match="sel overlaps sel_key"):
        be.ring_selector(ct, 4, l, key, 4, ks_t, out=key.view(-1, 2, N)[120:])
    # nothing above launched anything; depth = 0 is a no-op
    assert call(d=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert np.array_equal(arena.cpu().numpy(), held) and np.array_equal(key.cpu().numpy(), held_key)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), keygen.ring_selector_switch(ct.cpu().numpy(), 4, l, key.cpu().numpy(), 4, ks_t))
    with pytest.raises(ValueError, match="explicit ks_basebit"):
        be.ring_selector(ct, 4, l, key)
    with pytest.raises(ValueError):
        be.ring_selector(ct, 4, 8, key, 4, ks_t)
    with pytest.raises(ValueError):
        be.ring_selector(ct, 4, l, key, 4, 9)
    other = client.SecretKeySet.from_secret("redsec_medium", *keygen.secret_keys("redsec_medium", KEY_SEED, n=n_src))
    big = other.selector_key(8, 1, MASK_SEED, NOISE_SEED, stdev=2.0 ** -31)
    with pytest.raises(ValueError, match="N = 4096"):
        be.upload_selector_key(big)
    # the composed call refuses the same overlaps and those of its scratch (3,282 words here). It looks at them behind the check
    # for a loaded key, so the context gets one of random words; nothing below launches anything else
    be.load_synthetic_keys(5)
    key16 = _dev(_words(rng, 2, be.W, ks_t, 2, N))                           # a key of the context's n = 16
    out.fill_(7)
    torch.cuda.synchronize()
    words = scratch.numel()
    assert words == l * N + depth * l * (2 * be.W + 1)
    for o in (A, A + 4 * be.W, A + 4 * (depth * be.W - 1)):                   # sel == bits, one bit into them, on their last word
        assert boot(o=vp(o), c=vp(A), k=P(key16)) == -1 and b"sel overlaps bits" in L.rs_last_error()
    assert boot(o=P(key16), k=P(key16)) == -1 and b"sel overlaps sel_key" in L.rs_last_error()
    assert boot(o=vp(A), sc=vp(A), k=P(key16)) == -1 and b"sel overlaps scratch" in L.rs_last_error()
    assert boot(o=vp(A), sc=vp(A + 12 * ring - 4), k=P(key16)) == -1 and b"sel overlaps scratch" in L.rs_last_error()   # sel's last word
    assert boot(o=vp(A + 4 * (words - 1)), sc=vp(A), k=P(key16)) == -1 and b"sel overlaps scratch" in L.rs_last_error()  # scratch's last word
    assert boot(c=vp(A + 4 * (words - 1)), sc=vp(A), k=P(key16)) == -1 and b"scratch overlaps bits" in L.rs_last_error()
    assert boot(sc=P(key16), k=P(key16)) == -1 and b"scratch overlaps sel_key" in L.rs_last_error()
    with pytest.raises(ValueError, match="sel overlaps bits"):
        be.circuit_bootstrap(arena.view(-1)[:depth * be.W].view(depth, be.W), 4, l, key16, 4, ks_t, out=arena[:12])
    with pytest.raises(ValueError, match="sel overlaps sel_key"):
        be.circuit_bootstrap(bits, 4, l, key16, 4, ks_t, out=key16.view(-1, 2, N)[:12])
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and np.array_equal(arena.cpu().numpy(), held)


@pytest.fixture(scope="module")
def small_v2():
    """redsec_small_v2 with keys generated on the device, and ONE selector key at the default's (ks_basebit, ks_t), uploaded once"""
    import redsec_amd
    import torch
    be = redsec_amd.Backend(redsec_amd.params(NAME), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    shape = keygen.circuit_bootstrap_default(NAME)
    key = sk.selector_key(shape[2], shape[3], MASK_SEED, NOISE_SEED)
    yield be, sk, shape, key, be.upload_selector_key(key)
    be.close()
    torch.cuda.empty_cache()


def _sixteenths(sk, be, out, N):
    phase = sk.packed_phase(out.reshape(1, 2, N), N, backend=be).reshape(N)
    return phase, ((_u32(phase).astype(np.int64) + (1 << 27)) >> 28) & 15


def test_table_of_a_plus_b_without_a_round_trip(small_v2):
    """Two 2-bit encrypted integers in sixteen lanes, every (a, b): arith.add, the three sum bits of a lane through
    circuit_bootstrap, ring_lookup over eight plaintext rows of 1/16-step values; the decrypted row is table[a + b] and every slot
    lies within 8 sigma of its coefficient (circuit_bootstrap_sigma at depth 3). The shape is the default of the set, which
    keeps 8 sigma of the worst coefficient inside 1/32 for ONE CMUX; at depth 3 the formula gives the two end coefficients
    2^-7.3, so 1/32 is 4.9 sigma there (the first level, over plaintext rows, spends less), and the default refuses depth 3 at
    this step: INTEGRATION.md section 24. The first lane's selectors are also held word for word against the separate calls."""
    be, sk, (basebit, l, ks_basebit, ks_t), key, dkey = small_v2
    N, n = be.p.N, be.p.n
    pairs = [(a, b) for a in range(4) for b in range(4)]
    bits = lambda v: np.array([[(x >> k) & 1 for x in v] for k in range(2)])                 # [bit][lane]
    ea = _dev(sk.encrypt_bits(bits([a for a, _ in pairs]).ravel(), seed=5)).reshape(2, 16, n + 1)
    eb = _dev(sk.encrypt_bits(bits([b for _, b in pairs]).ravel(), seed=6)).reshape(2, 16, n + 1)
    total = arith.add(be, ea, eb)                                                           # [3][16][n+1]
    assert tuple(total.shape) == (3, 16, n + 1)
    values = np.random.default_rng(8).integers(0, 16, (8, N))
    table = _dev(keygen.ring_trivial((values << 28).astype(np.uint32).view(np.int32)))
    sigma = keygen.circuit_bootstrap_sigma(N, n, basebit, l, ks_basebit, ks_t, keygen.bootstrap_sigma(NAME),
                                           keygen.ring_selector_default_stdev(NAME), depth=3, coefficient=np.arange(N))
    worst = 0.0
    for lane, (a, b) in enumerate(pairs):
        index_bits = total[:, lane].contiguous()
        out = arith.lookup(be, index_bits, table, dkey, basebit, l, ks_basebit, ks_t)
        phase, got = _sixteenths(sk, be, out, N)
        err = (_u32(phase) - _u32(values[a + b] << 28)).view(np.int32) / 2.0 ** 32
        worst = max(worst, float(np.abs(err / sigma).max()))
        assert np.array_equal(got, values[a + b]), (a, b, np.flatnonzero(got != values[a + b])[:8].tolist())
        assert (np.abs(err) < 8 * sigma).all(), (a, b, float(np.abs(err / sigma).max()))
        if lane == 0:
            rep = be.gather_rows(index_bits, _dev(np.repeat(np.arange(3), l)))
            lut = _dev(np.repeat(np.array([1 << (31 - (j + 1) * basebit) for j in range(l)], np.int32)[:, None], N, axis=1))
            level = be.bootstrap_lut(rep, lut)
            apart = be.ring_selector(level, basebit, l, dkey, ks_basebit, ks_t)
            assert np.array_equal(apart.cpu().numpy(), be.circuit_bootstrap(index_bits, basebit, l, key).cpu().numpy())
            assert np.array_equal(apart.cpu().numpy(), keygen.ring_selector_switch(level.cpu().numpy(), basebit, l, key.expand(), ks_basebit, ks_t))
    print("table[a + b]: worst |error| / sigma_c over 16 lookups: %.2f" % worst)


def test_one_of_two_packed_results_under_a_bit_the_server_computed(small_v2):
    """Two packed ciphertexts of 1,024 NAND results each, the selecting bit an AND the server computed with rs_gate_dev from two
    encrypted bits: decrypt_packed_bits gives the chosen ciphertext, every phase within 8 sigma of the chosen one's. Bits at +-1/8
    are payloads of step 1/4: the shape is the default's for that step."""
    be, sk, _, key, dkey = small_v2
    N, n = be.p.N, be.p.n
    basebit, l, ks_basebit, ks_t = keygen.circuit_bootstrap_default(NAME, 1, step=1 / 4)
    assert (ks_basebit, ks_t) == (key.ks_basebit, key.ks_t)
    pack_key = sk.packing_key(mask_seed=PACK_MASK_SEED, noise_seed=PACK_NOISE_SEED, backend=be)
    rng = np.random.default_rng(31)
    x, y = rng.integers(0, 2, 2 * N), rng.integers(0, 2, 2 * N)
    ct = _dev(sk.encrypt_bits(np.concatenate([x, y]), seed=3))
    packed = be.pack(be.gate("NAND", ct[:2 * N].contiguous(), ct[2 * N:].contiguous()), pack_key)
    want = (1 - (x & y)).reshape(2, N)
    before = sk.packed_phase(packed, 2 * N, backend=be).reshape(2, N)
    sigma = keygen.circuit_bootstrap_sigma(N, n, basebit, l, ks_basebit, ks_t, keygen.bootstrap_sigma(NAME),
                                           keygen.ring_selector_default_stdev(NAME), coefficient=np.arange(N))
    assert 8 * sigma.max() <= 1 / 8
    for u, v in ((1, 1), (1, 0), (0, 0)):
        uv = _dev(sk.encrypt_bits(np.array([u, v]), seed=7 + u + 2 * v))
        bit = be.gate("AND", uv[:1].contiguous(), uv[1:].contiguous())
        sel = be.circuit_bootstrap(bit, basebit, l, dkey, ks_basebit, ks_t)
        out = be.ring_cmux(packed[1:], packed[:1], sel[0], basebit, l)
        assert np.array_equal(sk.decrypt_packed_bits(out, N, backend=be), want[u & v]), (u, v)
        err = (_u32(sk.packed_phase(out, N, backend=be)) - _u32(before[u & v])).view(np.int32) / 2.0 ** 32
        print("AND(%d, %d): largest CMUX error %.2f sigma_c" % (u, v, np.abs(err / sigma).max()))
        assert (np.abs(err) < 8 * sigma).all()
