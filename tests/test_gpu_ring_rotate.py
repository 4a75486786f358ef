"""Encrypted rotation on the device (rs_ring_rotate_dev, rs_ring_rotate_alt_dev, rs_ring_heads_dev):
word-for-word equality with the numpy restatement through the C ABI on every ring, exponent, depth, digit form, stride and selector
layout at which the kernels take another path, guard ciphertexts, refusals, and the end-to-end uses: arith.evaluate of a table under
bits the server bootstrapped itself on redsec_small_v2, and a packed ciphertext rotated by a client's hidden index."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import arith, client, keygen

pytestmark = pytest.mark.gpu

MASK_SEED = bytes(range(160, 192))
NOISE_SEED = bytes(range(41, 73))
KEY_SEED = bytes(range(9, 41))
GUARD = 0x5A5A5A5A
NAME = "redsec_small_v2"
RING_SETS = {1024: "redsec_small_v2", 2048: None, 4096: "redsec_medium", 8192: "redsec_large"}
FORMS = ["signed", "alternating"]

_BACKENDS = {}


def _backend(N):
    """One small-n context per ring, as tests/test_gpu_ring_cmux.py builds them: the calls need no loaded key and read nothing of a
    context but its N (N = 2048 is a ring no shipped set has)."""
    import redsec_amd
    if N not in _BACKENDS:
        p = redsec_amd.params(RING_SETS[N] or "default128", n=16)
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
    return [bytes((b + 43 * k + 17 * q) & 0xFF for b in range(32)) for q in range(3)]


def _exponents(N):
    return [1, 3, 4, 5, 511, 512, 513, N - 1, N, N + 1, 2 * N - 1, 0, 2 * N]


class _Case:
    """Device inputs and guarded targets of one shape: a ciphertext of guard words on either side of out and of scratch."""

    def __init__(self, N, R, stride, per_row, depth, l, seed):
        self.be = _backend(N)
        rng = np.random.default_rng(seed)
        self.N, self.R, self.stride, self.per_row, self.depth = N, R, stride, per_row, depth
        self.rows = _words(rng, (R - 1) * stride + 1, 2, N)
        self.sel = _words(rng, *(((R,) if per_row else ()) + (depth, 2 * l, 2, N)))
        self.t_rows, self.t_sel = _dev(self.rows), _dev(self.sel)
        self.g_out = self.be.empty(R + 2, 2, N).fill_(GUARD)
        self.g_scratch = self.be.empty(R + 2, 2, N).fill_(GUARD)
        self.out, self.scratch = self.g_out[1:R + 1], self.g_scratch[1:R + 1]

    def want(self, step, basebit, l, digits):
        w = keygen.ring_rotate(self.rows, self.sel, step, basebit, l, digits, per_row=bool(self.per_row), stride=self.stride)
        return np.repeat(w, self.R, axis=0) if self.stride == 0 and not self.per_row else w

    def call(self, step, basebit, l, digits, stream=None):
        L = self.be.L
        f = L.rs_ring_rotate_alt_dev if digits == "alternating" else L.rs_ring_rotate_dev
        P = lambda t: C.c_void_p(t.data_ptr())
        rc = f(self.be.h, P(self.out), P(self.t_rows), self.R, self.stride, P(self.t_sel), self.depth, self.per_row, step, basebit, l,
               P(self.scratch) if self.depth > 1 else None, stream)
        assert rc == 0, L.rs_last_error()

    def check(self, step, basebit, l, digits):
        import torch
        want = self.want(step, basebit, l, digits)
        self.call(step, basebit, l, digits)
        torch.cuda.synchronize()
        got = self.out.cpu().numpy()
        assert np.array_equal(got, want), (self.N, self.R, self.stride, self.per_row, self.depth, step, digits, np.argwhere(got != want)[:4].tolist())
        self.call(step, basebit, l, digits)                                  # every level initialises again: the same words
        torch.cuda.synchronize()
        assert np.array_equal(self.out.cpu().numpy(), want)
        for g in (self.g_out, self.g_scratch):
            assert bool((g[0] == GUARD).all()) and bool((g[self.R + 1] == GUARD).all())
        if self.depth == 1:
            assert bool((self.g_scratch == GUARD).all())                     # depth 1 does not touch scratch
        assert np.array_equal(self.t_rows.cpu().numpy(), self.rows) and np.array_equal(self.t_sel.cpu().numpy(), self.sel)


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("R", [1, 3])
def test_one_level_at_every_listed_exponent_equals_numpy_at_n_1024(R, digits):
    """Depth 1 with step = e through the C ABI: the sign, the wrap, the 4-word thread boundary, the tile boundary, e = 0 and 2N (the
    copy alone). R = 3 takes one selector per row at stride 2."""
    case = _Case(1024, R, 2 if R == 3 else 1, int(R == 3), 1, 3, 100 + R)
    for e in _exponents(1024):
        case.check(e, 8, 3, digits)


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("depth,steps", [(3, (-1, 513)), (4, (-4, 3, 512))])
def test_chains_equal_numpy_for_every_stride_and_selector_layout_at_n_1024(depth, steps, digits):
    """Odd and even depth (the parity of the ping-pong between scratch and out); step = 512 has exponent zero at levels 2 and 3;
    stride 0, 1 and 2 with one selector set for all rows and one per row."""
    for R, stride, per_row in ((1, 1, 0), (1, 0, 1), (3, 0, 1), (3, 1, 1), (3, 2, 0), (3, 0, 0)):
        case = _Case(1024, R, stride, per_row, depth, 3, 10 * depth + R + stride)
        for step in steps:
            case.check(step, 8, 3, digits)


def test_a_chain_on_a_side_stream_with_a_dependent_consumer():
    import torch
    case = _Case(1024, 3, 1, 1, 3, 6, 5)
    want = case.want(-1, 4, 6, "signed")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        case.call(-1, 4, 6, "signed", stream=C.c_void_p(s.cuda_stream))
        twice = case.out * 2
    s.synchronize()
    assert np.array_equal(_u32(twice.cpu().numpy()), _u32(want) * np.uint32(2))
    assert np.array_equal(case.out.cpu().numpy(), want)


@pytest.mark.parametrize("N", [2048, 4096, 8192])
def test_the_larger_rings_equal_numpy(N):
    """R = 1 at (8, 3). One level at e = N + 1025 in the signed form: the rotated word comes from another source block, wraps and
    carries the sign of X^N. One chain of depth 2 at step -1025 in the alternating form."""
    _Case(N, 1, 1, 0, 1, 3, N).check(N + 1025, 8, 3, "signed")
    _Case(N, 1, 1, 0, 2, 3, N + 1).check(-1025, 8, 3, "alternating")


@pytest.mark.parametrize("N,R,width", [(1024, 3, 1), (1024, 3, 4), (1024, 3, 1024), (8192, 1, 3)])
def test_ring_heads_equal_numpy(N, R, width):
    import torch
    be = _backend(N)
    rlwe = _words(np.random.default_rng(N + width), R, 2, N)
    guard = be.empty(R * width + 2, N + 1).fill_(GUARD)
    dev = _dev(rlwe)
    got = be.ring_heads(dev, width, out=guard[1:R * width + 1])
    torch.cuda.synchronize()
    assert tuple(got.shape) == (R * width, N + 1) and np.array_equal(got.cpu().numpy(), keygen.ring_heads(rlwe, width))
    assert bool((guard[0] == GUARD).all()) and bool((guard[R * width + 1] == GUARD).all())
    assert np.array_equal(dev.cpu().numpy(), rlwe)
    assert np.array_equal(be.ring_heads(dev, width).cpu().numpy()[:width], be.rlwe_extract(dev[:1], width).cpu().numpy())


def test_invalid_arguments_the_empty_batch_and_adjacent_buffers():
    import torch
    N, R, depth = 1024, 2, 2
    be = _backend(N)
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    sel, rows = _dev(_words(rng, R, depth, 12, 2, N)), _dev(_words(rng, 3, 2, N))
    out = be.empty(R, 2, N).fill_(7)
    scratch = be.empty(R + 2, 2, N).fill_(9)[1:R + 1]                         # inside its allocation: an out on its last word ends there
    u = be.empty(R * 2, N + 1).fill_(7)
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())
    INVALID = -1

    def call(f=L.rs_ring_rotate_dev, o=P(out), i=P(rows), r=R, stride=1, s=P(sel), depth=depth, per_row=0, step=-1, basebit=4, l=6, sc=P(scratch)):
        return f(be.h, o, i, r, stride, s, depth, per_row, step, basebit, l, sc, None)

    def heads(o=P(u), i=P(rows), r=R, width=2):
        return L.rs_ring_heads_dev(be.h, o, i, r, width, None)
    for f in (L.rs_ring_rotate_dev, L.rs_ring_rotate_alt_dev):
        assert call(f, o=None) == INVALID and call(f, i=None) == INVALID and call(f, s=None) == INVALID and b"null pointer" in L.rs_last_error()
        for bad in (0, 9, -1):
            assert call(f, basebit=bad, l=1) == INVALID and b"outside 1 .. 8" in L.rs_last_error()
        for bad in (0, -3):
            assert call(f, l=bad) == INVALID and b"below 1" in L.rs_last_error()
        for basebit, l in ((4, 8), (8, 4), (1, 32)):
            assert call(f, basebit=basebit, l=l) == INVALID and b"passes 31 bits" in L.rs_last_error()
        for bad in (0, -1, 31):
            assert call(f, depth=bad) == INVALID and b"depth" in L.rs_last_error() and b"outside 1 .. 30" in L.rs_last_error()
        assert call(f, sc=None) == INVALID and b"null scratch with depth = 2" in L.rs_last_error()
        assert call(f, r=1 << 62) == INVALID and b"too large" in L.rs_last_error()
        assert call(f, r=(1 << 64) - 1) == INVALID and b"too large" in L.rs_last_error()
        assert call(f, r=2, stride=1 << 63) == INVALID and b"too large" in L.rs_last_error()
        assert call(f, r=1 << 40) == INVALID and b"too large for one launch" in L.rs_last_error()
    # overlaps: every range below lies inside the arena of eight ciphertexts, the selectors (2 x 2 x 12 rows) or the scratch
    arena = _dev(_words(rng, 8, 2, N))
    held = arena.cpu().numpy()
    A, S, ct = arena.data_ptr(), sel.data_ptr(), 8 * N
    for o in (A, A + ct, A + 2 * ct - 4):
        assert call(o=vp(o), i=vp(A)) == INVALID and b"out overlaps in" in L.rs_last_error()
    assert call(o=vp(A), i=vp(A + 2 * ct - 4)) == INVALID and b"out overlaps in" in L.rs_last_error()
    assert call(o=vp(A + 2 * ct), i=vp(A), stride=2) == INVALID and b"out overlaps in" in L.rs_last_error()       # rows 0 and 2 are read
    assert call(o=vp(A + 2 * ct), i=vp(A + 3 * ct), stride=0) == INVALID and b"out overlaps in" in L.rs_last_error()
    for o in (S, S + 23 * ct, S + 24 * ct - 4):
        assert call(o=vp(o)) == INVALID and b"out overlaps sel" in L.rs_last_error()
    assert call(o=vp(S + 46 * ct), per_row=1) == INVALID and b"out overlaps sel" in L.rs_last_error()             # the end of the second row's set
    assert call(o=P(scratch)) == INVALID and b"out overlaps scratch" in L.rs_last_error()
    assert call(o=vp(scratch.data_ptr() + 2 * ct - 4)) == INVALID and b"out overlaps scratch" in L.rs_last_error()
    assert call(sc=vp(A + ct), i=vp(A)) == INVALID and b"scratch overlaps in" in L.rs_last_error()
    assert call(sc=vp(S + 23 * ct)) == INVALID and b"scratch overlaps sel" in L.rs_last_error()
    assert heads(o=None) == INVALID and heads(i=None) == INVALID and b"null pointer" in L.rs_last_error()
    for bad in (0, N + 1):
        assert heads(width=bad) == INVALID and b"width" in L.rs_last_error()
    assert heads(r=1 << 62) == INVALID and b"too large" in L.rs_last_error()
    assert heads(o=vp(A + ct), i=vp(A)) == INVALID and b"u overlaps rlwe" in L.rs_last_error()
    # R = 0 is a no-op, and nothing above launched anything
    assert call(r=0) == 0 and call(L.rs_ring_rotate_alt_dev, r=0) == 0 and heads(r=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((scratch == 9).all()) and bool((u == 7).all())
    assert np.array_equal(arena.cpu().numpy(), held)
    # accepted: depth 1 with a null scratch; an out that begins where the strided rows end (rows 0 and 2 of the arena into rows 3 and
    # 4, scratch rows 5 and 6); a scratch that an out at an unread selector set follows directly
    h_rows, h_sel = rows.cpu().numpy(), sel.cpu().numpy()
    assert call(depth=1, sc=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), keygen.ring_rotate(h_rows[:2], h_sel[0, :1], -1, 4, 6)) and bool((scratch == 9).all())
    assert call(o=vp(A + 3 * ct), i=vp(A), stride=2, sc=vp(A + 5 * ct)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(arena[3:5].cpu().numpy(), keygen.ring_rotate(held[:3], h_sel[0], -1, 4, 6, stride=2))
    assert np.array_equal(arena[:3].cpu().numpy(), held[:3]) and np.array_equal(arena[7:].cpu().numpy(), held[7:])
    assert heads() == 0
    torch.cuda.synchronize()
    assert np.array_equal(u.cpu().numpy(), keygen.ring_heads(h_rows[:2], 2))
    # the Python refusals
    with pytest.raises(ValueError, match="out overlaps in"):
        be.ring_rotate(arena[:2], sel[0], -1, 4, 6, out=arena[1:3])
    with pytest.raises(ValueError, match="out overlaps sel"):
        be.ring_rotate(rows[:2], sel[0], -1, 4, 6, out=sel[0, 1, 10:])
    with pytest.raises(ValueError, match="u overlaps rlwe"):
        be.ring_heads(arena[:1], 1, out=arena.view(-1)[N:2 * N + 1])
    with pytest.raises(ValueError, match="explicit basebit"):
        be.ring_rotate(rows, sel[0])
    with pytest.raises(ValueError):
        be.ring_rotate(rows, sel[0], -1, 4, 8)
    with pytest.raises(ValueError, match="stride"):
        be.ring_rotate(rows, sel[0], -1, 4, 6, stride=-1)
    with pytest.raises(ValueError, match="digit form"):
        be.ring_rotate(rows, sel[0], -1, 4, 6, digits="other")
    with pytest.raises(ValueError, match="width"):
        be.ring_heads(rows, 0)
    other = client.SecretKeySet.from_secret("redsec_medium", *keygen.secret_keys("redsec_medium", KEY_SEED))
    with pytest.raises(ValueError, match="N = 4096"):
        be.ring_rotate(rows, other.ring_selector(1, 1, 8, 1, MASK_SEED, NOISE_SEED, stdev=2.0 ** -31))
    # per_row is inferred from a 5-D tensor
    got = be.ring_rotate(rows[:2], sel, 3, 4, 6)
    assert np.array_equal(got.cpu().numpy(), keygen.ring_rotate(h_rows[:2], h_sel, 3, 4, 6, per_row=True))


@pytest.fixture(scope="module")
def small_v2():
    """redsec_small_v2 with keys generated on the device, and one selector key of the alternating default's shape at depth 10."""
    import redsec_amd
    import torch
    be = redsec_amd.Backend(redsec_amd.params(NAME), device=0)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    shape = keygen.circuit_bootstrap_default(NAME, 10, digits="alternating")
    key = sk.selector_key(shape[2], shape[3], MASK_SEED, NOISE_SEED)
    yield be, sk, shape, be.upload_selector_key(key), key
    be.close()
    torch.cuda.empty_cache()


def _index_bits(sk, indices, depth, n, seed):
    bits = np.array([[(i >> k) & 1 for i in indices] for k in range(depth)])                  # [bit][index], LSB first
    return _dev(sk.encrypt_bits(bits.ravel(), seed=seed)).reshape(depth, len(indices), n + 1)


def test_a_function_of_ten_encrypted_bits_re_enters_the_gates(small_v2):
    """arith.evaluate(digits="alternating") at depth 10 over a random table of 1,024 values +-1/8 and eight indices, 0 and 1023
    among them, whose bits are real encryptions: every output decrypts to table[index] under the LWE secret, NANDs of the outputs
    in pairs decrypt correctly, and with keyswitch=False every ring phase lies within 8 circuit_bootstrap_sigma(depth = 10) of the
    table value."""
    be, sk, (basebit, l, ks_basebit, ks_t), dkey, key = small_v2
    N, n, depth = be.p.N, be.p.n, 10
    rng = np.random.default_rng(10)
    table = rng.integers(0, 2, 1 << depth)
    values = np.where(table != 0, 1 << 29, -(1 << 29)).astype(np.int32)
    indices = [0, 1023, 1, 513, 682, 341, 1000, 77]
    bits = _index_bits(sk, indices, depth, n, 11)
    out = arith.evaluate(be, bits, values, key, digits="alternating")                          # the default shape, the key's ks shape
    assert tuple(out.shape) == (8, n + 1)
    assert np.array_equal(sk.decrypt_bits(out, backend=be), table[indices])
    nand = be.gate("NAND", out[0::2].contiguous(), out[1::2].contiguous())
    assert np.array_equal(sk.decrypt_bits(nand, backend=be), 1 - (table[indices[0::2]] & table[indices[1::2]]))
    u = arith.evaluate(be, bits, _dev(values), dkey, 1, basebit, l, ks_basebit, ks_t, digits="alternating", keyswitch=False)
    assert tuple(u.shape) == (8, N + 1)
    sigma = keygen.circuit_bootstrap_sigma(N, n, basebit, l, ks_basebit, ks_t, keygen.bootstrap_sigma(NAME),
                                           keygen.ring_selector_default_stdev(NAME), depth=depth, digits="alternating")
    err = (_u32(sk.phase(u, backend=be, ring=True)) - _u32(values[indices])).view(np.int32) / 2.0 ** 32
    print("evaluate depth 10, (%d, %d, %d, %d): rms / formula %.3f, largest error %.2f sigma (sigma %.3g)"
          % (basebit, l, ks_basebit, ks_t, float(np.sqrt(np.mean(err * err))) / sigma, np.abs(err).max() / sigma, sigma))
    assert np.abs(err).max() < 8 * sigma
    # one index alone, [depth][W]
    one = arith.evaluate(be, bits[:, 3].contiguous(), values, dkey, 1, basebit, l, ks_basebit, ks_t, digits="alternating")
    assert tuple(one.shape) == (1, n + 1) and sk.decrypt_bits(one, backend=be)[0] == table[513]
    with pytest.raises(ValueError, match="no shape"):
        arith.evaluate(be, bits, values, dkey, ks_basebit=ks_basebit, ks_t=ks_t)               # the signed default has none at depth 10
    with pytest.raises(ValueError, match="values holds"):
        arith.evaluate(be, bits, values[:-1], dkey, 1, basebit, l, ks_basebit, ks_t, digits="alternating")


def test_four_output_bits_per_index_at_width_four(small_v2):
    """width = 4, depth 8, step -4: 256 entries of four +-1/8 words in one row; four output bits per index, in the shape of the
    depth-10 default (a shorter chain under the same selectors carries less noise)."""
    be, sk, (basebit, l, ks_basebit, ks_t), dkey, _ = small_v2
    n, depth, width = be.p.n, 8, 4
    rng = np.random.default_rng(4)
    table = rng.integers(0, 2, (1 << depth, width))
    values = np.where(table != 0, 1 << 29, -(1 << 29)).astype(np.int32).ravel()
    indices = [0, 255, 1, 128, 170, 85]
    out = arith.evaluate(be, _index_bits(sk, indices, depth, n, 12), values, dkey, width, basebit, l, ks_basebit, ks_t, digits="alternating")
    assert tuple(out.shape) == (len(indices) * width, n + 1)
    assert np.array_equal(sk.decrypt_bits(out, backend=be).reshape(len(indices), width), table[indices])


def test_a_table_longer_than_a_row_takes_the_lookup_for_its_high_bits(small_v2):
    """width = 4, depth 9: 512 entries of four words are two rows of 256; the high bit goes through ring_lookup, the low eight
    rotate."""
    be, sk, (basebit, l, ks_basebit, ks_t), dkey, _ = small_v2
    n, depth, width = be.p.n, 9, 4
    rng = np.random.default_rng(9)
    table = rng.integers(0, 2, (1 << depth, width))
    values = np.where(table != 0, 1 << 29, -(1 << 29)).astype(np.int32).ravel()
    indices = [0, 511, 256, 255]
    out = arith.evaluate(be, _index_bits(sk, indices, depth, n, 13), values, dkey, width, basebit, l, ks_basebit, ks_t, digits="alternating")
    assert np.array_equal(sk.decrypt_bits(out, backend=be).reshape(len(indices), width), table[indices])


def test_a_packed_ciphertext_rotated_by_a_clients_hidden_index(small_v2):
    """One public-key encryption of N 1/4096-scale integers, a client's selector of depth 10 at the set's default shape, step -1:
    decrypt_packed_ints returns the negacyclic rotation, slot `index` at coefficient 0 and the wrapped slots negated; every error
    within 8 ring_cmux_sigma(depth = 10)."""
    be, sk = small_v2[0], small_v2[1]
    N, depth = be.p.N, 10
    basebit, l = keygen.ring_cmux_default(NAME, depth)
    stdev = keygen.rlwe_default_stdev(NAME)
    sigma = keygen.ring_cmux_sigma(N, basebit, l, stdev, depth)
    values = np.random.default_rng(3).integers(-2047, 2048, N)
    pk = sk.rlwe_public_key(*_seeds(5)[:2])
    src = be.rlwe_pk_encrypt(pk, _dev((values << 20).astype(np.int32)), rand_seed=_seeds(5)[2])
    before = sk.packed_phase(src, N, backend=be)
    for index in (0, 1, 513, 1023):
        s = _seeds(index)
        sel = sk.ring_selector(index, depth, mask_seed=s[0], noise_seed=s[1])
        assert (sel.basebit, sel.l) == (basebit, l)
        out = be.ring_rotate(src, sel)
        assert tuple(out.shape) == (1, 2, N)
        want = np.concatenate([values[index:], -values[:index]])
        assert np.array_equal(sk.decrypt_packed_ints(out, N, backend=be), want), index
        err = (_u32(sk.packed_phase(out, N, backend=be)) - _u32(keygen.ring_monomial(before, -index))).view(np.int32) / 2.0 ** 32
        print("index %d: rms %.3f sigma, largest error %.2f sigma (ring_cmux_sigma %.3g)" % (index, float(np.sqrt(np.mean(err * err))) / sigma, np.abs(err).max() / sigma, sigma))
        assert np.abs(err).max() < 8 * sigma
        if index == 513:
            assert np.array_equal(out.cpu().numpy(), keygen.ring_rotate(src.cpu().numpy(), sel.expand(), -1, basebit, l))
