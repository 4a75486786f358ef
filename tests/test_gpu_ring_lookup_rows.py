"""Batched encrypted lookup on the device (rs_ring_lookup_rows_dev, rs_ring_lookup_rows_alt_dev):
word-for-word equality through the C ABI with rs_ring_lookup_dev / rs_ring_lookup_alt_dev called once per row on a contiguous copy
of that row's table (and with the numpy restatement at N = 1024) for every shape, stride pair, digit form and selector layout of the
CPU list and on the larger rings, guard ciphertexts, a side stream, every refusal, Backend.ring_lookup_rows, and the end-to-end
uses on redsec_small_v2: arith.lookup_rows, and arith.evaluate against the route it replaces."""
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
CASES = [(3, 5, 3), (2, 1, 2), (2, 8, 3), (3, 6, 4), (1, 3, 2)]               # (R, entries, depth), the list of the CPU tests
EXTREMES = [0, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, 1]

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


def _strides(R, E):
    return [(0, 1), (E, 1), (1, R), (E + 1, 1)]


def _held(R, E, row_stride, entry_stride):
    return (R - 1) * row_stride + (E - 1) * entry_stride + 1


def _scratch_rows(R, E):
    first = -(-E // 2)
    return R * (first + -(-first // 2))


def _table(rng, cts, N):
    """Random ciphertexts whose first and last words are the extreme words, turned by one place from one ciphertext to the next."""
    t = _words(rng, cts, 2, N)
    n = len(EXTREMES)
    for c in range(cts):
        ends = np.array([EXTREMES[(i + c) % n] for i in range(n)], np.uint32).view(np.int32)
        t[c, :, :n] = ends
        t[c, :, -n:] = ends
    return t


def _P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rows_call(be, digits):
    return be.L.rs_ring_lookup_rows_alt_dev if digits == "alternating" else be.L.rs_ring_lookup_rows_dev


class _Case:
    """Device inputs and guarded targets of one (N, R, E, depth, l): a ciphertext of guard words on either side of out and scratch."""

    def __init__(self, N, R, E, depth, l, seed):
        self.be = _backend(N)
        rng = np.random.default_rng(seed)
        self.N, self.R, self.E, self.depth, self.l = N, R, E, depth, l
        self.sets = _words(rng, R, depth, 2 * l, 2, N)
        self.table = _table(rng, max(_held(R, E, rs, es) for rs, es in _strides(R, E)), N)
        self.t_sets, self.t_table = _dev(self.sets), _dev(self.table)
        self.t_first = self.t_sets[0].contiguous()
        rows = _scratch_rows(R, E)
        self.g_out = self.be.empty(R + 2, 2, N).fill_(GUARD)
        self.g_scratch = self.be.empty(rows + 2, 2, N).fill_(GUARD)
        self.out, self.scratch = self.g_out[1:R + 1], self.g_scratch[1:rows + 1]
        self.single = {}

    def call(self, row_stride, entry_stride, per_row, basebit, digits, stream=None):
        f = _rows_call(self.be, digits)
        rc = f(self.be.h, _P(self.out), _P(self.t_table), self.E, row_stride, entry_stride, self.R, _P(self.t_sets if per_row else self.t_first),
               self.depth, per_row, basebit, self.l, _P(self.scratch) if self.depth > 1 else None, stream)
        assert rc == 0, self.be.L.rs_last_error()

    def want(self, row_stride, entry_stride, per_row, basebit, digits, numpy_too):
        """rs_ring_lookup_dev / _alt_dev once per row on a contiguous copy of that row's table (Backend.ring_lookup is that call with
        its scratch allocated), remembered by (entries read, selector set, digit form); with numpy_too also the restatement."""
        out = np.zeros((self.R, 2, self.N), np.int32)
        for q in range(self.R):
            idx = [q * row_stride + e * entry_stride for e in range(self.E)]
            s = q if per_row else 0
            key = (tuple(idx), s, basebit, digits)
            if key not in self.single:
                rows = self.t_table[idx].contiguous()
                got = self.be.ring_lookup(rows, self.t_sets[s], basebit, self.l, digits=digits).cpu().numpy()
                if numpy_too:
                    assert np.array_equal(got, keygen.ring_lookup_rows(self.table[idx], self.sets[s], basebit, self.l, self.E, 1, digits=digits)[0])
                self.single[key] = got
            out[q] = self.single[key]
        return out

    def check(self, row_stride, entry_stride, per_row, basebit, digits, numpy_too=False):
        import torch
        want = self.want(row_stride, entry_stride, per_row, basebit, digits, numpy_too)
        self.call(row_stride, entry_stride, per_row, basebit, digits)
        torch.cuda.synchronize()
        got = self.out.cpu().numpy()
        assert np.array_equal(got, want), (self.N, self.R, self.E, row_stride, entry_stride, per_row, digits, np.argwhere(got != want)[:4].tolist())
        kept = self.scratch.clone()
        self.call(row_stride, entry_stride, per_row, basebit, digits)         # every level initialises again: the same words
        torch.cuda.synchronize()
        assert np.array_equal(self.out.cpu().numpy(), want) and bool((self.scratch == kept).all())
        for g in (self.g_out, self.g_scratch):
            assert bool((g[0] == GUARD).all()) and bool((g[-1] == GUARD).all())
        assert np.array_equal(self.t_table.cpu().numpy(), self.table) and np.array_equal(self.t_sets.cpu().numpy(), self.sets)


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("R,E,depth", CASES)
def test_every_stride_pair_and_selector_layout_equals_the_single_lookups_and_numpy_at_n_1024(R, E, depth, digits):
    case = _Case(1024, R, E, depth, 3, 100 * R + 10 * E + depth)
    for row_stride, entry_stride in _strides(R, E):
        for per_row in (0, 1):
            case.check(row_stride, entry_stride, per_row, 8, digits, numpy_too=True)


@pytest.mark.parametrize("N", [2048, 4096, 8192])
def test_the_larger_rings_equal_the_single_lookups(N):
    case = _Case(N, 2, 3, 2, 3, N)
    case.check(3, 1, 1, 8, "signed")
    case.check(1, 2, 0, 8, "alternating")


def test_depth_one_leaves_scratch_alone_and_takes_a_null_one():
    import torch
    case = _Case(1024, 3, 2, 1, 6, 41)
    case.check(2, 1, 1, 4, "signed", numpy_too=True)
    case.check(0, 1, 1, 4, "alternating")
    assert bool((case.g_scratch == GUARD).all())
    one = _Case(1024, 2, 1, 1, 6, 42)                                         # a single entry at depth 1: the d1-less case for every row
    one.check(1, 1, 1, 4, "signed", numpy_too=True)
    torch.cuda.synchronize()


def test_a_call_on_a_side_stream_with_a_dependent_consumer():
    import torch
    case = _Case(1024, 3, 5, 3, 6, 5)
    want = case.want(5, 1, 1, 4, "signed", False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        case.call(5, 1, 1, 4, "signed", stream=C.c_void_p(s.cuda_stream))
        twice = case.out * 2
    s.synchronize()
    assert np.array_equal(_u32(twice.cpu().numpy()), _u32(want) * np.uint32(2))
    assert np.array_equal(case.out.cpu().numpy(), want)


def test_invalid_arguments_the_empty_batch_and_adjacent_buffers():
    import torch
    N, R, E, depth = 1024, 2, 3, 2
    be = _backend(N)
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    sel, table = _dev(_words(rng, R, depth, 12, 2, N)), _dev(_words(rng, 6, 2, N))
    out = be.empty(R, 2, N).fill_(7)
    rows = _scratch_rows(R, E)                                                # 2 (2 + 1) = 6
    scratch = be.empty(rows + 2, 2, N).fill_(9)[1:rows + 1]
    torch.cuda.synchronize()
    INVALID = -1

    def call(f=L.rs_ring_lookup_rows_dev, o=_P(out), t=_P(table), entries=E, rs=E, es=1, r=R, s=_P(sel), depth=depth, per_row=1, basebit=4, l=6,
             sc=_P(scratch)):
        return f(be.h, o, t, entries, rs, es, r, s, depth, per_row, basebit, l, sc, None)

    def text():
        return L.rs_last_error()
    for f in (L.rs_ring_lookup_rows_dev, L.rs_ring_lookup_rows_alt_dev):
        assert call(f, o=None) == INVALID and call(f, t=None) == INVALID and call(f, s=None) == INVALID and b"null pointer" in text()
        for bad in (0, 9, -1):
            assert call(f, basebit=bad, l=1) == INVALID and b"outside 1 .. 8" in text()
        for bad in (0, -3):
            assert call(f, l=bad) == INVALID and b"below 1" in text()
        for basebit, l in ((4, 8), (8, 4), (1, 32)):
            assert call(f, basebit=basebit, l=l) == INVALID and b"passes 31 bits" in text()
        for bad in (0, -1, 31):
            assert call(f, depth=bad) == INVALID and b"depth" in text() and b"outside 1 .. 30" in text()
        for bad in (0, 5, 1 << 40):
            assert call(f, entries=bad) == INVALID and b"entries = " in text() and b"outside 1 .. 2^2" in text()
        assert call(f, es=0) == INVALID and text() == b"entry_stride = 0"
        assert call(f, sc=None) == INVALID and b"null scratch with depth = 2" in text()
        # row arithmetic: the read extent, the selector sets, the scratch; then the launch
        assert call(f, rs=1 << 63) == INVALID and b"too large for ciphertexts" in text()
        assert call(f, r=3, rs=1 << 63) == INVALID and b"too large for ciphertexts" in text()             # (R - 1) row_stride wraps to 0
        assert call(f, es=1 << 62) == INVALID and b"too large for ciphertexts" in text()
        assert call(f, rs=0, es=(1 << 63) + 1) == INVALID and b"too large for ciphertexts" in text()       # (E - 1) entry_stride wraps to 2
        assert call(f, r=(1 << 64) - 1, rs=1) == INVALID and b"too large for ciphertexts" in text()
        assert call(f, r=1 << 62, rs=0) == INVALID and b"too large for selector sets" in text()
        assert call(f, r=1 << 50, rs=0, per_row=0) == INVALID and b"too large for a scratch" in text()
        assert call(f, r=1 << 40, rs=0, per_row=0) == INVALID and b"too large for one launch" in text()
        assert call(f, r=1 << 27, rs=0, per_row=0) == INVALID and b"too large for one launch" in text()    # 2^27 x 2 pairs x 48 workgroups
    # overlaps: every range below lies inside the arena of sixteen ciphertexts, the selectors (2 x 2 x 12 rows) or the scratch
    arena = _dev(_words(rng, 16, 2, N))
    held = arena.cpu().numpy()
    A, S, ct = arena.data_ptr(), sel.data_ptr(), 8 * N
    for o in (A, A + 5 * ct, A + 6 * ct - 4):                                 # two tables of three at row stride 3: ciphertexts 0 .. 5
        assert call(o=vp(o), t=vp(A)) == INVALID and b"out overlaps table" in text()
    assert call(o=vp(A), t=vp(A + 2 * ct - 4)) == INVALID and b"out overlaps table" in text()
    assert call(o=vp(A + 5 * ct), t=vp(A), rs=1, es=2) == INVALID and b"out overlaps table" in text()      # 0, 2, 4 and 1, 3, 5
    assert call(o=vp(A + 2 * ct), t=vp(A), rs=0) == INVALID and b"out overlaps table" in text()            # one shared table 0 .. 2
    for o in (S, S + 23 * ct, S + 46 * ct):                                   # inside the two sets of 24 ciphertexts each
        assert call(o=vp(o)) == INVALID and b"out overlaps sel" in text()
    assert call(o=vp(S + 23 * ct), per_row=0) == INVALID and b"out overlaps sel" in text()
    assert call(o=_P(scratch)) == INVALID and b"out overlaps scratch" in text()
    assert call(o=vp(scratch.data_ptr() + rows * ct - 4)) == INVALID and b"out overlaps scratch" in text()
    assert call(sc=vp(A + 5 * ct), t=vp(A)) == INVALID and b"scratch overlaps table" in text()
    assert call(sc=vp(S + 42 * ct)) == INVALID and b"scratch overlaps sel" in text()                   # the last six ciphertexts of sel
    # R = 0 is a no-op, and nothing above launched anything
    assert call(r=0) == 0 and call(L.rs_ring_lookup_rows_alt_dev, r=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((scratch == 9).all())
    assert np.array_equal(arena.cpu().numpy(), held)
    # accepted: an out that begins where the strided tables end and a scratch behind it (tables 0 .. 5, out 6 .. 7, scratch 8 .. 13);
    # an out at the unread second selector set with one set for all rows; depth 1 with a null scratch
    h_table, h_sel = table.cpu().numpy(), sel.cpu().numpy()
    assert call(o=vp(A + 6 * ct), t=vp(A), sc=vp(A + 8 * ct)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(arena[6:8].cpu().numpy(), keygen.ring_lookup_rows(held[:6], h_sel, 4, 6, E, R, E, 1))
    assert np.array_equal(arena[:6].cpu().numpy(), held[:6]) and np.array_equal(arena[14:].cpu().numpy(), held[14:])
    assert call(depth=1, entries=2, rs=2, sc=None) == 0
    torch.cuda.synchronize()
    # with depth 1 a row's set is one sample: rows 0 and 1 read the first two samples of the selector tensor
    assert np.array_equal(out.cpu().numpy(), keygen.ring_lookup_rows(h_table, h_sel[0].reshape(R, 1, 12, 2, N), 4, 6, 2, R, 2, 1))
    assert bool((scratch == 9).all())


def test_backend_ring_lookup_rows_defaults_and_refusals():
    import torch
    N, R, E, depth = 1024, 2, 3, 2
    be = _backend(N)
    rng = np.random.default_rng(2)
    h_sel, h_table = _words(rng, R, depth, 12, 2, N), _words(rng, 6, 2, N)
    sel, table = _dev(h_sel), _dev(h_table)
    # per_row and R from a 5-D tensor, entries from a shared table
    got = be.ring_lookup_rows(table[:E], sel, basebit=4, l=6)
    assert tuple(got.shape) == (R, 2, N)
    assert np.array_equal(got.cpu().numpy(), keygen.ring_lookup_rows(h_table[:E], h_sel, 4, 6, E, R))
    # one set for all rows, R tables one after another, the alternating form, into `out`
    out = be.empty(R, 2, N)
    back = be.ring_lookup_rows(table, sel[1], E, R, E, 1, basebit=4, l=6, out=out, digits="alternating")
    assert back.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), keygen.ring_lookup_rows(h_table, h_sel[1], 4, 6, E, R, E, 1, digits="alternating"))
    for q in range(R):
        assert np.array_equal(out[q].cpu().numpy(), be.ring_lookup(table[q * E:(q + 1) * E], sel[1], 4, 6, digits="alternating").cpu().numpy())
    # entries R ciphertexts wide
    wide = be.ring_lookup_rows(table, sel, E, R, 1, R, basebit=4, l=6)
    assert np.array_equal(wide.cpu().numpy(), keygen.ring_lookup_rows(h_table, h_sel, 4, 6, E, R, 1, R))
    assert tuple(be.ring_lookup_rows(table[:E], sel[:0], basebit=4, l=6).shape) == (0, 2, N)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="out overlaps table"):
        be.ring_lookup_rows(table, sel, E, R, E, 1, basebit=4, l=6, out=table[4:6])
    with pytest.raises(ValueError, match="out overlaps sel"):
        be.ring_lookup_rows(table[:E], sel, basebit=4, l=6, out=sel[1, 1, 8:10])
    with pytest.raises(ValueError, match="explicit basebit"):
        be.ring_lookup_rows(table[:E], sel)
    with pytest.raises(ValueError):
        be.ring_lookup_rows(table[:E], sel, basebit=4, l=8)
    with pytest.raises(ValueError, match="digit form"):
        be.ring_lookup_rows(table[:E], sel, basebit=4, l=6, digits="other")
    with pytest.raises(ValueError, match="entry_stride"):
        be.ring_lookup_rows(table, sel, E, R, E, 0, basebit=4, l=6)
    with pytest.raises(ValueError, match="row_stride"):
        be.ring_lookup_rows(table, sel, E, R, -1, 1, basebit=4, l=6)
    with pytest.raises(ValueError, match="entries must be given"):
        be.ring_lookup_rows(table, sel, None, R, E, 1, basebit=4, l=6)
    with pytest.raises(ValueError, match="entries = 5"):
        be.ring_lookup_rows(table[:5], sel, basebit=4, l=6)
    with pytest.raises(ValueError, match="the strides read"):
        be.ring_lookup_rows(table, sel, E, R, E + 1, 1, basebit=4, l=6)
    with pytest.raises(ValueError, match="selector sets"):
        be.ring_lookup_rows(table[:E], sel, R=3, basebit=4, l=6)
    with pytest.raises(ValueError, match="context's ring"):
        be.ring_lookup_rows(table[:E], sel.view(R, depth, 12, 4, N // 2), basebit=4, l=6)
    other = client.SecretKeySet.from_secret("redsec_medium", *keygen.secret_keys("redsec_medium", KEY_SEED))
    with pytest.raises(ValueError, match="N = 4096"):
        be.ring_lookup_rows(table[:2], other.ring_selector(1, 1, 8, 1, MASK_SEED, NOISE_SEED, stdev=2.0 ** -31))


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


def test_lookup_rows_of_bits_the_server_bootstrapped_itself(small_v2):
    """arith.lookup_rows at depth 3, R = 4 over a shared table of eight trivial rows of 1/16-step values (the step the produced
    selectors of tests/test_gpu_ring_selector.py carry; here in the finer alternating shape of depth 10): every row decrypts to
    table[index_r]."""
    be, sk, (basebit, l, ks_basebit, ks_t), dkey, key = small_v2
    N, n, depth = be.p.N, be.p.n, 3
    values = np.random.default_rng(33).integers(0, 16, (1 << depth, N))
    table = _dev(keygen.ring_trivial((values << 28).astype(np.uint32).view(np.int32)))
    indices = [0, 7, 5, 2]
    bits = _index_bits(sk, indices, depth, n, 31)
    out = arith.lookup_rows(be, bits, table, dkey, basebit, l, ks_basebit, ks_t, digits="alternating")
    assert tuple(out.shape) == (len(indices), 2, N)
    phase = sk.packed_phase(out, len(indices) * N, backend=be).reshape(len(indices), N)
    assert np.array_equal(((_u32(phase).astype(np.int64) + (1 << 27)) >> 28) & 15, values[indices])
    again = arith.lookup_rows(be, bits, table, key, basebit, l, digits="alternating")          # the key object carries its ks shape
    assert np.array_equal(again.cpu().numpy(), out.cpu().numpy())


def test_evaluate_of_a_table_of_two_rows_gives_the_words_of_the_route_it_replaces(small_v2):
    """arith.evaluate(digits="alternating") at depth 9, width 4 (512 entries of four words are two table rows of 256), R = 3: word
    for word what the route before the batched lookup gives, restated here from the public calls (circuit_bootstrap_batch, one
    ring_lookup per index, ring_rotate, ring_heads, keyswitch), and every bit decrypts right."""
    be, sk, (basebit, l, ks_basebit, ks_t), dkey, _ = small_v2
    N, n, depth, width = be.p.N, be.p.n, 9, 4
    rng = np.random.default_rng(9)
    table = rng.integers(0, 2, (1 << depth, width))
    values = np.where(table != 0, 1 << 29, -(1 << 29)).astype(np.int32).ravel()
    indices = [511, 256, 255]
    R = len(indices)
    bits = _index_bits(sk, indices, depth, n, 13)
    out = arith.evaluate(be, bits, values, dkey, width, basebit, l, ks_basebit, ks_t, digits="alternating")
    assert tuple(out.shape) == (R * width, n + 1)
    assert np.array_equal(sk.decrypt_bits(out, backend=be).reshape(R, width), table[indices])
    # the old route
    flat = bits.permute(1, 0, 2).contiguous().reshape(R * depth, n + 1)
    sel = be.empty(R, depth, 2 * l, 2, N)
    be.circuit_bootstrap_batch(flat, basebit, l, dkey, ks_basebit, ks_t, out=sel.view(R * depth, 2 * l, 2, N))
    low = 8
    rows = np.zeros((2, 2, N), np.int32)
    rows[:, 1, :] = values.reshape(2, N)
    t_rows = _dev(rows)
    chosen = be.empty(R, 2, N)
    for r in range(R):
        be.ring_lookup(t_rows, sel[r, low:], basebit, l, out=chosen[r], digits="alternating")
    turned = be.ring_rotate(chosen, sel[:, :low].contiguous(), -width, basebit, l, stride=1, per_row=True, digits="alternating")
    want = be.keyswitch(be.ring_heads(turned, width))
    assert np.array_equal(out.cpu().numpy(), want.cpu().numpy())
