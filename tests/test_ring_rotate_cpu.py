"""Encrypted rotation without a GPU (rs_ring_rotate_dev, rs_ring_rotate_alt_dev, rs_ring_heads_dev): the
lane emulator of the kernels against the numpy restatement word for word, the restatement's monomial against a brute-force one, the
phase of the result against the rotated phase under noise-free and noisy selectors of a real secret, defaults, symbols and kernel
budgets."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib
import redsec_amd
from redsec_amd import client, keygen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEY_SEED = bytes(range(9, 41))
NAME, N1 = "redsec_small_v2", 1024
SHAPES = [(1, 1), (8, 3), (4, 6), (1, 31)]
FORMS = ["signed", "alternating"]
SENTINEL = 0x5A5A5A5A


def _exponents(N):
    return [1, 3, 4, 5, 511, 512, 513, N - 1, N, N + 1, 2 * N - 1, 0, 2 * N] + ([1023, 1024, 1025] if N > 1024 else [])


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _secret(name=NAME, seed=KEY_SEED):
    return client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, seed))


def _seeds(k):
    return [bytes((b + 43 * k + 17 * q) & 0xFF for b in range(32)) for q in range(4)]


def _emu():
    E = emu_lib.lib()
    E.rs_emu_ring_rotate.restype = E.rs_emu_ring_rotate_alt.restype = E.rs_emu_ring_heads.restype = None
    sig = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    E.rs_emu_ring_rotate.argtypes = E.rs_emu_ring_rotate_alt.argtypes = sig
    E.rs_emu_ring_heads.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p]
    E.rs_emu_ring_rotate_exponent.argtypes = [C.c_int32, C.c_int, C.c_int]
    E.rs_emu_ring_rotate_source.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return E


def _emu_rotate(rlwe, R, stride, sel, step, basebit, l, digits, per_row):
    """The emulated call with guard rows behind out and scratch; scratch starts from a sentinel and is null at depth 1."""
    E = _emu()
    N, depth = sel.shape[-1], sel.shape[-4]
    out = np.full((R + 1, 2, N), SENTINEL, np.int32)
    scratch = np.full((R + 1, 2, N), SENTINEL, np.int32) if depth > 1 else None
    before = rlwe.copy()
    f = E.rs_emu_ring_rotate_alt if digits == "alternating" else E.rs_emu_ring_rotate
    f(_p(rlwe), R, stride, N, _p(sel), depth, int(per_row), step, basebit, l, _p(scratch), _p(out))
    assert (out[R] == SENTINEL).all() and (scratch is None or (scratch[R] == SENTINEL).all())
    assert np.array_equal(rlwe, before)
    return out[:R]


def _extreme_row(rng, N, e, basebit, l):
    """A random ciphertext [2][N] whose differences (X^e v)_c - v_c at the first and last coefficients are the extreme words of the
    CMUX tests' _extreme (0, +-2^31 and its neighbours, 2^32 - off, which wraps x + off to 0, and off), wherever coefficient c and
    the coefficient it is rotated from can be set apart."""
    v = _words(rng, 2, N)
    off = keygen.ring_cmux_offset(basebit, l)
    ext = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, (1 << 32) - off, ((1 << 32) - off - 1) & 0xFFFFFFFF, off]
    s, flip = e % N, (e // N) & 1
    spots = list(range(len(ext))) + list(range(N - len(ext), N))
    for i, c in enumerate(spots):
        src = (c - s) % N
        if src in spots:
            continue
        sign = -1 if flip != (c < s) else 1
        for poly in range(2):
            v[poly, c] = np.array((sign * int(v[poly, src]) - ext[i % len(ext)]) & 0xFFFFFFFF, np.uint64).astype(np.uint32).view(np.int32)
    return v


def test_the_monomial_is_a_negacyclic_shift_and_the_device_index_agrees():
    """ring_monomial against one coefficient at a time in Python integers, and ro_source (the kernel's and the emulator's index)
    against it for every exponent of the list, every coefficient."""
    E = _emu()
    rng = np.random.default_rng(1)
    for N in (16, 1024, 2048):
        v = _words(rng, N)
        for e in _exponents(N) + [-1, -4, -N - 3, 5 * N + 7]:
            want = [0] * N
            for c in range(N):
                k = c + e % (2 * N)
                want[k % N] = (-1) ** (k // N) * int(v[c])
            got = keygen.ring_monomial(v, e)
            assert np.array_equal(got.astype(np.int64) & 0xFFFFFFFF, np.array(want, np.int64) & 0xFFFFFFFF), (N, e)
            neg = C.c_int(0)
            for c in (range(N) if N == 16 else (0, 1, 3, 4, 511, 512, 1023, N - 1)):
                idx = E.rs_emu_ring_rotate_source(N, e % (2 * N), c, C.byref(neg))
                assert 0 <= idx < N and (int(got[c]) - (-1) ** neg.value * int(v[idx])) % (1 << 32) == 0, (N, e, c)
    both = _words(rng, 3, 2, 64)
    assert np.array_equal(keygen.ring_monomial(both, 5)[1, 0], keygen.ring_monomial(both[1, 0], 5))
    assert np.array_equal(keygen.ring_monomial(keygen.ring_monomial(both, 70), -70), both)
    for step, k in ((-1, 0), (-1, 29), (3, 7), (-(1 << 31), 29), ((1 << 31) - 1, 29), (513, 2)):
        assert E.rs_emu_ring_rotate_exponent(step, k, 1024) == (step << k) % 2048


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("N,basebit,l", [(1024, 4, 6), (2048, 8, 3)])
def test_one_level_at_every_listed_exponent_equals_numpy(N, basebit, l, digits):
    """Depth 1 with step = e: the sign, the wrap, the 4-word thread boundary, the tile boundary and, at N = 2048, a rotated word
    that comes from the other source block; extreme differences at both ends of the polynomials."""
    rng = np.random.default_rng(N + l)
    sel = _words(rng, 1, 2 * l, 2, N)
    for e in _exponents(N):
        v = _extreme_row(rng, N, e, basebit, l)[None]
        want = keygen.ring_rotate(v, sel, e, basebit, l, digits)
        assert np.array_equal(_emu_rotate(v, 1, 1, sel, e, basebit, l, digits, False), want), e
        if e % (2 * N) == 0:
            assert np.array_equal(want, v)


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("depth", [3, 4])
def test_chains_equal_numpy_for_every_stride_and_selector_layout(depth, digits):
    """Odd and even depth (the parity of the ping-pong), steps whose exponents wrap, and step = N / 2, whose levels 2 and 3 have
    exponent zero; R in {1, 3}, stride in {0, 1, 2}, one selector set for all rows and one per row."""
    N, basebit, l = N1, 8, 3
    rng = np.random.default_rng(depth)
    rows = _words(rng, 5, 2, N)
    sets = _words(rng, 3, depth, 2 * l, 2, N)
    for step in (-1, -4, 3, N // 2 + 1, N // 2):
        for R, stride, per_row in ((1, 1, 0), (3, 0, 1), (3, 1, 1), (3, 2, 0), (3, 2, 1), (3, 0, 0), (1, 0, 1)):
            sel = np.ascontiguousarray(sets[:R] if per_row else sets[0])
            src = rows[:(R - 1) * stride + 1]
            want = keygen.ring_rotate(src, sel, step, basebit, l, digits, per_row=bool(per_row), stride=stride)
            if stride == 0 and not per_row:
                want = np.repeat(want, R, axis=0)
            assert want.shape == (R, 2, N)
            assert np.array_equal(_emu_rotate(src, R, stride, sel, step, basebit, l, digits, per_row), want), (step, R, stride, per_row)


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("basebit,l", SHAPES)
def test_every_digit_shape_equals_numpy(basebit, l, digits):
    rng = np.random.default_rng(10 * basebit + l)
    sel = _words(rng, 2, 2 * l, 2, N1)
    v = _extreme_row(rng, N1, 2 * N1 - 1, basebit, l)[None]
    assert np.array_equal(_emu_rotate(v, 1, 1, sel, -1, basebit, l, digits, False), keygen.ring_rotate(v, sel, -1, basebit, l, digits))


def test_a_second_emulated_call_into_the_same_buffers_gives_the_same_words():
    E = _emu()
    rng = np.random.default_rng(8)
    v, sel = _words(rng, 2, 2, N1), _words(rng, 3, 6, 2, N1)
    out, scratch = np.zeros((2, 2, N1), np.int32), np.zeros((2, 2, N1), np.int32)
    E.rs_emu_ring_rotate(_p(v), 2, 1, N1, _p(sel), 3, 0, -1, 8, 3, _p(scratch), _p(out))
    first = out.copy()
    E.rs_emu_ring_rotate(_p(v), 2, 1, N1, _p(sel), 3, 0, -1, 8, 3, _p(scratch), _p(out))
    assert np.array_equal(out, first) and np.array_equal(first, keygen.ring_rotate(v, sel, -1, 8, 3))


@pytest.mark.parametrize("N,R,width", [(1024, 3, 1), (1024, 3, 4), (1024, 2, 1024), (2048, 1, 3)])
def test_the_emulated_heads_equal_numpy_and_the_extraction_on_shared_slots(N, R, width):
    E = _emu()
    rlwe = _words(np.random.default_rng(N + width), R, 2, N)
    want = keygen.ring_heads(rlwe, width)
    u = np.full((R * width + 1, N + 1), SENTINEL, np.int32)
    E.rs_emu_ring_heads(_p(rlwe), R, width, N, _p(u))
    assert want.shape == (R * width, N + 1) and np.array_equal(u[:-1], want) and (u[-1] == SENTINEL).all()
    for r in range(R):                                                       # slots r N .. r N + width - 1 of rlwe_extract
        assert np.array_equal(want[r * width:(r + 1) * width], keygen.rlwe_extract(rlwe[r:r + 1], width))
    for bad in (0, N + 1):
        with pytest.raises(ValueError):
            keygen.ring_heads(rlwe, bad)


def _rotated_phase_error(sk, out, src, turn):
    """phase(out) - X^turn phase(src) per coefficient, in words."""
    want = keygen.ring_monomial(keygen.rlwe_phase(src, sk.tlwe_key), turn)
    return (_u32(keygen.rlwe_phase(out, sk.tlwe_key)) - _u32(want)).view(np.int32).astype(np.int64)


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("depth,indices,step", [(3, range(8), -1), (3, range(8), 5), (10, (0, 1, 513, 1023), -1)])
def test_noise_free_selectors_of_a_real_secret_rotate_the_phase_up_to_the_rounding(depth, indices, step, digits):
    """Truth, not a restatement: under selectors without noise the phase of the result is X^(step index) times the phase of the
    input, up to the rounding of each level's difference to l basebit bits: half a step on the coefficient's own b word and on each
    of the N/2 a words that meet a set key bit, depth (1 + N/2) 2^(31 - l basebit) words in all (the CMUX tests' bound per level).
    The emulated kernels give the words of the restatement."""
    sk = _secret()
    basebit, l = keygen.ring_cmux_default(NAME, 10)
    assert (basebit, l) == (7, 3)
    rng = np.random.default_rng(depth)
    src = _words(rng, 1, 2, N1)
    bound = depth * (1 + N1 // 2) * (1 << (31 - l * basebit))
    for index in indices:
        s = _seeds(index)
        sel = sk.ring_selector(index, depth, basebit, l, s[0], s[1], stdev=0.0).expand()
        out = keygen.ring_rotate(src, sel, step, basebit, l, digits)
        err = _rotated_phase_error(sk, out, src, step * index)
        print("depth %d index %d %s: largest phase error %d words, bound %d" % (depth, index, digits, np.abs(err).max(), bound))
        assert np.abs(err).max() <= bound
        if depth == 3 or index == 513:
            assert np.array_equal(_emu_rotate(src, 1, 1, sel, step, basebit, l, digits, False), out)


def test_noisy_selectors_at_the_default_shape_meet_the_formula():
    """Ten indices of depth 10 at the default shape and deviation of redsec_small_v2, each on a fresh public-key encryption (a
    trivial row has no mask, so its first levels would carry less than the formula): every error below 8 ring_cmux_sigma(depth =
    10), and the pooled rms within 15 % of the formula (the band of tests/test_ring_cmux_cpu.py and tests/test_pack_cpu.py for the
    same statistic). The rounding term reaches the phase where the level's bit is set, so the expected variance of an index is the
    sum over its levels of ring_cmux_sigma(depth = 1, bit = b_k)^2, the existing formula level by level."""
    sk = _secret()
    depth = 10
    basebit, l = keygen.ring_cmux_default(NAME, depth)
    stdev = keygen.rlwe_default_stdev(NAME)
    sigma = keygen.ring_cmux_sigma(N1, basebit, l, stdev, depth)
    per_bit = [keygen.ring_cmux_sigma(N1, basebit, l, stdev, bit=b) ** 2 for b in (0, 1)]
    pk = sk.rlwe_public_key(*_seeds(77)[:2])
    rng = np.random.default_rng(26)
    errs, expect = [], []
    for index in (0, 1, 2, 341, 512, 513, 682, 1000, 1022, 1023):
        s = _seeds(index)
        mu = (rng.integers(-2047, 2048, N1) << 20).astype(np.int32)
        src = keygen.rlwe_pk_encrypt(pk.expand() if hasattr(pk, "expand") else pk, mu, s[2], stdev=stdev)
        sel = sk.ring_selector(index, depth, basebit, l, s[0], s[1]).expand()
        out = keygen.ring_rotate(src, sel, -1, basebit, l)
        e = _rotated_phase_error(sk, out, src, -index) / 2.0 ** 32
        errs.append(e)
        expect.append(sum(per_bit[(index >> k) & 1] for k in range(depth)))
        assert np.abs(e).max() < 8 * sigma, index
    errs = np.array(errs)
    rms, formula = float(np.sqrt(np.mean(errs * errs))), float(np.sqrt(np.mean(expect)))
    print("(%d, %d) depth %d: sigma %.4g, rms / formula %.3f, largest %.2f sigma" % (basebit, l, depth, sigma, rms / formula, np.abs(errs).max() / sigma))
    assert abs(rms / formula - 1.0) < 0.15
    assert formula <= sigma


def test_the_defaults_give_the_quoted_shapes_and_refuse_default128():
    assert keygen.ring_cmux_default(NAME, 10) == (7, 3)
    for digits in FORMS:                                                     # +-1/8 bits (step 1/4) to depth 13 in both digit forms
        assert len(keygen.circuit_bootstrap_default(NAME, 13, step=1.0 / 4, digits=digits)) == 4
    assert len(keygen.circuit_bootstrap_default(NAME, 13, digits="alternating")) == 4        # step 1/16
    with pytest.raises(ValueError, match="no \\(basebit, l\\)"):
        keygen.ring_cmux_default("default128", 20)
    for digits in FORMS:
        with pytest.raises(ValueError, match="no shape"):
            keygen.circuit_bootstrap_default("default128", 10, step=1.0 / 4, digits=digits)
    z = np.zeros((1, 2, 1024), np.int32)
    with pytest.raises(ValueError):
        keygen.ring_rotate(z, np.zeros((31, 2, 2, 1024), np.int32), -1, 8, 1)
    with pytest.raises(ValueError):
        keygen.ring_rotate(z, np.zeros((1, 2, 2, 1024), np.int32), -1, 8, 4)
    with pytest.raises(ValueError):
        keygen.ring_rotate(z, np.zeros((1, 2, 2, 1024), np.int32), -1, 8, 1, digits="other")


def test_symbols_prototypes_and_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_ring_rotate_dev\(rs_ctx\* ctx, int32_t\* out, const int32_t\* in, size_t R, size_t stride,\s+"
                     r"const int32_t\* sel, int32_t depth, int32_t per_row, int32_t step, int32_t basebit, int32_t l,\s+"
                     r"int32_t\* scratch, void\* stream\);", header)
    assert re.search(r"int rs_ring_rotate_alt_dev\(rs_ctx\* ctx, int32_t\* out, const int32_t\* in, size_t R, size_t stride,", header)
    assert "int rs_ring_heads_dev(rs_ctx* ctx, int32_t* u, const int32_t* rlwe, size_t R, size_t width, void* stream);" in header
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    L = redsec_amd.load_library()
    for sym in ("rs_ring_rotate_dev", "rs_ring_rotate_alt_dev", "rs_ring_heads_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and hasattr(L, sym)
        assert sym in integration, sym
    assert "rs_ring_rotate_dev" in design and "rs_ring_rotate_dev" in readme and "## 26." in integration
    for f in ("ring_rotate", "ring_heads"):
        assert callable(getattr(redsec_amd.Backend, f)) and callable(getattr(keygen, f))
    assert callable(keygen.ring_monomial)
    from redsec_amd import arith
    assert callable(arith.evaluate)
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_ring_rotate", "rs_ring_rotate.hip", [])' in build and build.count('"rs_ring_rotate.h"') == 2
    named = re.findall(r"profiles/r31/[\w./-]*\w", integration + design + open(os.path.join(ROOT, "profiles", "r31", "README.md")).read())
    assert named
    for path in named:
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_failure_without_a_context_matches_ring_cmux():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    rc = L.rs_ring_cmux_dev(None, p, p, p, 1, 1, p, 4, 6, None)
    msg = L.rs_last_error()
    assert rc != 0
    for call in (L.rs_ring_rotate_dev, L.rs_ring_rotate_alt_dev):
        assert call(None, p, p, 1, 1, p, 1, 0, -1, 4, 6, p, None) == rc and L.rs_last_error() == msg
        assert call(None, None, None, 0, 0, None, 0, 0, 0, 0, 0, None, None) == rc and L.rs_last_error() == msg
    assert L.rs_ring_heads_dev(None, p, p, 1, 1, None) == rc and L.rs_last_error() == msg


def test_the_new_kernels_keep_the_budget_of_the_cmux_kernels():
    """No scratch, no static LDS (the 10 KB are dynamic), and no more registers than the CMUX kernels' bound, so the occupancy is
    no lower than theirs."""
    import test_kernel_budgets as kb
    ks = kb._kernels()
    cmux = [k for n, k in ks.items() if "16ring_cmux_kernel" in n or "20ring_cmux_alt_kernel" in n]
    assert len(cmux) == 2
    for pat, vgpr in (("18ring_rotate_kernel", 40), ("22ring_rotate_alt_kernel", 40), ("23ring_rotate_init_kernel", 16), ("17ring_heads_kernel", 16)):
        hit = {n: k for n, k in ks.items() if pat in n}
        assert len(hit) == 1, (pat, sorted(hit))
        for k in hit.values():
            assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= vgpr, (pat, k)


def test_ring_rotate_sources_are_integer_only_and_hold_no_inline_assembly():
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_ring_rotate.h", "rs_ring_rotate.hip"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\b(double|float|half|__fp16|_Float16|asm|__asm__)\b|rs_general\.h|rs_fft\.h|rs_ntt\.h", code), f
