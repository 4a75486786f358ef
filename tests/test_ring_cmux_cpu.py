"""Encrypted selection without a GPU (rs_ring_cmux_dev, rs_ring_lookup_dev): the numpy restatement against
a brute-force product, the lane emulator of the kernels against the numpy restatement, the exact identities of a noise-free
selector, lookups under real selectors, the error of noisy selectors against ring_cmux_sigma, files, refusals, defaults, symbols
and kernel budgets."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import emu_lib
import redsec_amd
from redsec_amd import client, keygen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MASK_SEED = bytes(range(160, 192))
NOISE_SEED = bytes(range(41, 73))
KEY_SEED = bytes(range(9, 41))
SHAPES = [(1, 1), (8, 3), (4, 6), (2, 12), (5, 6), (1, 31)]
NAME, N1 = "redsec_small_v2", 1024


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _secret(name=NAME, seed=KEY_SEED):
    return client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, seed))


def _seeds(k):
    return [bytes((b + 43 * k + 17 * q) & 0xFF for b in range(32)) for q in range(4)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _extreme(rng, R, N, basebit, l):
    """Random ciphertext pairs whose first differences d1 - d0 are the extreme words and 2^32 - off, which wraps x + off to 0."""
    d0, d1 = _words(rng, R, 2, N), _words(rng, R, 2, N)
    off = keygen.ring_cmux_offset(basebit, l)
    ext = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, (1 << 32) - off, ((1 << 32) - off - 1) & 0xFFFFFFFF, off], np.uint64).astype(np.uint32)
    for poly in range(2):
        d1[:, poly, :ext.size] = (_u32(d0[:, poly, :ext.size]) + ext).view(np.int32)
        d1[0, poly, -ext.size:] = (_u32(d0[0, poly, -ext.size:]) + ext).view(np.int32)
    return d1, d0


def _public_selector(m, N, basebit, l):
    """The noise-free public selector: zero masks, rows = m H."""
    sel = np.zeros((2 * l, 2, N), np.int64)
    for j in range(l):
        sel[j, 0, 0] = sel[l + j, 1, 0] = m << (32 - (j + 1) * basebit)
    return (sel & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _brute(d1, d0, sel, basebit, l):
    """Python integers, one term at a time."""
    N = sel.shape[2]
    B, off = 1 << basebit, sum((1 << basebit >> 1) << (32 - (j + 1) * basebit) for j in range(l)) + (1 << (31 - l * basebit))
    out = [[int(v) & 0xFFFFFFFF for v in d0[p]] for p in range(2)]
    for jr in range(2 * l):
        j, src = jr % l, jr // l
        for k in range(N):
            x = ((0 if d1 is None else int(d1[src][k])) - int(d0[src][k]) + off) & 0xFFFFFFFF
            dig = ((x >> (32 - (j + 1) * basebit)) & (B - 1)) - B // 2
            for p in range(2):
                for i in range(N):
                    w = int(sel[jr][p][i]) & 0xFFFFFFFF
                    if k + i < N:
                        out[p][k + i] = (out[p][k + i] + dig * w) & 0xFFFFFFFF
                    else:
                        out[p][k + i - N] = (out[p][k + i - N] - dig * w) & 0xFFFFFFFF
    return np.array(out, np.uint64).astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("N", [16, 64])
def test_the_numpy_cmux_equals_a_brute_force_negacyclic_product(N):
    rng = np.random.default_rng(N)
    for basebit, l in ((8, 3), (4, 6), (1, 31), (5, 2)):
        d1, d0 = _extreme(rng, 2, N, basebit, l)
        sel = _words(rng, 2 * l, 2, N)
        got = keygen.ring_cmux(d1, d0, sel, basebit, l)
        assert np.array_equal(got[0], _brute(d1[0], d0[0], sel, basebit, l)) and np.array_equal(got[1], _brute(d1[1], d0[1], sel, basebit, l))
        assert np.array_equal(keygen.ring_cmux(None, d0[:1], sel, basebit, l)[0], _brute(None, d0[0], sel, basebit, l))


def test_the_digits_are_signed_and_rebuild_the_rounded_word():
    rng = np.random.default_rng(4)
    E = emu_lib.lib()
    E.rs_emu_ring_cmux_offset.restype = E.rs_emu_ring_cmux_digit.restype = C.c_uint32
    for basebit, l in SHAPES:
        d1, d0 = _extreme(rng, 1, 1024, basebit, l)
        x = (_u32(d1[0, 0]) - _u32(d0[0, 0])).view(np.int32)
        d = keygen.ring_cmux_digits(x, basebit, l)
        B = 1 << basebit
        assert d.shape == (l, 1024) and d.min() >= -B // 2 and d.max() <= B // 2 - 1
        h = np.array([1 << (32 - (j + 1) * basebit) for j in range(l)], np.int64)
        step = 1 << (32 - l * basebit)
        want = ((_u32(x).astype(np.int64) + step // 2) // step * step) & 0xFFFFFFFF           # x rounded to l basebit bits
        assert np.array_equal((d * h[:, None]).sum(0) & 0xFFFFFFFF, want)
        off = keygen.ring_cmux_offset(basebit, l)
        assert E.rs_emu_ring_cmux_offset(basebit, l) == off
        for j in range(l):
            for k in range(8):
                xbar = (int(_u32(x)[k]) + off) & 0xFFFFFFFF
                assert E.rs_emu_ring_cmux_digit(C.c_uint32(xbar), basebit, j) == int(d[j, k]) & 0xFFFFFFFF


def _emu_cmux(d1, d0, R, stride, N, sel, basebit, l):
    E = emu_lib.lib()
    out = np.full((R + 1, 2, N), 0x5A5A5A5A, np.int32)
    E.rs_emu_ring_cmux(_p(d1), _p(d0), C.c_long(R), C.c_long(stride), N, _p(sel), basebit, l, _p(out))
    assert (out[R] == 0x5A5A5A5A).all()
    return out[:R]


@pytest.mark.parametrize("N,basebit,l,R", [(1024, 4, 6, 1), (1024, 4, 6, 2), (1024, 4, 6, 3), (2048, 8, 3, 1), (2048, 2, 12, 2)]
                         + [(1024, b, l, 1) for b, l in SHAPES])
def test_the_emulated_ring_cmux_kernels_equal_numpy(N, basebit, l, R):
    """Every tile, both source blocks and four tiles of N = 2048, every selector row, every ciphertext; d1 = None; stride 2."""
    E = emu_lib.lib()
    E.rs_emu_ring_cmux_groups.restype = C.c_long
    assert E.rs_emu_ring_cmux_groups(C.c_long(R), N, l) == R * 2 * (N // 512) * (N // 1024) * 2 * l
    rng = np.random.default_rng(N + 10 * basebit + l + 1000 * R)
    d1, d0 = _extreme(rng, 2 * R, N, basebit, l)
    sel = _words(rng, 2 * l, 2, N)
    assert np.array_equal(_emu_cmux(d1, d0, R, 1, N, sel, basebit, l), keygen.ring_cmux(d1[:R], d0[:R], sel, basebit, l))
    assert np.array_equal(_emu_cmux(None, d0, R, 1, N, sel, basebit, l), keygen.ring_cmux(None, d0[:R], sel, basebit, l))
    assert np.array_equal(_emu_cmux(d1, d0, R, 2, N, sel, basebit, l), keygen.ring_cmux(d1[::2], d0[::2], sel, basebit, l))
    # the even and odd entries of a table: d1 = d0 + one row
    assert np.array_equal(_emu_cmux(d0[1:], d0, R, 2, N, sel, basebit, l), keygen.ring_cmux(d0[1::2], d0[0::2], sel, basebit, l))


@pytest.mark.parametrize("basebit,l", SHAPES)
def test_the_noise_free_public_selector_returns_d0_exactly_and_d1_up_to_the_rounding(basebit, l):
    """m = 0: every row of the selector is zero, out = d0 word for word. m = 1: out = d0 + round(d1 - d0), and every coefficient's
    phase is within (1 + N/2) 2^(31 - l basebit) words of d1's: half a step of its own b word and of each of the N/2 a words that
    meet a set key bit (the derived worst case at the key's expected weight N/2; the largest error is printed)."""
    N, sk = N1, _secret()
    d1, d0 = _extreme(np.random.default_rng(10 * basebit + l), 2, N, basebit, l)
    out0 = keygen.ring_cmux(d1, d0, _public_selector(0, N, basebit, l), basebit, l)
    assert np.array_equal(out0, d0)
    out1 = keygen.ring_cmux(d1, d0, _public_selector(1, N, basebit, l), basebit, l)
    err = (_u32(keygen.rlwe_phase(out1, sk.tlwe_key)) - _u32(keygen.rlwe_phase(d1, sk.tlwe_key))).view(np.int32).astype(np.int64)
    bound = (1 + N // 2) * (1 << (31 - l * basebit))
    print("(%d, %d): largest phase error %d words, bound %d" % (basebit, l, np.abs(err).max(), bound))
    assert np.abs(err).max() <= bound                                        # vacuous below 10 bits, where it passes 2^31
    # the emulator on the same selectors
    assert np.array_equal(_emu_cmux(d1, d0, 2, 1, N, _public_selector(0, N, basebit, l), basebit, l), d0)
    assert np.array_equal(_emu_cmux(d1, d0, 2, 1, N, _public_selector(1, N, basebit, l), basebit, l), out1)


@pytest.mark.parametrize("entries", [1, 2, 3, 5, 8])
def test_lookups_under_real_selectors_return_the_entry_and_zero_past_the_table(entries):
    """Trivial rows of 1/4096-scale integers, a seeded selector of the set's deviation for every index below 2^depth: the numpy
    restatement and the emulated kernels agree word for word, and the row (zero past `entries`) decrypts."""
    E = emu_lib.lib()
    E.rs_emu_ring_lookup_scratch_rows.restype = C.c_long
    N, sk = N1, _secret()
    depth = max(1, (entries - 1).bit_length())
    basebit, l = keygen.ring_cmux_default(NAME, depth)
    rng = np.random.default_rng(entries)
    values = rng.integers(-2047, 2048, (entries, N))
    table = keygen.ring_trivial((values << 20).astype(np.int32))
    assert table.shape == (entries, 2, N) and not table[:, 0].any()
    rows = E.rs_emu_ring_lookup_scratch_rows(C.c_long(entries))
    assert rows == -(-entries // 2) + -(-(-(-entries // 2)) // 2)
    for index in range(1 << depth):
        s = _seeds(index)
        sel = sk.ring_selector(index, depth, mask_seed=s[0], noise_seed=s[1])
        assert (sel.basebit, sel.l, sel.depth, sel.nbytes) == (basebit, l, depth, 32 + 4 * N * 2 * l * depth)
        want = keygen.ring_lookup(table, sel.expand(), basebit, l)
        scratch = np.full((rows + 1, 2, N), 0x5A5A5A5A, np.int32)
        out = np.full((2, 2, N), 0x5A5A5A5A, np.int32)
        E.rs_emu_ring_lookup(_p(table), C.c_long(entries), N, _p(sel.expand()), depth, basebit, l, _p(scratch) if depth > 1 else None, _p(out))
        assert np.array_equal(out[0], want) and (out[1] == 0x5A5A5A5A).all() and (scratch[rows] == 0x5A5A5A5A).all()
        got = sk.decrypt_packed_ints(want[None], N)
        assert np.array_equal(got, values[index] if index < entries else np.zeros(N, np.int64)), (entries, index)


def _errors(basebit, l, stdev, bit, count=4):
    """CMUX errors per coefficient as reals, [count][2][N], of fresh secrets and selectors of `bit` and two ciphertext pairs each."""
    errs = []
    for k in range(count):
        s = _seeds(k + 10 * bit + 100 * basebit)
        sk = _secret(NAME, s[0])
        sel = sk.ring_selector(bit, 1, basebit, l, s[1], s[2], stdev=stdev)
        d1, d0 = (_words(np.random.default_rng(k + 50 * q), 2, 2, N1) for q in range(2))
        out = keygen.ring_cmux(d1, d0, sel.expand()[0], basebit, l)
        want = keygen.rlwe_phase(d1 if bit else d0, sk.tlwe_key)
        errs.append((_u32(keygen.rlwe_phase(out, sk.tlwe_key)) - _u32(want)).view(np.int32) / 2.0 ** 32)
    return np.array(errs)


@pytest.mark.parametrize("shape", ["default", (8, 3)])
def test_noisy_selectors_meet_the_formula(shape):
    """Eight selectors (four of each bit, fresh secrets) x two ciphertext pairs at N = 1024 and the set's deviation: the pooled rms
    lies within 15 % of ring_cmux_sigma (the band of tests/test_pack_cpu.py) and every error below 8 sigma. The rounding of x
    reaches the phase multiplied by the selected bit, so the selectors of 1 are held against the formula as it stands and those of
    0 against it without its rounding term (bit=0); the eight together against the mean of the two variances."""
    basebit, l = keygen.ring_cmux_default(NAME) if shape == "default" else shape
    stdev = keygen.rlwe_default_stdev(NAME)
    sig = [keygen.ring_cmux_sigma(N1, basebit, l, stdev, bit=b) for b in (0, 1)]
    e = [_errors(basebit, l, stdev, b) for b in (0, 1)]
    for b in (0, 1):
        rms = float(np.sqrt(np.mean(e[b] * e[b])))
        print("(%d, %d) bit %d: sigma %.4g, rms / formula %.3f, largest %.2f sigma" % (basebit, l, b, sig[b], rms / sig[b], np.abs(e[b]).max() / sig[b]))
        assert abs(rms / sig[b] - 1.0) < 0.15
        assert np.abs(e[b]).max() < 8 * sig[b]
    both, pooled = np.concatenate(e), np.sqrt((sig[0] ** 2 + sig[1] ** 2) / 2)
    assert abs(float(np.sqrt(np.mean(both * both))) / pooled - 1.0) < 0.15 and np.abs(both).max() < 8 * sig[1]
    assert sig[0] <= sig[1] == keygen.ring_cmux_sigma(N1, basebit, l, stdev)


def test_selector_files_round_trip_and_reject_damage():
    sk = _secret()
    sel = sk.ring_selector(5, 3, 4, 6, MASK_SEED, NOISE_SEED)
    assert sel.body.shape == (3, 12, 1024) and sel.expand().shape == (3, 12, 2, 1024) and sel.nbytes == 32 + 4 * 1024 * 12 * 3
    assert np.array_equal(sel.expand()[:, :, 1], sel.body)
    assert np.array_equal(sel.expand()[:, :, 0].reshape(36, 1024), keygen.ring_selector_mask(MASK_SEED, 1024, np.arange(36)))
    buf = io.BytesIO()
    client.write_ring_selector(buf, sel)
    raw = buf.getvalue()
    hs = client._RS_HEADER.itemsize
    assert len(raw) == hs + 12 + sel.nbytes and raw[:4] == b"RSG1"
    back = client.read_ring_selector(io.BytesIO(raw))
    assert (back.name, back.N, back.depth, back.basebit, back.l, back.mask_seed) == (NAME, 1024, 3, 4, 6, MASK_SEED)
    assert np.array_equal(back.expand(), sel.expand())
    digits = lambda *v: raw[:hs] + np.array(v, "<i4").tobytes() + raw[hs + 12:]
    bad_shape = np.frombuffer(raw[:hs], client._RS_HEADER).copy()
    bad_shape["N"] = 512
    for damaged in (raw[:-4], raw + b"\0\0\0\0", raw[:40], raw[:3], b"", raw[:hs + 8], b"RSX1" + raw[4:], b"RSK1" + raw[4:],
                    digits(3, 9, 6), digits(3, 0, 6), digits(3, 4, 0), digits(3, 4, 8), digits(0, 4, 6), digits(31, 4, 6),
                    digits(2, 4, 6), digits(3, 4, 5), bad_shape.tobytes() + raw[hs:],
                    client._rs_header("RSG1", "redsec_medium", 3072) + raw[hs:]):
        with pytest.raises(ValueError):
            client.read_ring_selector(io.BytesIO(damaged))
    with pytest.raises(ValueError):
        client.read_ring_rekey_key(io.BytesIO(raw))                          # a selector is not an RSX1 file
    assert client.RS_MAGIC["RSG1"] not in [v for k, v in client.RS_MAGIC.items() if k != "RSG1"]


def test_refusals_and_defaults():
    sk = _secret()
    with pytest.raises(ValueError, match="equal"):
        sk.ring_selector(1, 1, mask_seed=MASK_SEED, noise_seed=MASK_SEED)
    for index, depth in ((2, 1), (8, 3), (-1, 3), (0, 0), (0, 31)):
        with pytest.raises(ValueError):
            sk.ring_selector(index, depth, mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    a, b = sk.ring_selector(1, 1), sk.ring_selector(1, 1)                    # fresh seeds by default
    assert (a.basebit, a.l) == keygen.ring_cmux_default(NAME, 1) and a.mask_seed != b.mask_seed and not np.array_equal(a.body, b.body)
    medium = _secret("redsec_medium")                                        # bk_stdev truncates to zero
    with pytest.raises(ValueError, match="explicit stdev"):
        medium.ring_selector(1, 1, mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    assert medium.ring_selector(1, 1, 8, 1, MASK_SEED, NOISE_SEED, stdev=2.0 ** -31).body.shape == (1, 2, 4096)
    z = np.zeros((1, 2, 1024), np.int32)
    for basebit, l in ((0, 4), (9, 2), (4, 0), (4, 8), (8, 4), (1, 32)):
        with pytest.raises(ValueError):
            sk.ring_selector(1, 1, basebit, l, MASK_SEED, NOISE_SEED)
        with pytest.raises(ValueError):
            keygen.ring_cmux(z, z, np.zeros((2 * max(l, 1), 2, 1024), np.int32), basebit, l)
        with pytest.raises(ValueError):
            keygen.ring_cmux_sigma(1024, basebit, l, 0.0)
    with pytest.raises(ValueError):
        keygen.ring_lookup(np.zeros((3, 2, 1024), np.int32), np.zeros((1, 6, 2, 1024), np.int32), 8, 3)    # three entries, one level
    assert np.array_equal(keygen.ring_trivial(np.arange(4, dtype=np.int32)), [[0, 0, 0, 0], [0, 1, 2, 3]])
    assert keygen.ring_cmux_sigma(1024, 8, 3, 2.0 ** -30, depth=4) == pytest.approx(2 * keygen.ring_cmux_sigma(1024, 8, 3, 2.0 ** -30))


UNREACHED = {("default128", 20), ("default128", 30)}                         # INTEGRATION.md section 23 lists them


def test_the_defaults_keep_eight_sigma_or_the_set_is_listed():
    """8 ring_cmux_sigma against the half step 1/8192 at rows of the set's rlwe_default_stdev (2^-31 where that is refused), for the
    smallest l that reaches it; default-128, whose rows are 32 times noisier, has no shape past depth 10."""
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, v in client.PARAM_SETS.items():
        stdev = keygen.ring_selector_default_stdev(name)
        for depth in (1, 3, 10, 20, 30):
            if (name, depth) in UNREACHED:
                with pytest.raises(ValueError, match="no \\(basebit, l\\)"):
                    keygen.ring_cmux_default(name, depth)
                best = max((1 / 8192) / keygen.ring_cmux_sigma(v[1], b, l, stdev, depth) for b in range(1, 9) for l in range(1, 32) if b * l <= 31)
                assert best < 8
                continue
            basebit, l = keygen.ring_cmux_default(name, depth)
            sigma = keygen.ring_cmux_sigma(v[1], basebit, l, stdev, depth)
            print("%s depth %d (%d, %d): sigma %.3g, margin %.1f sigma" % (name, depth, basebit, l, sigma, (1 / 8192) / sigma))
            assert 8 * sigma <= 1 / 8192 and l * basebit <= 31
            # no smaller l reaches it
            assert all(8 * keygen.ring_cmux_sigma(v[1], b, l - 1, stdev, depth) > 1 / 8192 for b in range(1, 9) if l > 1 and b * (l - 1) <= 31)
    assert "default-128" in integration and "depth 10" in integration
    assert keygen.ring_cmux_default(NAME, 10) == (7, 3) and keygen.ring_cmux_default("redsec_large", 10) == (6, 4)


def test_symbols_prototypes_and_formula_are_in_the_header_the_library_the_binding_the_recipe_and_the_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_ring_cmux_dev\(rs_ctx\* ctx, int32_t\* out, const int32_t\* d1, const int32_t\* d0, size_t R, size_t stride,\s+"
                     r"const int32_t\* sel, int32_t basebit, int32_t l, void\* stream\);", header)
    assert re.search(r"int rs_ring_lookup_dev\(rs_ctx\* ctx, int32_t\* out, const int32_t\* table, size_t entries,\s+"
                     r"const int32_t\* sel, int32_t depth, int32_t basebit, int32_t l, int32_t\* scratch, void\* stream\);", header)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    formula = "sigma^2 = depth (2 l N (B^2 + 2)/12 sigma_row^2  +  (1 + N/2) 2^(-2 l basebit)/12)"
    assert formula in integration and formula in (keygen.ring_cmux_sigma.__doc__ or "")
    for line in ("out[r]   = d0[r] + sum_{j<l} Da_j(X) sel[j] + sum_{j<l} Db_j(X) sel[l+j]",
                 "u_j(w)   = ((w + off) >> (32 - (j+1) basebit)) & (B - 1),   dig_j(w) = u_j(w) - B/2"):
        assert line in header and line in integration, line
    L = redsec_amd.load_library()
    for sym in ("rs_ring_cmux_dev", "rs_ring_lookup_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and hasattr(L, sym)
        assert sym in integration and sym in design and sym in readme
    for f in ("ring_cmux", "ring_lookup", "upload_ring_selector"):
        assert callable(getattr(redsec_amd.Backend, f))
    assert callable(client.SecretKeySet.ring_selector)
    for f in ("ring_cmux", "ring_lookup", "ring_cmux_digits", "ring_selector_rows", "ring_selector_expand", "ring_trivial",
              "ring_cmux_sigma", "ring_cmux_default"):
        assert callable(getattr(keygen, f))
    for f in ("RingSelector", "write_ring_selector", "read_ring_selector"):
        assert hasattr(client, f)
    assert (keygen.DOMAIN_RING_SELECTOR_MASK, keygen.DOMAIN_RING_SELECTOR_NOISE) == (18, 19) and "domain 18" in keygen.__doc__
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_ring_cmux", "rs_ring_cmux.hip", [])' in build and build.count('"rs_ring_cmux.h"') == 2
    assert "## 23." in integration
    named = re.findall(r"profiles/r26/[\w./-]*\w", integration + design + open(os.path.join(ROOT, "profiles", "r26", "README.md")).read())
    assert named
    for path in named:
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_failure_without_a_context_matches_ring_rekey():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    rc = L.rs_ring_rekey_dev(None, p, p, 1, p, 4, 5, None)
    msg = L.rs_last_error()
    assert rc != 0
    assert L.rs_ring_cmux_dev(None, p, p, p, 1, 1, p, 4, 6, None) == rc and L.rs_last_error() == msg
    assert L.rs_ring_cmux_dev(None, None, None, None, 0, 0, None, 0, 0, None) == rc and L.rs_last_error() == msg
    assert L.rs_ring_lookup_dev(None, p, p, 1, p, 1, 4, 6, p, None) == rc and L.rs_last_error() == msg
    assert L.rs_ring_lookup_dev(None, None, None, 0, None, 0, 0, 0, None, None) == rc and L.rs_last_error() == msg


def test_new_kernels_hold_zero_scratch_and_no_static_lds():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    for pat, vgpr in (("16ring_cmux_kernel", 40), ("21ring_cmux_init_kernel", 16)):
        hit = {n: k for n, k in ks.items() if pat in n}
        assert len(hit) == 1, (pat, sorted(hit))
        for k in hit.values():
            assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= vgpr, (pat, k)   # the LDS is dynamic


def test_ring_cmux_sources_are_integer_only():
    """As rs_pack.*, rs_rekey.* and rs_ring_rekey.*: the sources name no floating type and include neither a transform nor the
    split-key product."""
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_ring_cmux.h", "rs_ring_cmux.hip", "rs_ring_sweep.h"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\b(double|float|half|__fp16|_Float16)\b|rs_general\.h|rs_fft\.h|rs_ntt\.h", code), f
