"""Batched encrypted lookup without a GPU (rs_ring_lookup_rows_dev, rs_ring_lookup_rows_alt_dev): the lane
emulator of the kernels against the numpy restatement and against R emulated single lookups word for word, the phase of the result
against the phase of the chosen entry under noise-free selectors of a real secret, decryption under noisy ones, the scratch plan,
symbols, the failure without a context and kernel budgets."""
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
FORMS = ["signed", "alternating"]
SENTINEL = 0x5A5A5A5A
# (R, entries, depth): an odd row count at two successive levels, a single entry, a full tree, an index range larger than the
# table, and R = 1
CASES = [(3, 5, 3), (2, 1, 2), (2, 8, 3), (3, 6, 4), (1, 3, 2)]
EXTREMES = [0, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, 1]


def _strides(R, E):
    """(row_stride, entry_stride): one shared table, R tables one after another, entries R ciphertexts wide, padded tables."""
    return [(0, 1), (E, 1), (1, R), (E + 1, 1)]


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


def _held(R, E, row_stride, entry_stride):
    return (R - 1) * row_stride + (E - 1) * entry_stride + 1


def _table(rng, cts, N):
    """Random ciphertexts whose first and last words are the extreme words, turned by one place from one ciphertext to the next:
    the differences of any two of them at both ends of both polynomials are 0, +-2^31, 2^31 - 1 and their neighbours, and an
    unpaired row (whose difference is minus itself) carries them too."""
    t = _words(rng, cts, 2, N)
    n = len(EXTREMES)
    for c in range(cts):
        ends = np.array([EXTREMES[(i + c) % n] for i in range(n)], np.uint32).view(np.int32)
        t[c, :, :n] = ends
        t[c, :, -n:] = ends
    return t


def _emu():
    E = emu_lib.lib()
    sig = [C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    E.rs_emu_ring_lookup_rows.argtypes = E.rs_emu_ring_lookup_rows_alt.argtypes = sig
    E.rs_emu_ring_lookup_rows.restype = E.rs_emu_ring_lookup_rows_alt.restype = None
    sig1 = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    E.rs_emu_ring_lookup.argtypes = E.rs_emu_ring_lookup_alt.argtypes = sig1
    E.rs_emu_ring_lookup.restype = E.rs_emu_ring_lookup_alt.restype = None
    for f, args in ((E.rs_emu_ring_lookup_level_rows, [C.c_long]), (E.rs_emu_ring_lookup_rows_groups, [C.c_long, C.c_long, C.c_int, C.c_int]),
                    (E.rs_emu_ring_lookup_rows_scratch_rows, [C.c_long, C.c_long]), (E.rs_emu_ring_cmux_groups, [C.c_long, C.c_int, C.c_int])):
        f.argtypes, f.restype = args, C.c_long
    E.rs_emu_ring_lookup_rows_place.argtypes = [C.c_long, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    E.rs_emu_ring_lookup_rows_place.restype = None
    return E


def _scratch_rows(R, E):
    first = -(-E // 2)
    return R * (first + -(-first // 2))


def _emu_rows(table, E, row_stride, entry_stride, R, sel, basebit, l, digits, per_row, buffers=None):
    """The emulated call with guard ciphertexts behind out and scratch; scratch starts from a sentinel and is null at depth 1."""
    lib = _emu()
    N, depth = sel.shape[-1], sel.shape[-4]
    rows = _scratch_rows(R, E)
    out, scratch = buffers or (np.full((R + 1, 2, N), SENTINEL, np.int32), np.full((rows + 1, 2, N), SENTINEL, np.int32) if depth > 1 else None)
    before, sel_before = table.copy(), sel.copy()
    f = lib.rs_emu_ring_lookup_rows_alt if digits == "alternating" else lib.rs_emu_ring_lookup_rows
    f(_p(table), E, row_stride, entry_stride, R, N, _p(sel), depth, int(per_row), basebit, l, _p(scratch), _p(out))
    assert (out[R] == SENTINEL).all() and (scratch is None or (scratch[rows] == SENTINEL).all())
    assert np.array_equal(table, before) and np.array_equal(sel, sel_before)
    return out[:R]


def _numpy_rows(cache, table, sets, E, row_stride, entry_stride, R, basebit, l, digits, per_row):
    """keygen.ring_lookup_rows, the single lookups of it remembered in the caller's `cache` by (entries read, selector set): rows of
    different stride pairs that read the same ciphertexts under the same set are computed once."""
    out = np.zeros((R, 2, table.shape[-1]), np.int32)
    for q in range(R):
        idx = tuple(q * row_stride + e * entry_stride for e in range(E))
        s = q if per_row else 0
        if (idx, s) not in cache:
            cache[(idx, s)] = keygen.ring_lookup_rows(table[list(idx)], sets[s], basebit, l, E, 1, 0, 1, digits=digits)[0]
        out[q] = cache[(idx, s)]
    return out


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("R,E,depth", CASES)
def test_the_emulated_kernels_equal_numpy_for_every_stride_pair_and_selector_layout(R, E, depth, digits):
    N, basebit, l = N1, 8, 3
    rng = np.random.default_rng(100 * R + 10 * E + depth)
    sets = _words(rng, R, depth, 2 * l, 2, N)
    table = _table(rng, max(_held(R, E, rs, es) for rs, es in _strides(R, E)), N)
    cache = {}
    for row_stride, entry_stride in _strides(R, E):
        for per_row in (0, 1):
            sel = sets if per_row else np.ascontiguousarray(sets[0])
            want = _numpy_rows(cache, table, sets, E, row_stride, entry_stride, R, basebit, l, digits, per_row)
            got = _emu_rows(table[:_held(R, E, row_stride, entry_stride)].copy(), E, row_stride, entry_stride, R, sel, basebit, l, digits, per_row)
            assert np.array_equal(got, want), (row_stride, entry_stride, per_row)
    direct = keygen.ring_lookup_rows(table, sets, basebit, l, E, R, E, 1, digits=digits)      # the restatement itself, not the cache
    assert np.array_equal(direct, _numpy_rows(cache, table, sets, E, E, 1, R, basebit, l, digits, 1))


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("basebit,l", [(1, 1), (4, 6), (1, 31)])
def test_every_digit_shape_equals_numpy(basebit, l, digits):
    R, E, depth = 3, 5, 3
    rng = np.random.default_rng(10 * basebit + l)
    sets = _words(rng, R, depth, 2 * l, 2, N1)
    table = _table(rng, _held(R, E, E, 1), N1)
    want = keygen.ring_lookup_rows(table, sets, basebit, l, E, R, E, 1, digits=digits)
    assert np.array_equal(_emu_rows(table, E, E, 1, R, sets, basebit, l, digits, 1), want)


@pytest.mark.parametrize("digits", FORMS)
def test_the_larger_ring_equals_numpy(digits):
    N, basebit, l, (R, E, depth) = 2048, 8, 3, (2, 3, 2)
    rng = np.random.default_rng(2048)
    sets = _words(rng, R, depth, 2 * l, 2, N)
    table = _table(rng, _held(R, E, E, 1), N)
    want = keygen.ring_lookup_rows(table, sets, basebit, l, E, R, E, 1, digits=digits)
    assert np.array_equal(_emu_rows(table, E, E, 1, R, sets, basebit, l, digits, 1), want)
    shared = keygen.ring_lookup_rows(table, sets[1], basebit, l, E, R, 1, 2, digits=digits)
    assert np.array_equal(_emu_rows(table[:_held(R, E, 1, 2)].copy(), E, 1, 2, R, np.ascontiguousarray(sets[1]), basebit, l, digits, 0), shared)


@pytest.mark.parametrize("digits", FORMS)
@pytest.mark.parametrize("R,E,depth", CASES)
def test_the_rows_call_gives_the_words_of_single_emulated_lookups_and_a_second_call_gives_them_again(R, E, depth, digits):
    lib = _emu()
    N, basebit, l = N1, 8, 3
    rng = np.random.default_rng(7 * R + E)
    sets = _words(rng, R, depth, 2 * l, 2, N)
    row_stride, entry_stride = 1, R
    table = _table(rng, _held(R, E, row_stride, entry_stride), N)
    single = lib.rs_emu_ring_lookup_alt if digits == "alternating" else lib.rs_emu_ring_lookup
    want = np.zeros((R, 2, N), np.int32)
    for q in range(R):
        rows = np.ascontiguousarray(table[q::entry_stride][:E])
        scratch = np.zeros((_scratch_rows(1, E), 2, N), np.int32)
        single(_p(rows), E, N, _p(sets[q]), depth, basebit, l, _p(scratch), _p(want[q]))
    buffers = (np.full((R + 1, 2, N), SENTINEL, np.int32), np.full((_scratch_rows(R, E) + 1, 2, N), SENTINEL, np.int32))
    first = _emu_rows(table, E, row_stride, entry_stride, R, sets, basebit, l, digits, 1, buffers).copy()
    assert np.array_equal(first, want)
    kept = buffers[1].copy()
    again = _emu_rows(table, E, row_stride, entry_stride, R, sets, basebit, l, digits, 1, buffers)
    assert np.array_equal(again, first) and np.array_equal(buffers[1], kept)


def test_noise_free_selectors_of_a_real_secret_return_the_phase_of_the_chosen_entry_up_to_the_rounding():
    """Truth, not a restatement: eight rows, one for every index of depth 3 over a shared table of E = 5 random ciphertexts, in ONE
    emulated call. Under selectors without noise the phase of out[q] is the phase of table[index_q] (zero for the indices 5 to 7),
    up to the rounding of each level's difference to l basebit bits: half a step on the coefficient's own b word and on each of
    the N/2 a words that meet a set key bit, depth (1 + N/2) 2^(31 - l basebit) words in all."""
    sk = _secret()
    depth, E, R = 3, 5, 8
    basebit, l = keygen.ring_cmux_default(NAME, 10)
    assert (basebit, l) == (7, 3)
    rng = np.random.default_rng(28)
    table = _words(rng, E, 2, N1)
    sets = np.stack([sk.ring_selector(q, depth, basebit, l, _seeds(q)[0], _seeds(q)[1], stdev=0.0).expand() for q in range(R)])
    bound = depth * (1 + N1 // 2) * (1 << (31 - l * basebit))
    for digits in FORMS:
        out = _emu_rows(table, E, 0, 1, R, sets, basebit, l, digits, 1)
        for q in range(R):
            want = keygen.rlwe_phase(table[q:q + 1], sk.tlwe_key) if q < E else np.zeros((1, N1), np.int32)
            err = (_u32(keygen.rlwe_phase(out[q:q + 1], sk.tlwe_key)) - _u32(want)).view(np.int32).astype(np.int64)
            print("%s index %d: largest phase error %d words, bound %d" % (digits, q, np.abs(err).max(), bound))
            assert np.abs(err).max() <= bound, (digits, q)


def test_noisy_selectors_at_the_default_shape_decrypt_to_the_chosen_entries():
    """Four rows with the indices 0 .. 3 over a shared table of three trivial rows at the 1/4096 scale, seeded selectors of the set's
    default shape and deviation: every row decrypts to its entry, index 3 (past the table) to zero."""
    sk = _secret()
    depth, E, R = 2, 3, 4
    basebit, l = keygen.ring_cmux_default(NAME, depth)
    rng = np.random.default_rng(4096)
    values = rng.integers(-2047, 2048, (E, N1))
    table = keygen.ring_trivial((values << 20).astype(np.int32))
    sels = [sk.ring_selector(q, depth, mask_seed=_seeds(q)[0], noise_seed=_seeds(q)[1]) for q in range(R)]
    assert all((s.basebit, s.l) == (basebit, l) for s in sels)
    sets = np.stack([s.expand() for s in sels])
    out = _emu_rows(table, E, 0, 1, R, sets, basebit, l, "signed", 1)
    assert np.array_equal(out, keygen.ring_lookup_rows(table, sets, basebit, l, E, R))
    for q in range(R):
        got = sk.decrypt_packed_ints(out[q:q + 1], N1)
        assert np.array_equal(got, values[q] if q < E else np.zeros(N1, np.int64)), q


def test_the_scratch_plan_the_level_rows_and_the_placement():
    lib = _emu()
    for R in (0, 1, 3, 256):
        for E in (1, 2, 3, 5, 8, 63, 64, 1 << 30):
            assert lib.rs_emu_ring_lookup_rows_scratch_rows(R, E) == R * (-(-E // 2) + -(-E // 4)) == _scratch_rows(R, E)
    for rows in (1, 2, 3, 5, 8, 1 << 30):
        assert lib.rs_emu_ring_lookup_level_rows(rows) == (rows + 1) // 2
        assert lib.rs_emu_ring_lookup_rows_groups(3, rows, 1024, 3) == 3 * ((rows + 1) // 2) * lib.rs_emu_ring_cmux_groups(1, 1024, 3)
    q, i = C.c_long(), C.c_long()
    for P in (1, 2, 3, 7):
        for g in (0, 1, P - 1, P, 5 * P + P // 2, (1 << 31) - 1):
            lib.rs_emu_ring_lookup_rows_place(g, P, C.byref(q), C.byref(i))
            assert (q.value, i.value) == divmod(g, P), (g, P)


def test_the_numpy_restatement_refuses_bad_arguments():
    z, s = np.zeros((2, 2, 1024), np.int32), np.zeros((1, 2, 2, 1024), np.int32)
    with pytest.raises(ValueError):
        keygen.ring_lookup_rows(z, s, 8, 1, 2, 1, entry_stride=0)
    with pytest.raises(ValueError):
        keygen.ring_lookup_rows(z, s, 8, 1, 2, 1, row_stride=-1)
    with pytest.raises(ValueError):
        keygen.ring_lookup_rows(z, s, 8, 4, 2, 1)
    with pytest.raises(ValueError):
        keygen.ring_lookup_rows(z, s, 8, 1, 2, 1, digits="other")
    with pytest.raises(ValueError):
        keygen.ring_lookup_rows(np.zeros((3, 2, 1024), np.int32), s, 8, 1, 3, 1)             # three entries, depth 1


def test_symbols_prototypes_and_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    for name in ("rs_ring_lookup_rows_dev", "rs_ring_lookup_rows_alt_dev"):
        assert re.search(r"int %s\(rs_ctx\* ctx, int32_t\* out, const int32_t\* table, size_t entries,\s+"
                         r"size_t row_stride, size_t entry_stride, size_t R,\s+"
                         r"const int32_t\* sel, int32_t depth, int32_t per_row,\s+"
                         r"int32_t basebit, int32_t l, int32_t\* scratch, void\* stream\);" % name, header), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    L = redsec_amd.load_library()
    for sym in ("rs_ring_lookup_rows_dev", "rs_ring_lookup_rows_alt_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and hasattr(L, sym)
        assert sym in integration, sym
    assert "rs_ring_lookup_rows_dev" in design and "rs_ring_lookup_rows_dev" in readme and "## 28." in integration
    assert callable(redsec_amd.Backend.ring_lookup_rows) and callable(keygen.ring_lookup_rows)
    from redsec_amd import arith, build
    assert callable(arith.lookup_rows) and callable(arith.evaluate)
    assert "out of scope" not in arith.evaluate.__doc__ and "ring_lookup_rows" in arith.evaluate.__doc__
    assert ("rs_ring_lookup", "rs_ring_lookup.hip", []) in build.HIP_OBJECTS
    assert "rs_ring_lookup.h" in build.HIP_DEPS and "rs_ring_lookup.h" in build.EMU_DEPS and "rs_ring_lookup.hip" in build.HIP_SOURCES
    E = emu_lib.lib()
    for sym in ("rs_emu_ring_lookup_rows", "rs_emu_ring_lookup_rows_alt", "rs_emu_ring_lookup_rows_groups", "rs_emu_ring_lookup_rows_scratch_rows"):
        assert hasattr(E, sym), sym
    named = re.findall(r"profiles/r33/[\w./-]*\w", integration + design + open(os.path.join(ROOT, "profiles", "r33", "README.md")).read())
    assert named
    for path in named:
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_failure_without_a_context_matches_ring_cmux():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    L.rs_ring_lookup_rows_dev.argtypes = L.rs_ring_lookup_rows_alt_dev.argtypes = \
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
         C.c_void_p, C.c_void_p]
    rc = L.rs_ring_cmux_dev(None, p, p, p, 1, 1, p, 4, 6, None)
    msg = L.rs_last_error()
    assert rc != 0
    for call in (L.rs_ring_lookup_rows_dev, L.rs_ring_lookup_rows_alt_dev):
        assert call(None, p, p, 1, 0, 1, 1, p, 1, 0, 4, 6, p, None) == rc and L.rs_last_error() == msg
        assert call(None, None, None, 0, 0, 0, 0, None, 0, 0, 0, 0, None, None) == rc and L.rs_last_error() == msg


def test_the_new_kernels_keep_the_budget_of_the_rotate_kernels():
    """No scratch, no static LDS (the 10 KB are dynamic, the launch's own figure), and no more vector registers than the rotation
    kernels of the same library, so the occupancy is no lower than theirs."""
    import test_kernel_budgets as kb
    ks = kb._kernels()

    def one(pat):
        hit = [k for n, k in ks.items() if pat in n]
        assert len(hit) == 1, (pat, sorted(n for n in ks if pat in n))
        return hit[0]
    for new, old in (("24ring_lookup_level_kernel", "18ring_rotate_kernel"), ("28ring_lookup_level_alt_kernel", "22ring_rotate_alt_kernel"),
                     ("23ring_lookup_init_kernel", "23ring_rotate_init_kernel")):
        k, ref = one(new), one(old)
        assert ref["scratch"] == 0 and ref["lds"] == 0
        assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= ref["vgpr"], (new, k, ref)


def test_ring_lookup_sources_are_integer_only_and_hold_no_inline_assembly():
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_ring_lookup.h", "rs_ring_lookup.hip"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\b(double|float|half|__fp16|_Float16|asm|__asm__)\b|rs_general\.h|rs_fft\.h|rs_ntt\.h", code), f
