"""Batched circuit bootstrapping without a GPU (rs_ring_selector_batch_dev, rs_circuit_bootstrap_batch_dev; INTEGRATION.md section
27): the lane emulator of the wide selector kernel against the numpy restatement (keygen.ring_selector_switch, which takes any
number of rows) at every shape at which the kernel takes another path, the plan that picks the kernel at both sides of its
boundary, the closed formulas of the workgroup counts and the scratch, and the kernel's budget read from the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib
import redsec_amd
import test_kernel_budgets as budgets
from redsec_amd import keygen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS_SHAPES = [(8, 4), (1, 1), (4, 6), (2, 12)]                  # (ks_basebit, ks_t); (8, 4) has off = 0
GUARD = 0x5A5A5A5A
AUTO, CHUNKED, WIDE = -1, 0, 1


def _lib():
    E = emu_lib.lib()
    E.rs_emu_ring_selector_wide_groups.restype = C.c_long
    E.rs_emu_ring_selector_wide_groups.argtypes = [C.c_long, C.c_int]
    E.rs_emu_ring_selector_groups.restype = C.c_long
    E.rs_emu_ring_selector_groups.argtypes = [C.c_long, C.c_int, C.c_int]
    E.rs_emu_selector_form.restype = C.c_long
    E.rs_emu_selector_form.argtypes = [C.c_long, C.c_int, C.c_int, C.c_int, C.c_int]
    E.rs_emu_circuit_scratch_words.restype = C.c_long
    E.rs_emu_circuit_scratch_words.argtypes = [C.c_int, C.c_int, C.c_long, C.c_int]
    E.rs_emu_ring_selector_wide.restype = None
    E.rs_emu_ring_selector_wide.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return E


RB = _lib().rs_emu_ring_selector_wide_rows()
PIECE = _lib().rs_emu_ring_selector_wide_piece()


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _extreme(rng, rows, n_src, basebit, l, ks_basebit, ks_t):
    """The samples of _extreme in tests/test_gpu_ring_selector.py: random words whose first and last coordinates x_i (the b word
    before its half step is added) are 0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF and 2^32 - off, which wraps x + off to 0."""
    ct = _words(rng, rows, n_src + 1)
    off = 0 if ks_basebit * ks_t >= 32 else 1 << (31 - ks_basebit * ks_t)
    ext = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, ((1 << 32) - off) & 0xFFFFFFFF], np.uint64).astype(np.uint32)
    for r in range(rows):
        half = 1 << (31 - (r % l + 1) * basebit)
        ct[r, 0] = ext[r % ext.size].view(np.int32)
        ct[r, n_src] = np.uint32((int(ext[(r + 2) % ext.size]) - half) & 0xFFFFFFFF).view(np.int32)
    return ct


def _check(N, n_src, count, basebit, l, ks_basebit, ks_t):
    """The emulated walk into a buffer of guard words with one selector of guards behind it: every word written once, equal to
    numpy, nothing past the rows."""
    E = _lib()
    rng = np.random.default_rng(N + 7 * n_src + 100 * count + l + 1000 * ks_t)
    ct = _extreme(rng, count * l, n_src, basebit, l, ks_basebit, ks_t)
    key = _words(rng, 2, n_src + 1, ks_t, 2, N)
    held_ct, held_key = ct.copy(), key.copy()
    want = keygen.ring_selector_switch(ct, basebit, l, key, ks_basebit, ks_t)
    out = np.full((count + 1, 2 * l, 2, N), GUARD, np.int32)
    E.rs_emu_ring_selector_wide(_p(ct), count, basebit, l, n_src, N, _p(key), ks_basebit, ks_t, _p(out))
    assert (out[count] == GUARD).all()
    assert np.array_equal(out[:count], want), (N, n_src, count, basebit, l, ks_basebit, ks_t, np.argwhere(out[:count] != want)[:4].tolist())
    assert np.array_equal(ct, held_ct) and np.array_equal(key, held_key)


def test_the_constants_the_cases_below_are_built_on():
    E = _lib()
    assert RB == 16 and PIECE == 64 and E.rs_emu_ring_selector_wide_lds_bytes() == PIECE * RB * 4 == 4096
    assert E.rs_emu_ring_selector_rows() == 8 and E.rs_emu_ring_selector_chunk() == 8       # the chunked kernel keeps its own


@pytest.mark.parametrize("l", [1, 3])
@pytest.mark.parametrize("count", [1, RB - 1, RB, RB + 1, 2 * RB + 2])
def test_the_emulated_wide_kernel_equals_numpy_around_the_row_block(count, l):
    """1, RB - 1, RB, RB + 1 and 2 RB + 2: as row counts (l = 1) and as bit counts at l = 3, where a row block of sixteen straddles
    selectors (rows 3, 45, 48, 51 and 102: part of a block, blocks that end inside a selector, whole blocks, several blocks)."""
    _check(1024, 13, count, 3, l, 4, 6)


@pytest.mark.parametrize("n_src", [PIECE - 2, PIECE - 1, PIECE, 2 * PIECE + 5])
def test_the_emulated_wide_kernel_equals_numpy_around_the_staging_piece(n_src):
    """n_src + 1 coordinates one below the staging piece, at it, one past it, and two pieces plus six; nine rows"""
    assert n_src + 1 in (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 6)
    _check(1024, n_src, 3, 3, 3, 4, 6)


@pytest.mark.parametrize("N", [1024, 2048, 4096, 8192])
def test_the_emulated_wide_kernel_equals_numpy_on_every_ring(N):
    """two to sixteen tiles a polynomial, both families and polynomials, nine rows"""
    _check(N, 9, 3, 3, 3, 8, 4)


@pytest.mark.parametrize("ks_basebit,ks_t", KS_SHAPES)
def test_the_emulated_wide_kernel_equals_numpy_for_every_digit_shape_and_gadget(ks_basebit, ks_t):
    _check(1024, 10, 2, 1, 31, ks_basebit, ks_t)
    _check(1024, 10, 1, 8, 3, ks_basebit, ks_t)


@pytest.mark.parametrize("count", [31, 61])
def test_the_emulated_wide_kernel_equals_numpy_past_the_old_limit_of_thirty_bits(count):
    _check(1024, 9, count, 4, 2, 4, 6)


def _form(rows, N, n_src, cus, force=AUTO):
    v = _lib().rs_emu_selector_form(rows, N, n_src, cus, force)
    return v % 2, v // 2


def _wide_groups(rows, N):
    return 4 * (N // 512) * -(-rows // RB)


def _chunked_groups(rows, N, n_src):
    return 4 * (N // 512) * -(-(n_src + 1) // 8) * -(-rows // 8)


@pytest.mark.parametrize("N,cus,first", [(1024, 256, 497), (1024, 304, 593), (8192, 256, 49), (8192, 304, 65)])
def test_the_plan_at_both_sides_of_its_boundary(N, cus, first):
    """wide as soon as its own grid 4 (N / 512) ceil(rows / RB) gives every CU a workgroup: `first` is the smallest such row count"""
    n_src = 350
    assert first == (-(-cus // (4 * (N // 512))) - 1) * RB + 1
    assert _wide_groups(first - 1, N) < cus <= _wide_groups(first, N)
    assert _form(first - 1, N, n_src, cus) == (CHUNKED, _chunked_groups(first - 1, N, n_src))
    assert _form(first, N, n_src, cus) == (WIDE, _wide_groups(first, N))
    assert _form(first + 1, N, n_src, cus) == (WIDE, _wide_groups(first + 1, N))
    assert _form(1, N, n_src, cus) == (CHUNKED, _chunked_groups(1, N, n_src))
    assert _form(38400, N, n_src, cus) == (WIDE, _wide_groups(38400, N))
    assert _form(0, N, n_src, cus) == (CHUNKED, 0)                           # nothing is launched
    for rows in (1, first - 1, first, 38400):                               # the diagnostic switch, at any size
        assert _form(rows, N, n_src, cus, WIDE) == (WIDE, _wide_groups(rows, N))
        assert _form(rows, N, n_src, cus, CHUNKED) == (CHUNKED, _chunked_groups(rows, N, n_src))
    assert _form(0, N, n_src, cus, WIDE) == (CHUNKED, 0)


def test_the_workgroup_counts_and_the_scratch_equal_their_closed_formulas():
    E = _lib()
    for N in (1024, 2048, 4096, 8192):
        for rows in (1, RB - 1, RB, RB + 1, 183, 12800 * 3):
            assert E.rs_emu_ring_selector_wide_groups(rows, N) == _wide_groups(rows, N)
            for n_src in (9, 350, N):
                assert E.rs_emu_ring_selector_groups(rows, N, n_src) == _chunked_groups(rows, N, n_src)
    assert _wide_groups(38400, 1024) == 19200 and _chunked_groups(38400, 1024, 350) == 1689600
    for N, l, count, n in ((1024, 3, 61, 350), (1024, 2, 12800, 350), (8192, 4, 2560, 750), (1024, 1, 1, 16)):
        rows = count * l
        assert E.rs_emu_circuit_scratch_words(N, l, rows, n) == l * N + rows * (2 * (n + 1) + 1)


def test_wide_selector_kernel_budget_from_the_built_library():
    """No scratch, the LDS its header states (one staging piece), and no fewer than two waves per SIMD."""
    ks = budgets._kernels()
    hit = {n: k for n, k in ks.items() if re.search(r"25ring_selector_wide_kernel", n)}
    assert len(hit) == 1, sorted(hit)
    for n, k in hit.items():
        assert k["scratch"] == 0 and 0 < k["lds"] <= _lib().rs_emu_ring_selector_wide_lds_bytes() and k["vgpr"] <= 256, (n, k)
    chunked = {n: k for n, k in ks.items() if re.search(r"20ring_selector_kernel", n)}
    assert len(chunked) == 1                                                # the parent's kernel is still there, beside it


def test_symbols_recipe_and_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_ring_selector_batch_dev\(rs_ctx\* ctx, int32_t\* sel, const int32_t\* ct, size_t count, int32_t basebit, int32_t l,\s+"
                     r"int32_t n_src, const int32_t\* sel_key, int32_t ks_basebit, int32_t ks_t, void\* stream\);", header)
    assert re.search(r"int rs_circuit_bootstrap_batch_dev\(rs_ctx\* ctx, int32_t\* sel, const int32_t\* bits, size_t count, int32_t basebit, int32_t l,\s+"
                     r"const int32_t\* sel_key, int32_t ks_basebit, int32_t ks_t, int32_t\* scratch, void\* stream\);", header)
    assert "int rs_last_selector(rs_ctx* ctx, int32_t* form, int64_t* workgroups);" in header
    for sym in ("rs_ring_selector_batch_dev", "rs_circuit_bootstrap_batch_dev", "rs_last_selector"):
        assert sym in redsec_amd.ABI_SYMBOLS
    for f in ("ring_selector_batch", "circuit_bootstrap_batch", "last_selector"):
        assert callable(getattr(redsec_amd.Backend, f))
    from redsec_amd import build
    assert ("rs_ring_selector_wide", "rs_ring_selector_wide.hip", []) in build.HIP_OBJECTS
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "RS_SEL_FORM" in integration and "rs_circuit_bootstrap_batch_dev" in integration
