"""Which form a keyswitch launch takes (csrc/rs_host.h keyswitch_form, replayed on the CPU through the emulator library), at every
boundary of the batch size, and the register / scratch / LDS budget of the wide kernel read from the built library."""
import ctypes
import re

import pytest

import emu_lib
import test_kernel_budgets as budgets

GATHER, TILED, SLICED, WIDE = 0, 1, 2, 3
AUTO = -1
CUS = 256
TILE = 1024          # ciphertexts of a wide workgroup


def _form(B, W, N, t, basebit, cus=CUS, force=AUTO):
    L = emu_lib.lib()
    L.rs_emu_keyswitch_form.restype = ctypes.c_long
    L.rs_emu_keyswitch_form.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.rs_emu_keyswitch_slices.restype = ctypes.c_long
    v = L.rs_emu_keyswitch_form(B, W, N, t, basebit, cus, force)
    return v % 16, v // 16


def _slices(B, W, N):
    return emu_lib.lib().rs_emu_keyswitch_slices(B, W, N)


# (t, basebit, W, N, has a wide kernel): the three tiled shapes at the width of their shipped sets
SHAPES = [(8, 2, 631, 1024, True), (9, 3, 351, 1024, True), (18, 1, 501, 1024, False)]


def _first_unsliced(W, N):
    """Smallest B whose tiled launch is not sliced: ceil(B / 256) x ceil(W / 32) workgroups reach 1,024."""
    gy = (W + 31) // 32
    gx = -(-1024 // gy)
    return (gx - 1) * 256 + 1


def _first_wide(W, cus):
    """Smallest B with one full 1,024-ciphertext tile per CU over all word columns."""
    gy = (W + 31) // 32
    return -(-cus // gy) * TILE


@pytest.mark.parametrize("t,basebit,W,N,wide", SHAPES)
def test_form_at_every_boundary_of_the_batch_size(t, basebit, W, N, wide):
    assert _form(0, W, N, t, basebit) == (GATHER, 1)            # nothing is launched
    assert _form(1, W, N, t, basebit) == (SLICED, 64)
    for B in (TILE - 1, TILE, TILE + 1):
        assert _form(B, W, N, t, basebit) == (SLICED, _slices(B, W, N)) and _slices(B, W, N) > 1
    b1 = _first_unsliced(W, N)
    assert _slices(b1 - 1, W, N) == 2 and _slices(b1, W, N) == 1
    assert _form(b1 - 1, W, N, t, basebit) == (SLICED, 2)
    assert _form(b1, W, N, t, basebit) == (TILED, 1)             # un-sliced, but not yet a full wide tile per CU
    assert _form(b1 + 1, W, N, t, basebit) == (TILED, 1)
    bw = _first_wide(W, CUS)
    assert bw > b1
    assert _form(bw - 1, W, N, t, basebit) == (TILED, 1)
    assert _form(bw, W, N, t, basebit) == ((WIDE if wide else TILED), 1)
    assert _form(bw + 1, W, N, t, basebit) == ((WIDE if wide else TILED), 1)
    assert _form(65536, W, N, t, basebit) == ((WIDE if wide else TILED), 1)   # the benchmark's batch


def test_the_thresholds_of_the_shipped_sets_in_numbers():
    assert (_first_unsliced(631, 1024), _first_wide(631, CUS)) == (13057, 13312)     # default-128: 20 word columns
    assert (_first_unsliced(351, 1024), _first_wide(351, CUS)) == (23809, 24576)     # REDsec set: 11 word columns
    assert _form(13312, 631, 1024, 8, 2, cus=304) == (TILED, 1) and _form(16384, 631, 1024, 8, 2, cus=304) == (WIDE, 1)   # follows the CU count


def test_an_untiled_shape_takes_the_gather_form_at_every_size():
    for B in (1, TILE - 1, TILE, TILE + 1, 13056, 13057, 13312, 65536):
        for force in (AUTO, TILED, WIDE):
            assert _form(B, 25, 1024, 6, 2, force=force) == (GATHER, 1)


@pytest.mark.parametrize("t,basebit,W,N,wide", SHAPES)
def test_the_diagnostic_switch_forces_and_forbids_the_wide_form(t, basebit, W, N, wide):
    for B in (1, TILE - 1, TILE, TILE + 1, 2049, 65536):
        plain = _form(B, W, N, t, basebit)
        assert _form(B, W, N, t, basebit, force=WIDE) == ((WIDE, 1) if wide else plain)
        never = _form(B, W, N, t, basebit, force=TILED)
        assert never == ((TILED, 1) if plain[0] == WIDE else plain)
    assert _form(0, W, N, t, basebit, force=WIDE) == (GATHER, 1)


def test_wide_kernel_budget_from_the_built_library():
    """One workgroup of 16 waves per CU: at most 128 VGPRs (four waves per SIMD), no scratch, both double-buffered tables inside
    112 KB of LDS."""
    ks = budgets._kernels()
    hit = {n: k for n, k in ks.items() if re.search(r"21keyswitch_wide_kernel", n)}
    assert any("ILi8ELi2ELi4ELi2ELb0E" in n for n in hit), sorted(hit)          # the flagship shape <8, 2, D = 2>
    for n, k in hit.items():
        assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["lds"] <= 112 * 1024, (n, k)


def test_the_sample_load_probe_build_compiles():
    """-DRS_DIAG=512 (csrc/rs_diag.h): nothing else would notice that path rotting. Front end only."""
    import test_abi
    r = test_abi._syntax_only("rs_keyswitch_wide.hip", ["-DRS_DIAG=512"])
    assert r.returncode == 0, r.stderr[-3000:]
