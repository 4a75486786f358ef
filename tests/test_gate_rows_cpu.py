"""Three-input gates and indexed gate batches without a GPU (include/redsec_hip.h rs_gate3_dev / rs_gate_rows_dev; INTEGRATION.md
section 14): the row-op table of csrc/rs_rows.h (compiled into the lane emulator) against the oracle's gate constants, the noise-free
truth tables and margins of the three-input combinations, the kernel's own per-word function against the numpy restatement
(tests/rows_ref.py), redsec_amd/arith.py against a stub backend on plaintext bits, and the exports. Nothing here bootstraps: there
is no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import rows_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i32p = C.POINTER(C.c_int32)
E8, E4, HALF = 1 << 29, 1 << 30, 1 << 31


@pytest.fixture(scope="module")
def emu():
    """The emulator library's row exports, loaded here (tests/emu_lib.py does not know them)."""
    from redsec_amd import build
    L = C.CDLL(build.build_emulator())
    L.rs_emu_row_coef.argtypes = [C.c_int, _i32p]
    L.rs_emu_gate_rows.argtypes = [_i32p, _i32p, _i32p, C.c_long, _i32p, _i32p, C.POINTER(C.c_long), C.c_int, C.c_int, C.c_long, _i32p]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def _emu_rows(L, srcs, idx, groups):
    """gate_rows_kernel's placement of the per-word function of rs_rows.h, on the CPU -> x int32 [B][W]."""
    srcs = [np.ascontiguousarray(s, np.int32) for s in srcs]
    in_rows, W = srcs[0].shape
    B = sum(int(c) for _, c in groups)
    idx = None if idx is None else np.ascontiguousarray(idx, np.int32).reshape(B, 3)
    ops = np.array([rr.OPS.index(rr.name(op)) for op, _ in groups], np.int32)
    counts = (C.c_long * len(groups))(*[int(c) for _, c in groups])
    out = np.full((B, W), 0x5a5a5a5a, np.int32)
    assert L.rs_emu_gate_rows(_p(srcs[0]), _p(srcs[1]), _p(srcs[2]), in_rows, _p(idx), _p(ops), counts, len(groups), W, B, _p(out)) == 0
    return out


def _random_rows(rng, rows, W):
    return rng.integers(-2**31, 2**31, (rows, W)).astype(np.int32)


def test_row_op_table_is_the_restated_one_and_ends_at_12(emu):
    for number, op in enumerate(rr.OPS):
        got = (C.c_int32 * 4)()
        assert emu.rs_emu_row_coef(number, got) == 1, op
        coef, bconst = rr.COEF[op]
        assert tuple(got[:3]) == coef and got[3] == bconst, (op, list(got))
    for bad in (-1, 13, 255):
        assert emu.rs_emu_row_coef(bad, (C.c_int32 * 4)()) == 0, bad


@pytest.mark.parametrize("W", [21, 25])
def test_two_input_ops_equal_the_oracle_precombination_word_for_word(emu, W):
    """Ops 0..9 through the row path = TFHE's gate constants as the oracle states them (ro_gate_precombine); the third index
    points anywhere: its row is ignored."""
    rng = np.random.default_rng(W)
    B = 6
    a, b = _random_rows(rng, B, W), _random_rows(rng, B, W)
    inp = np.concatenate([a, b])
    for number, op in enumerate(rr.OPS[:10]):
        assert ol.GATES[op] == number
        third = rng.integers(-5, 2 * B + 5, B)
        idx = np.stack([np.arange(B), B + np.arange(B), third], 1)
        got = _emu_rows(emu, [inp] * 3, idx, [(op, B)])
        assert np.array_equal(got, ol.gate_precombine(op, a, b)), op
        assert np.array_equal(got, rr.combine(inp, idx, [(op, B)])), op


@pytest.mark.parametrize("op,margin", [("MAJ3", E8), ("MAJ3N", E8), ("XOR3", E4)])
def test_three_input_truth_tables_noise_free(emu, op, margin):
    """All eight noise-free inputs (the trivial samples, by index -2 / -1): the combined phase has the sign of the truth table and lies
    exactly `margin` from the nearer of 0 and 1/2 -- for XOR3 exactly 1/4 from both."""
    W = 21
    inp = np.zeros((1, W), np.int32)
    bits = np.array([[(v >> 2) & 1, (v >> 1) & 1, v & 1] for v in range(8)])
    idx = np.where(bits == 1, -2, -1)
    x = _emu_rows(emu, [inp] * 3, idx, [(op, 8)])
    assert not x[:, :W - 1].any()
    phase = x[:, W - 1].astype(np.int64)
    want = np.array([rr.TRUTH[op](int(a), int(b), int(c)) for a, b, c in bits])
    assert np.array_equal((phase > 0).astype(int), want), (op, phase)
    from_zero, from_half = np.abs(phase), HALF - np.abs(phase)
    assert np.array_equal(np.minimum(from_zero, from_half), np.full(8, margin)), (op, phase)
    if op == "XOR3":
        assert np.array_equal(from_zero, from_half)


def _edge_case(rng, B, W, in_rows):
    inp = _random_rows(rng, in_rows, W)
    idx = rng.integers(0, in_rows, (B, 3))
    special = [-1, -2, in_rows, in_rows + 7, -3, 2**31 - 1, -2**31]
    for k, v in enumerate(special[:3 * B]):          # B = 1 takes the first three (-1, -2, in_rows) in one row
        idx[k % B, (k // B) % 3] = v
    if B > 1:
        idx[B - 1] = [2, 2, 2]                       # a repeated row
        idx[1, 2] = in_rows + 7
    return inp, idx.astype(np.int64)


@pytest.mark.parametrize("W", [21, 25])
@pytest.mark.parametrize("B,groups", [
    (1, [("XOR3", 1), ("AND", 0), ("MAJ3N", 0)]),
    (1, [("NOR", 0), ("MAJ3", 1), ("XOR", 0)]),
    (5, [("MAJ3", 2), ("XNOR", 0), ("XOR3", 3)]),
    (5, [("ORNY", 1), ("MAJ3N", 4), ("NAND", 0)]),
    (5, [("XOR3", 0), ("MAJ3N", 1), ("MAJ3", 4)]),
])
def test_per_word_function_equals_the_numpy_restatement(emu, W, B, groups):
    """The function the kernel runs per word, in the kernel's lane placement, against tests/rows_ref.py: three groups (one or two
    empty), indices -1, -2, in_rows, in_rows + 7 and the int32 extremes, a repeated row, W = 21 and 25 (both below one wave)."""
    rng = np.random.default_rng(100 * W + B + len(groups[0][0]))
    in_rows = 4
    inp, idx = _edge_case(rng, B, W, in_rows)
    got = _emu_rows(emu, [inp] * 3, idx, groups)
    assert np.array_equal(got, rr.combine(inp, idx, groups))
    if B == 1:
        assert {-1, -2, in_rows} <= set(idx.ravel().tolist())
    else:
        assert {-1, -2, in_rows, in_rows + 7} <= set(idx.ravel().tolist())


@pytest.mark.parametrize("W", [25, 631])
def test_identity_index_with_three_bases_is_gate3(emu, W):
    """rs_gate3_dev's form: no index table, three base pointers; W = 631 spans ten lane steps with a partial last one."""
    rng = np.random.default_rng(W)
    B = 3
    a, b, c = (_random_rows(rng, B, W) for _ in range(3))
    for op in ("MAJ3", "XOR3", "MAJ3N"):
        got = _emu_rows(emu, [a, b, c], None, [(op, B)])
        coef, _ = rr.COEF[op]
        want = (coef[0] * a.astype(np.int64) + coef[1] * b.astype(np.int64) + coef[2] * c.astype(np.int64)) & 0xFFFFFFFF
        assert np.array_equal(got, want.astype(np.uint32).view(np.int32)), op
        assert np.array_equal(got, rr.combine3(a, b, c, None, [(op, B)])), op


def test_emulated_entry_refuses_what_the_host_refuses(emu):
    inp = np.zeros((1, 21), np.int32)
    out = np.zeros((1, 21), np.int32)
    idx = np.zeros((1, 3), np.int32)
    call = lambda ops, counts, B: emu.rs_emu_gate_rows(_p(inp), _p(inp), _p(inp), 1, _p(idx), _p(np.array(ops, np.int32)),
                                                        (C.c_long * len(counts))(*counts), len(counts), 21, B, _p(out))
    assert call([10], [1], 1) == 0
    assert call([13], [1], 1) == -1 and call([-1], [1], 1) == -1          # op outside 0..12
    assert call([10, 11], [1, 1], 1) == -1 and call([10], [0], 1) == -1   # counts do not sum to B
    assert call([0] * 17, [1] + [0] * 16, 1) == -1                        # more than 16 groups


# ---- redsec_amd/arith.py against a stub backend that evaluates rows on plaintext bits ----
class _StubBackend:
    """gate_rows on noise-free two-word samples (a = 0, b = +-1/8): the combination of tests/rows_ref.py, then the sign of its
    phase instead of a bootstrap. Records every call."""
    W = 2

    def __init__(self):
        self.calls = []

    def gate_rows(self, inp, idx, groups, mu=None, out=None):
        import torch
        assert inp.dtype == torch.int32 and idx.dtype == torch.int32 and idx.is_contiguous() and out.is_contiguous()
        rows = inp.numpy().reshape(-1, self.W).copy()
        index = idx.numpy().reshape(-1, 3).copy()
        assert mu is None and sum(c for _, c in groups) == len(index) and out.shape == (len(index), self.W)
        self.calls.append((index, list(groups), len(rows)))
        x = rr.combine(rows, index, groups)
        assert not x[:, 0].any()
        res = np.zeros_like(x)
        res[:, 1] = np.where(x[:, 1] > 0, E8, -E8)
        out.copy_(torch.from_numpy(res))               # after every read: out may be rows of inp
        return out


def _encode(values, bits):
    import torch
    v = np.asarray(values)
    ct = np.zeros((bits, len(v), 2), np.int32)
    for i in range(bits):
        ct[i, :, 1] = np.where((v >> i) & 1, E8, -E8)
    return torch.from_numpy(ct)


def _decode(ct):
    return (ct.numpy()[..., 1] > 0).astype(np.int64)


def _all_pairs(bits):
    v = np.arange(1 << bits)
    return np.repeat(v, 1 << bits), np.tile(v, 1 << bits)


def test_arith_is_exact_on_all_pairs_of_3_bit_values_against_a_plaintext_stub():
    from redsec_amd import arith
    bits = 3
    xa, xb = _all_pairs(bits)
    B = len(xa)
    a, b = _encode(xa, bits), _encode(xb, bits)
    weights = (1 << np.arange(bits + 1))[:, None]

    be = _StubBackend()
    s = arith.add(be, a, b)
    assert tuple(s.shape) == (bits + 1, B, 2)
    assert np.array_equal((_decode(s) * weights).sum(0), xa + xb)
    assert len(be.calls) == bits
    for bit, (index, groups, in_rows) in enumerate(be.calls):
        assert groups == [("XOR3", B), ("MAJ3", B)] and index.shape == (2 * B, 3)
        assert np.array_equal(index[:B], index[B:])                       # both gates of a lane read the same three rows
        assert ((index[:, :2] >= 0) & (index[:, :2] < in_rows)).all()
        assert (index[:, 2] == -1).all() if bit == 0 else ((index[:, 2] >= 0) & (index[:, 2] < in_rows)).all()
    assert be.calls[0][0] is not be.calls[1][0]

    be = _StubBackend()
    d, borrow = arith.sub(be, a, b)
    assert tuple(d.shape) == (bits, B, 2) and tuple(borrow.shape) == (B, 2)
    assert np.array_equal((_decode(d) * weights[:bits]).sum(0), (xa - xb) % (1 << bits))
    assert np.array_equal(_decode(borrow), (xa < xb).astype(np.int64))
    assert len(be.calls) == bits and all(g == [("XOR3", B), ("MAJ3N", B)] for _, g, _ in be.calls)

    be = _StubBackend()
    lt = arith.less_than(be, a, b)
    assert np.array_equal(_decode(lt), (xa < xb).astype(np.int64))
    assert len(be.calls) == bits and all(g == [("MAJ3N", B)] and len(i) == B for i, g, _ in be.calls)


def test_arith_call_count_is_the_bit_count():
    from redsec_amd import arith
    for bits in (1, 5):
        rng = np.random.default_rng(bits)
        xa, xb = rng.integers(0, 1 << bits, 7), rng.integers(0, 1 << bits, 7)
        be = _StubBackend()
        s = arith.add(be, _encode(xa, bits), _encode(xb, bits))
        assert len(be.calls) == bits
        assert np.array_equal((_decode(s) * (1 << np.arange(bits + 1))[:, None]).sum(0), xa + xb)


# ---- exports ----
def test_row_symbols_are_exported_and_documented():
    import redsec_amd
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    L = redsec_amd.load_library()
    for sym in ("rs_gate3_dev", "rs_gate_rows_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and re.search(r"\bint %s\(rs_ctx\* ctx" % sym, header) and hasattr(L, sym)
    assert "typedef struct rs_row_group { int32_t op; int32_t reserved; uint64_t count; } rs_row_group;" in header
    for f in ("gate3", "gate_rows"):
        assert callable(getattr(redsec_amd.Backend, f))
    # the binding's name table follows the two enums of the header
    enum = dict((k, int(v)) for k, v in re.findall(r"\bRS_ROW_([A-Z0-9]+)\s*=\s*(\d+)", header))
    assert enum == {"MAJ3": 10, "XOR3": 11, "MAJ3N": 12}
    gates = dict((k, int(v)) for k, v in re.findall(r"\bRS_([A-Z]+) = (\d+)", header[header.index("typedef enum rs_gate_op"):header.index("} rs_gate_op;")]))
    assert redsec_amd.ROW_OPS == dict(gates, **enum) and len(redsec_amd.ROW_OPS) == 13
    assert [redsec_amd.ROW_OPS[n] for n in rr.OPS] == list(range(13))
    from redsec_amd import backend
    assert C.sizeof(backend.RsRowGroup) == 16 and backend.RsRowGroup.count.offset == 8


def test_no_cpu_fallback_for_the_row_calls():
    """Without a device nothing computes and the reason is said: RS_ERR_NO_DEVICE (no context can exist: rs_create refuses). With a
    device the same null-context calls are plain argument errors."""
    import torch
    import redsec_amd
    from redsec_amd import backend
    L = redsec_amd.load_library()
    want = -1 if torch.cuda.is_available() else -2
    buf = np.zeros((1, 631), np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    g = (backend.RsRowGroup * 1)()
    g[0].op, g[0].count = 10, 1
    assert L.rs_gate3_dev(None, 10, p, p, p, p, 1, None) == want
    assert L.rs_gate_rows_dev(None, p, p, 1, p, g, 1, E8, 1, None) == want
    if want == -2:
        assert b"no HIP device" in L.rs_last_error()
    assert np.array_equal(buf, np.zeros_like(buf))


def test_the_row_kernel_is_plain_cpp_in_an_object_of_its_own():
    from redsec_amd import build
    assert ("rs_rows", "rs_rows.hip", []) in build.HIP_OBJECTS and "rs_rows.h" in build.HIP_DEPS and "rs_rows.h" in build.EMU_DEPS
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_rows.hip", "rs_rows.h"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\basm\b|__shared__|\batomic|\b(double|float)\b", code), f
