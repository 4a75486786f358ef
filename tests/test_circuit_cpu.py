"""Compiled circuits without a GPU (include/redsec_hip.h rs_circuit_create / rs_circuit_run_dev): the
kernels' own per-word function and the host validation of csrc/rs_circuit.h (compiled into the lane emulator) against the numpy
restatement (tests/circuit_ref.py), the noise-free truth tables of every op and neg pattern, the compiler and the generators of
redsec_amd/circuit.py against a plaintext stub backend, and the exports. Nothing here bootstraps: there is no CPU fallback."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import circuit_ref as cr
import rows_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
E8 = 1 << 29


@pytest.fixture(scope="module")
def emu():
    from redsec_amd import build
    L = C.CDLL(build.build_emulator())
    L.rs_emu_circuit_check.argtypes = [C.c_void_p, C.c_size_t, _u32p, C.c_size_t, C.c_size_t]
    L.rs_emu_circuit_rows.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_long, _i32p, C.c_int, _i32p]
    L.rs_emu_circuit_fold.argtypes = [_i32p, C.c_long, C.c_long, C.c_int]
    return L


def _table(cells):
    """[(op, (s0, s1, s2), neg[, reserved])] -> rs_cell array"""
    t = np.zeros(len(cells), cr.CELL)
    for i, (op, src, neg, *reserved) in enumerate(cells):
        t["op"][i], t["src"][i], t["neg"][i], t["reserved"][i] = op, src, neg, reserved[0] if reserved else 0
    return t


def _check(L, cells, level_end, n_inputs, n_cells=None):
    t = _table(cells)
    ends = np.array(level_end, np.uint32)
    return L.rs_emu_circuit_check(t.ctypes.data_as(C.c_void_p), len(t) if n_cells is None else n_cells, ends.ctypes.data_as(_u32p),
                                  len(ends), n_inputs)


def _emu_level(L, arena, table, first, Cn, M):
    arena = np.ascontiguousarray(arena, np.int32)
    _, lanes, W = arena.shape
    out = np.full(((Cn + M) * lanes, W), 0x5a5a5a5a, np.int32)
    assert L.rs_emu_circuit_rows(table.ctypes.data_as(C.c_void_p), first, Cn, M, lanes, arena.ctypes.data_as(_i32p), W,
                                 out.ctypes.data_as(_i32p)) == 0
    return out


# ---- the per-word function ----
@pytest.mark.parametrize("W", [21, 25])
def test_per_word_function_equals_the_numpy_restatement(emu, W):
    """Random words, all 14 ops x all 8 neg patterns, both constants among the sources, three lanes; the level sits behind three
    cells of an earlier one, so `first` and wires of cells are exercised. Then the fold."""
    rng = np.random.default_rng(W)
    n_in, lanes = 4, 3
    early = [(2, (0, 1, -1), 0), (13, (1, 2, 3), 5), (13, (-2, 0, 1), 0)]
    pool = list(range(n_in + len(early))) + [-1, -2]
    cells = list(early)
    for op in range(14):                       # MUX (13) last: the level's MUX cells follow its other cells
        for neg in range(8):
            src = tuple(int(s) for s in rng.choice(pool, 3))
            cells.append((op, src, neg))
    cells[len(early)] = (0, (-1, -2, 0), 0)    # both constants in one cell, and in a MUX cell
    cells[-1] = (13, (-2, -1, 3), 7)
    table = _table(cells)
    Cn, M = 14 * 8, 8
    assert emu.rs_emu_circuit_check(table.ctypes.data_as(C.c_void_p), len(table), np.array([3, len(table)], np.uint32).ctypes.data_as(_u32p), 2, n_in) == 0
    arena = rng.integers(-2**31, 2**31, (n_in + len(table), lanes, W)).astype(np.int32)
    got = _emu_level(emu, arena, table, len(early), Cn, M)
    assert np.array_equal(got, cr.stage_level(arena, table, len(early), Cn, M))
    first_level = _emu_level(emu, arena, table, 0, 3, 2)
    assert np.array_equal(first_level, cr.stage_level(arena, table, 0, 3, 2)) and first_level.shape[0] == 5 * lanes
    # the fold on random extracted samples of 1025 words (17 lane steps with a partial last one)
    B, mux_rows, words = Cn * lanes, M * lanes, 1025
    u = rng.integers(-2**31, 2**31, (B + mux_rows, words)).astype(np.int32)
    want = cr.fold(u, B, mux_rows)
    assert emu.rs_emu_circuit_fold(u.ctypes.data_as(_i32p), B, mux_rows, words) == 0
    assert np.array_equal(u, want)


@pytest.mark.parametrize("W", [21, 25])
def test_cells_without_neg_bits_are_the_rows_of_gate_rows(emu, W):
    """Ops 0..12 with neg = 0: the staged words are those of rs_gate_rows_dev's combination (tests/rows_ref.py) on the same rows."""
    rng = np.random.default_rng(7 * W)
    n_in, lanes = 5, 2
    pool = list(range(n_in)) + [-1, -2]
    cells = [(op, tuple(int(s) for s in rng.choice(pool, 3)), 0) for op in range(13)]
    table = _table(cells)
    arena = rng.integers(-2**31, 2**31, (n_in + 13, lanes, W)).astype(np.int32)
    got = _emu_level(emu, arena, table, 0, 13, 0)
    idx = np.array([[s * lanes + lane if s >= 0 else s for s in src] for _, src, _ in cells for lane in range(lanes)])
    groups = [(rr.OPS[op], lanes) for op, _, _ in cells]
    assert np.array_equal(got, rr.combine(arena.reshape(-1, W), idx, groups))


# ---- truth tables ----
@pytest.mark.parametrize("op", range(14))
def test_truth_tables_of_every_neg_pattern_noise_free(emu, op):
    """Two-word samples, the eight input combinations as lanes, all eight neg patterns: the staged phase has the sign of the op on
    the negated inputs; MUX's two combinations are checked by the sign of u1 + u2 + 1/8. A neg bit on an unread source changes
    nothing."""
    v = np.arange(8)
    bits = np.stack([(v >> 2) & 1, (v >> 1) & 1, v & 1])
    arena = np.zeros((4, 8, 2), np.int32)
    arena[:3] = cr.encode(bits)
    name = cr.OPS[op]
    sign = lambda x: np.where(x > 0, E8, -E8).astype(np.int64)
    for neg in range(8):
        table = _table([(op, (0, 1, 2), neg)])
        M = 1 if op == cr.MUX else 0
        x = _emu_level(emu, arena, table, 0, 1, M)
        assert not x[:, 0].any()
        flipped = [bits[j] ^ ((neg >> j) & 1) for j in range(3)]
        want = cr.TRUTH[name](*flipped)
        if M:
            phase = cr.wrap(sign(x[:8, 1]) + sign(x[8:, 1]) + E8)
        else:
            phase = x[:, 1]
            if op < 10:
                assert np.array_equal(x, _emu_level(emu, arena, _table([(op, (0, 1, 2), neg & 3)]), 0, 1, 0))
        assert np.array_equal((phase > 0).astype(int), want), (name, neg)
        # the same with constants for sources: a negated constant is the other constant
        for lane in range(8):
            consts = tuple(-2 if bits[j][lane] else -1 for j in range(3))
            y = _emu_level(emu, arena[:, :1], _table([(op, consts, neg)]), 0, 1, M)
            assert np.array_equal(y[:, 1], x[lane::8, 1]), (name, neg, lane)


# ---- validation ----
def test_validation_refuses_what_rs_circuit_create_refuses(emu):
    ok = [(2, (0, 1, -1), 0), (11, (0, 1, -2), 3), (13, (0, 1, 2), 0), (0, (3, 4, 5), 0), (13, (5, 3, 0), 1)]
    assert _check(emu, ok, [3, 5], 3) == 0
    assert _check(emu, ok[:2], [2], 3) == 0                                    # a plan without MUX
    assert _check(emu, [ok[2], (13, (3, 0, 1), 2)], [1, 2], 3) == 0           # levels of only MUX cells
    t = _table(ok)
    ends = np.array([3, 5], np.uint32)
    pt, pe = t.ctypes.data_as(C.c_void_p), ends.ctypes.data_as(_u32p)
    assert emu.rs_emu_circuit_check(None, 5, pe, 2, 3) == -1 and emu.rs_emu_circuit_check(pt, 5, None, 2, 3) == -1     # null pointers
    assert emu.rs_emu_circuit_check(pt, 5, pe, 0, 3) == -1                    # n_levels = 0
    assert _check(emu, ok, [0, 5], 3) == -1 and _check(emu, ok, [3, 3, 5], 3) == -1      # an empty level
    assert _check(emu, ok, [4, 3, 5], 3) == -1                                # level_end not increasing
    assert _check(emu, ok, [3, 4], 3) == -1 and _check(emu, ok, [3, 6], 3) == -1 and _check(emu, ok, [3, 5], 3, n_cells=4) == -1   # last != n_cells
    assert _check(emu, ok, [6, 5], 3) == -1                                   # a cut past n_cells
    for bad_op in (14, 255):
        assert _check(emu, [(bad_op, (0, 1, 2), 0)], [1], 3) == -1            # op outside 0..13
    assert _check(emu, [(2, (0, 1, 2), 0, 1)], [1], 3) == -1                  # reserved != 0
    assert _check(emu, [(2, (0, -3, 2), 0)], [1], 3) == -1 and _check(emu, [(2, (0, 1, -2**31), 0)], [1], 3) == -1     # src below -2
    assert _check(emu, [(2, (0, 1, 3), 0)], [1], 3) == -1                     # itself
    assert _check(emu, ok[:3] + [(0, (3, 4, 6), 0), ok[4]], [3, 5], 3) == -1  # a cell of its own level
    assert _check(emu, ok[:3] + [(0, (3, 4, 7), 0), ok[4]], [3, 5], 3) == -1  # a later cell
    assert _check(emu, ok[:3] + [(0, (3, 4, 8), 0), ok[4]], [3, 5], 3) == -1  # no wire at all
    assert _check(emu, [(4, (0, 1, 3), 0)], [1], 3) == -1                     # ... also at a source the op does not read
    assert _check(emu, [ok[0], ok[2], ok[1]], [3], 3) == -1                   # a MUX cell followed by another op in its level
    assert _check(emu, [ok[2], ok[0]], [1, 2], 3) == 0                        # ... which the next level may hold
    assert _check(emu, ok[:1], [1], 2**31 - 1) == -1                          # wires past int32
    assert _check(emu, ok[:1], [1], 2**31 - 2) == 0
    assert _check(emu, ok[:1], [1], 2**40) == -1


# ---- the compiler ----
def _random_netlist(rng):
    from redsec_amd import circuit
    n_in = int(rng.integers(1, 7))
    nl = circuit.Netlist(n_in)
    wires = nl.inputs()

    def pick():
        k = rng.integers(0, 10)
        if k == 0:
            return nl.const(int(rng.integers(0, 2)))
        w = wires[int(rng.integers(0, len(wires)))]
        return nl.not_(w) if rng.integers(0, 3) == 0 else w
    for _ in range(int(rng.integers(0, 61))):
        op = int(rng.integers(0, 14))
        wires.append(nl.gate(op, pick(), pick(), pick() if op >= 10 else None))
    for _ in range(int(rng.integers(1, 6))):
        nl.output(pick())
    return nl


def _live_and_depth(nl):
    """the gates some output depends on and the longest path to an output counted in gates, worked out recursively here"""
    n_in = nl.n_inputs
    memo = {}

    def depth(node):
        if node < n_in:
            return 0
        if node not in memo:
            memo[node] = 1 + max(depth(s.node) for s in nl.gates[node - n_in][1] if s is not None)
        return memo[node]
    deepest = max([depth(w.node) for w in nl.outputs], default=0)
    return set(memo), deepest


def test_compiler_on_200_random_netlists(emu):
    from redsec_amd import circuit
    rng = np.random.default_rng(17)
    seen_mux_only = seen_dead = seen_neg = 0
    for case in range(200):
        nl = _random_netlist(rng)
        plan = nl.compile()
        live, deepest = _live_and_depth(nl)
        assert plan.cells == len(live) and plan.depth == deepest, case
        seen_dead += plan.cells < len(nl.gates)
        seen_neg += bool(plan.table["neg"].any())
        assert plan.rotations == plan.cells + sum(1 for node in live if nl.gates[node - nl.n_inputs][0] == 13)
        assert plan.table.dtype == cr.CELL and plan.table.dtype.itemsize == 16
        bits = rng.integers(0, 2, (nl.n_inputs, 5))
        want = nl.evaluate(bits)
        if plan.cells:
            assert emu.rs_emu_circuit_check(plan.table.ctypes.data_as(C.c_void_p), plan.cells, plan.level_end.ctypes.data_as(_u32p),
                                            plan.depth, plan.n_inputs) == 0, case
            level_of = np.zeros(plan.wires, np.int64)
            for v, (first, cells, mux) in enumerate(plan.levels()):
                level_of[plan.n_inputs + first:plan.n_inputs + first + cells] = v + 1
                ops = plan.table["op"][first:first + cells]
                assert (ops[:cells - mux] != 13).all() and (ops[cells - mux:] == 13).all(), case
                seen_mux_only += mux == cells
            for i, cell in enumerate(plan.table):
                srcs = [int(s) for s in cell["src"]]
                assert all(s >= -2 for s in srcs)
                here = level_of[plan.n_inputs + i]
                assert all(level_of[s] < here for s in srcs if s >= 0), case
                assert here == 1 + max([level_of[s] for s in srcs if s >= 0], default=0), case      # as soon as possible
        import torch
        be = cr.StubBackend()
        got = plan.bind(be).run(torch.from_numpy(cr.encode(bits)))
        assert np.array_equal(cr.decode(got.numpy()), want), case
        assert be.levels == [(c, m) for _, c, m in plan.levels()] and be.runs == (1 if plan.cells else 0)
    assert seen_mux_only and seen_dead and seen_neg


def test_not_creates_no_cell_and_polarities_become_neg_bits():
    from redsec_amd import circuit
    nl = circuit.Netlist(2)
    a, b = nl.inputs()
    g = nl.gate("AND", nl.not_(a), b)
    assert len(nl.gates) == 1
    nl.output(nl.not_(g))
    nl.output(nl.not_(nl.not_(a)))
    nl.output(nl.const(1))
    nl.output(nl.not_(nl.const(1)))
    nl.output(nl.mux(nl.not_(g), nl.const(1), nl.not_(nl.const(1))))
    plan = nl.compile()
    assert plan.cells == 2 and plan.depth == 2 and plan.rotations == 3
    assert plan.table["neg"].tolist() == [1, 1] and plan.table["src"].tolist() == [[0, 1, -1], [2, -2, -1]]
    assert plan.outputs == [(2, 1), (0, 0), (-2, 0), (-1, 0), (3, 0)]
    bits = np.array([[0, 0, 1, 1], [0, 1, 0, 1]])
    assert np.array_equal(nl.evaluate(bits), [[1, 0, 1, 1], [0, 0, 1, 1], [1] * 4, [0] * 4, [1, 0, 1, 1]])


# ---- the generators, exhaustively at 3 bits ----
def _bits_of(values, bits):
    return np.stack([(np.asarray(values) >> i) & 1 for i in range(bits)])


def _number(rows):
    return sum(rows[i].astype(np.int64) << i for i in range(len(rows)))


def _run_stub(nl, bits):
    import torch
    be = cr.StubBackend()
    out = cr.decode(nl.compile().bind(be).run(torch.from_numpy(cr.encode(bits))).numpy())
    assert np.array_equal(out, nl.evaluate(bits))
    return out


def test_generators_exhaustively_at_3_bits_on_the_stub():
    from redsec_amd import circuit
    bits = 3
    v = np.arange(1 << bits)
    xa, xb = np.repeat(v, 1 << bits), np.tile(v, 1 << bits)
    ab = np.concatenate([_bits_of(xa, bits), _bits_of(xb, bits)])
    assert np.array_equal(_number(_run_stub(circuit.adder(bits), ab)), xa + xb)
    d = _run_stub(circuit.subtractor(bits), ab)
    assert np.array_equal(_number(d[:bits]), (xa - xb) % 8) and np.array_equal(d[bits], xa < xb)
    assert np.array_equal(_run_stub(circuit.less_than(bits), ab)[0], xa < xb)
    assert np.array_equal(_run_stub(circuit.equal(bits), ab)[0], xa == xb)
    assert np.array_equal(_number(_run_stub(circuit.maximum(bits), ab)), np.maximum(xa, xb))
    assert np.array_equal(_number(_run_stub(circuit.multiplier(bits), ab)), xa * xb)
    for cond in (0, 1):
        sel = _run_stub(circuit.select(bits), np.concatenate([np.full((1, len(xa)), cond), ab]))
        assert np.array_equal(_number(sel), xa if cond else xb)
    mul = circuit.multiplier(bits).compile()
    assert mul.cells == bits * bits + 2 * bits * (bits - 1) and mul.depth < mul.cells and mul.rotations == mul.cells
    sel = circuit.select(bits).compile()
    assert (sel.cells, sel.rotations, sel.depth) == (bits, 2 * bits, 1)
    mx = circuit.maximum(bits).compile()
    assert (mx.cells, mx.rotations, mx.depth) == (2 * bits, 3 * bits, bits + 1)
    assert circuit.adder(bits).compile().depth == bits and circuit.adder(bits).compile().cells == 2 * bits
    assert circuit.equal(4).compile().depth == 3
    for one in (circuit.multiplier(1), circuit.equal(1), circuit.maximum(1)):
        pairs = np.array([[0, 0, 1, 1], [0, 1, 0, 1]])
        _run_stub(one, pairs)
    assert np.array_equal(_number(_run_stub(circuit.multiplier(1), np.array([[0, 0, 1, 1], [0, 1, 0, 1]]))), [0, 0, 0, 1])


def test_arith_functions_through_cached_plans_on_the_stub():
    import torch
    from redsec_amd import arith
    bits = 3
    v = np.arange(1 << bits)
    xa, xb = np.repeat(v, 1 << bits), np.tile(v, 1 << bits)
    enc = lambda x: torch.from_numpy(cr.encode(_bits_of(x, bits)))
    a, b = enc(xa), enc(xb)
    be = cr.StubBackend()
    assert np.array_equal(_number(cr.decode(arith.multiply(be, a, b).numpy())), xa * xb)
    assert np.array_equal(_number(cr.decode(arith.maximum(be, a, b).numpy())), np.maximum(xa, xb))
    eq = arith.equal(be, a, b)
    assert tuple(eq.shape) == (len(xa), 2) and np.array_equal(cr.decode(eq.numpy()), xa == xb)
    cond = torch.from_numpy(cr.encode(xa < xb))
    assert np.array_equal(_number(cr.decode(arith.select(be, cond, a, b).numpy())), np.where(xa < xb, xa, xb))
    assert len(be.circuits) == 4 and be.runs == 4
    arith.multiply(be, a, b)
    arith.maximum(be, a[:, :5].contiguous(), b[:, :5].contiguous())          # another lane count: the same plan
    assert len(be.circuits) == 4 and be.runs == 6


# ---- exports ----
def test_circuit_symbols_are_exported_and_documented():
    import redsec_amd
    from redsec_amd import backend
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    L = redsec_amd.load_library()
    for sym in ("rs_circuit_create", "rs_circuit_destroy", "rs_circuit_run_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and re.search(r"\bint %s\(rs_ctx\* ctx" % sym, header) and hasattr(L, sym)
    assert "typedef enum rs_cell_op { RS_CELL_MUX = 13 } rs_cell_op;" in header
    assert "typedef struct rs_cell { int32_t src[3]; uint8_t op; uint8_t neg; uint16_t reserved; } rs_cell;" in header
    assert "typedef struct rs_circuit rs_circuit;" in header
    assert C.sizeof(backend.RsCell) == 16 and backend.CELL_DTYPE.itemsize == 16 and backend.CELL_DTYPE == cr.CELL
    assert (backend.RsCell.op.offset, backend.RsCell.neg.offset, backend.RsCell.reserved.offset) == (12, 13, 14)
    assert backend.CELL_OPS == dict(backend.ROW_OPS, MUX=13) and [backend.CELL_OPS[n] for n in cr.OPS] == list(range(14))
    for f in ("circuit_create", "circuit_destroy", "circuit_run"):
        assert callable(getattr(redsec_amd.Backend, f))
    # the row interface keeps its table: three names, thirteen ops
    assert dict(re.findall(r"\bRS_ROW_([A-Z0-9]+)\s*=\s*(\d+)", header)) == {"MAJ3": "10", "XOR3": "11", "MAJ3N": "12"}
    assert len(redsec_amd.ROW_OPS) == 13


def test_no_cpu_fallback_for_the_circuit_calls():
    """Without a device nothing computes and the reason is said: RS_ERR_NO_DEVICE. With one, null-context calls are argument errors."""
    import torch
    import redsec_amd
    L = redsec_amd.load_library()
    want = -1 if torch.cuda.is_available() else -2
    table = _table([(2, (0, 1, -1), 0)])
    ends = np.array([1], np.uint32)
    h = C.c_void_p()
    buf = np.zeros((3, 631), np.int32)
    assert L.rs_circuit_create(None, C.byref(h), table.ctypes.data_as(C.c_void_p), 1, ends.ctypes.data_as(_u32p), 1, 2) == want
    assert not h.value
    if want == -2:
        assert b"no HIP device" in L.rs_last_error()
    assert L.rs_circuit_run_dev(None, None, buf.ctypes.data_as(C.c_void_p), 1, None) == want
    assert L.rs_circuit_destroy(None, None) == want
    assert not buf.any()


def test_the_circuit_kernels_are_plain_cpp_in_an_object_of_their_own():
    from redsec_amd import build
    assert ("rs_circuit", "rs_circuit.hip", []) in build.HIP_OBJECTS
    assert "rs_circuit.h" in build.HIP_DEPS and "rs_circuit.h" in build.EMU_DEPS and "rs_circuit.hip" in build.HIP_SOURCES
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_circuit.hip", "rs_circuit.h"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\basm\b|__shared__|\batomic|\b(double|float)\b", code), f
    # the kernels live in rs_circuit.hip alone; the row files do not know them
    for f in ("rs_rows.hip", "rs_rows.h"):
        assert "circuit" not in open(os.path.join(csrc, f)).read()
