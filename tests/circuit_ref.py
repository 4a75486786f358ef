"""Independent numpy restatement of the compiled circuits (include/redsec_hip.h rs_circuit_create / rs_circuit_run_dev;
INTEGRATION.md section 15). TEST INFRASTRUCTURE ONLY.

  stage_level       the combinations one level stages, as circuit_rows_kernel lays them out
  oracle_wires      a gate-by-gate evaluator in NETLIST order on the EXISTING oracle: ctx.bootstrap_batch(x, 1/8) for cells 0..12,
                    ctx.mux_batch on the (negated) sources for MUX
  StubBackend       circuit_create / circuit_run on noise-free two-word samples, level by level, the sign of a phase for a bootstrap
A cell's words depend only on its source words, never on the schedule: the evaluator's wires equal the device's, whatever the
levelisation."""
import numpy as np

import rows_ref as rr

E8 = 1 << 29
MUX = 13
OPS = rr.OPS + ["MUX"]
TRUTH = dict(rr.TRUTH, MUX=lambda a, b, c: (a & b) | ((1 - a) & c))
CELL = np.dtype([("src", np.int32, (3,)), ("op", np.uint8), ("neg", np.uint8), ("reserved", np.uint16)])   # rs_cell


def wrap(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def coef(op, neg, second=False):
    """((c0, c1, c2), bconst) of a cell's combination: rs_rows.h's table for 0..12, TFHE's bootsMUX pair for 13; bit j of neg flips c_j"""
    if op == MUX:
        c, bconst = ((-1, 0, 1), -E8) if second else ((1, 1, 0), -E8)
    else:
        assert not second
        c, bconst = rr.COEF[rr.OPS[op]]
    return tuple(-cj if (neg >> j) & 1 else cj for j, cj in enumerate(c)), bconst


def trivial(bit, L, W):
    out = np.zeros((L, W), np.int64)
    out[:, W - 1] = E8 if bit else -E8
    return out


def source(arena, src):
    """int64 [L][W]: the rows of wire src, or the trivial sample of -1 (FALSE) / -2 (TRUE)"""
    _, L, W = arena.shape
    assert src >= -2
    return trivial(src == -2, L, W) if src < 0 else arena[src].astype(np.int64)


def combination(arena, cell, second=False):
    """int32 [L][W]: what the pre-pass stages for one cell"""
    c, bconst = coef(int(cell["op"]), int(cell["neg"]), second)
    x = sum(cj * source(arena, int(cell["src"][j])) for j, cj in enumerate(c) if cj != 0)
    x = x + np.zeros(arena.shape[1:], np.int64)
    x[:, -1] += bconst
    return wrap(x)


def stage_level(arena, table, first, C, M):
    """int32 [(C + M) L][W]: the C cells' own rows, cell-major, then the second combinations of the last M (MUX) cells"""
    rows = [combination(arena, table[first + k]) for k in range(C)]
    rows += [combination(arena, table[first + k], second=True) for k in range(C - M, C)]
    return np.concatenate(rows)


def fold(u, B, mux_rows):
    """the extracted samples after circuit_fold_kernel"""
    u = u.astype(np.int64)
    u[B - mux_rows:B] += u[B:B + mux_rows]
    u[B - mux_rows:B, -1] += E8
    return wrap(u)


def _negated(x, neg):
    return wrap(-x) if neg else wrap(x)


def oracle_wires(ctx, nl, inputs):
    """{netlist node: int32 [L][W]} of every gate an output depends on, evaluated in netlist order on the oracle. inputs [n_in][L][W]."""
    inputs = np.asarray(inputs, np.int32)
    n_in, L, W = inputs.shape
    live, stack = set(), [w.node for w in nl.outputs if w.node >= n_in]
    while stack:
        node = stack.pop()
        if node not in live:
            live.add(node)
            stack.extend(s.node for s in nl.gates[node - n_in][1] if s is not None and s.node >= n_in)
    value = {i: inputs[i] for i in range(n_in)}

    def read(s):
        """(rows int64, negated) of a handle; a constant's polarity picks the sample"""
        if s.node < 0:
            return trivial(s.neg, L, W), False
        return value[s.node].astype(np.int64), s.neg
    for node in sorted(live):
        op, srcs = nl.gates[node - n_in]
        if op == MUX:
            a, b, c = (_negated(*read(s)) for s in srcs)
            value[node] = ctx.mux_batch(a, b, c)
        else:
            c, bconst = rr.COEF[rr.OPS[op]]
            x = np.zeros((L, W), np.int64)
            for cj, s in zip(c, srcs):
                if cj != 0:
                    rows, neg = read(s)
                    x += (-cj if neg else cj) * rows
            x[:, -1] += bconst
            value[node] = ctx.bootstrap_batch(wrap(x), E8)
    return {node: value[node] for node in live}


def expected_arena(plan, inputs, wires):
    """the arena rs_circuit_run_dev leaves: the inputs, then every cell's rows at its wire"""
    inputs = np.asarray(inputs, np.int32)
    arena = np.zeros((plan.wires,) + inputs.shape[1:], np.int32)
    arena[:plan.n_inputs] = inputs
    for node, w in plan.wire_of.items():
        arena[w] = wires[node]
    return arena


class StubBackend:
    """The circuit calls of Backend on noise-free two-word samples (a = 0, b = +-1/8), on CPU tensors: a level's staged rows are
    restated above, a bootstrap is the sign of the phase, a MUX the sign of u1 + u2 + 1/8. Records the levels it ran."""
    W = 2
    closed = False

    def __init__(self):
        self.circuits, self.levels, self.runs = {}, [], 0

    def circuit_create(self, table, level_end, n_inputs):
        h = len(self.circuits) + 1
        self.circuits[h] = (np.array(table, CELL), [int(e) for e in level_end], int(n_inputs))
        return h

    def circuit_destroy(self, h):
        del self.circuits[h]

    def circuit_run(self, h, arena, lanes):
        import torch
        table, level_end, n_inputs = self.circuits[h]
        a = arena.numpy().reshape(n_inputs + len(table), lanes, self.W)
        sign = lambda x: np.where(x > 0, E8, -E8).astype(np.int64)
        lo = 0
        self.runs += 1
        for hi in level_end:
            C = hi - lo
            M = int((table["op"][lo:hi] == MUX).sum())
            x = stage_level(a, table, lo, C, M)
            assert not x[:, 0].any()
            u = sign(x[:, 1])
            B = C * lanes
            u[B - M * lanes:B] = sign(wrap(u[B - M * lanes:B] + u[B:] + E8))
            a[n_inputs + lo:n_inputs + hi, :, 0] = 0
            a[n_inputs + lo:n_inputs + hi, :, 1] = u[:B].reshape(C, lanes)
            self.levels.append((C, M))
            lo = hi
        assert torch.from_numpy(a).data_ptr() == arena.data_ptr()
        return arena

    def lincomb(self, a, ca, b=None, cb=0, bconst=0):
        import torch
        assert b is None and bconst == 0
        return torch.from_numpy(wrap(a.numpy().astype(np.int64) * ca))


def encode(bits):
    """0/1 array [...] -> noise-free two-word samples int32 [...][2]"""
    bits = np.asarray(bits)
    out = np.zeros(bits.shape + (2,), np.int32)
    out[..., 1] = np.where(bits == 1, E8, -E8)
    return out


def decode(ct):
    return (np.asarray(ct)[..., 1] > 0).astype(np.int64)
