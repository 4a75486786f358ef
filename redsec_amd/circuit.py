"""Boolean netlists compiled into levelised cell tables for rs_circuit_run_dev.

A Netlist is a list of gates over wire handles. A handle carries a polarity, so `not_` creates no gate: the negation becomes a
`neg` bit of every cell that reads the wire (a sign flip of that source's coefficient), or one lincomb(-1) when the wire is an
output. `compile()` drops the gates no output depends on, puts every live gate at level 1 + the largest level of its sources
(inputs and constants are level 0), orders each level non-MUX first and numbers the wires; the Plan it returns does not depend on
the lane count. `Plan.bind(be).run(inputs)` lays the arena out and makes ONE call of Backend.circuit_run: one bootstrap batch per
level. Nothing here computes on ciphertext words.

Generators (inputs LSB first; two operands a then b): adder, subtractor, less_than, equal, select, maximum, multiplier.
"""
import numpy as np

from .backend import CELL_DTYPE, CELL_OPS

E8 = 1 << 29
_OP_NAMES = sorted(CELL_OPS, key=CELL_OPS.get)
_ARITY = [2] * 10 + [3] * 4
_TRUTH = [
    lambda a, b, c: 1 - (a & b), lambda a, b, c: a | b, lambda a, b, c: a & b, lambda a, b, c: 1 - (a | b),
    lambda a, b, c: a ^ b, lambda a, b, c: 1 - (a ^ b), lambda a, b, c: (1 - a) & b, lambda a, b, c: a & (1 - b),
    lambda a, b, c: (1 - a) | b, lambda a, b, c: a | (1 - b),
    lambda a, b, c: (a & b) | (a & c) | (b & c), lambda a, b, c: a ^ b ^ c, lambda a, b, c: ((1 - a) & b) | ((1 - a) & c) | (b & c),
    lambda a, b, c: (a & b) | ((1 - a) & c),
]
_CONST = -1      # node of the constant FALSE; TRUE is its negation


class Wire:
    """A node of a netlist with a polarity. node: an input (0 .. n_inputs-1), a gate (n_inputs + its position), or the constant."""
    __slots__ = ("node", "neg")

    def __init__(self, node, neg=False):
        self.node, self.neg = int(node), bool(neg)

    def __invert__(self):
        return Wire(self.node, not self.neg)

    def __repr__(self):
        return "%sw%d" % ("~" if self.neg else "", self.node)


class Netlist:
    def __init__(self, n_inputs):
        self.n_inputs = int(n_inputs)
        self.gates = []          # (op number, (Wire, Wire, Wire or None))
        self.outputs = []

    def input(self, i):
        assert 0 <= i < self.n_inputs
        return Wire(i)

    def inputs(self, first=0, count=None):
        return [Wire(i) for i in range(first, first + (self.n_inputs - first if count is None else count))]

    def const(self, bit):
        return Wire(_CONST, bool(bit))

    def not_(self, a):
        return ~a

    def gate(self, op, a, b=None, c=None):
        """op: a name or number of CELL_OPS (0..9 two inputs, 10..13 three) -> the wire of the new gate."""
        op = CELL_OPS[op] if isinstance(op, str) else int(op)
        assert 0 <= op < len(_ARITY), "unknown op"
        srcs = (a, b, c)
        assert all(isinstance(s, Wire) for s in srcs[:_ARITY[op]]) and (c is None or _ARITY[op] == 3), "op %s takes %d wires" % (_OP_NAMES[op], _ARITY[op])
        for s in srcs[:_ARITY[op]]:
            assert s.node < self.n_inputs + len(self.gates), "wire of another netlist"
        self.gates.append((op, srcs))
        return Wire(self.n_inputs + len(self.gates) - 1)

    def mux(self, a, b, c):
        """a ? b : c"""
        return self.gate("MUX", a, b, c)

    def output(self, w):
        self.outputs.append(w)
        return w

    def evaluate(self, bits):
        """The outputs on plaintext: bits [n_inputs] or [n_inputs][L] of 0/1 -> int64 [n_out] or [n_out][L]."""
        bits = np.asarray(bits, np.int64)
        assert bits.shape[0] == self.n_inputs
        zero = np.zeros(bits.shape[1:], np.int64)
        value = list(bits)

        def read(w):
            if w is None:
                return zero
            v = zero if w.node == _CONST else value[w.node]
            return 1 - v if w.neg else v
        for op, srcs in self.gates:
            value.append(_TRUTH[op](*(read(s) for s in srcs)))
        return np.stack([read(w) for w in self.outputs]) if self.outputs else np.zeros((0,) + bits.shape[1:], np.int64)

    def compile(self):
        n_in = self.n_inputs
        live = set()
        stack = [w.node for w in self.outputs if w.node >= n_in]
        while stack:
            node = stack.pop()
            if node in live:
                continue
            live.add(node)
            stack.extend(s.node for s in self.gates[node - n_in][1] if s is not None and s.node >= n_in)
        level = {}
        for node in sorted(live):                    # netlist order is a topological order
            srcs = self.gates[node - n_in][1]
            level[node] = 1 + max([level[s.node] for s in srcs if s is not None and s.node >= n_in], default=0)
        is_mux = lambda node: self.gates[node - n_in][0] == CELL_OPS["MUX"]
        order = sorted(live, key=lambda node: (level[node], is_mux(node), node))
        wire = {node: n_in + i for i, node in enumerate(order)}

        def source(s):
            """(src, neg bit) of a handle: constants fold their polarity into the index"""
            if s is None:
                return -1, 0
            if s.node == _CONST:
                return (-2 if s.neg else -1), 0
            return (wire[s.node] if s.node >= n_in else s.node), int(s.neg)
        table = np.zeros(len(order), CELL_DTYPE)
        for i, node in enumerate(order):
            op, srcs = self.gates[node - n_in]
            table["op"][i] = op
            for j, s in enumerate(srcs):
                table["src"][i, j], bit = source(s)
                table["neg"][i] |= bit << j
        depth = max(level.values(), default=0)
        level_end = np.array([sum(1 for node in order if level[node] <= v) for v in range(1, depth + 1)], np.uint32)
        return Plan(n_in, table, level_end, [source(w) for w in self.outputs], wire)


class Plan:
    """A compiled netlist: `table` (CELL_DTYPE, sorted by level, MUX cells last in each), `level_end`, and the outputs as (wire or
    constant index, negated)."""

    def __init__(self, n_inputs, table, level_end, outputs, wire_of):
        self.n_inputs, self.table, self.level_end, self.outputs = n_inputs, table, level_end, outputs
        self.wire_of = wire_of                                                        # netlist node of a live gate -> its wire
        self.cells = len(table)
        self.rotations = self.cells + int((table["op"] == CELL_OPS["MUX"]).sum())   # blind rotations per lane
        self.depth = len(level_end)                                                   # bootstrap batches of a run
        self.wires = n_inputs + self.cells

    def levels(self):
        """[(first cell, cells, MUX cells)] per level"""
        lo, out = 0, []
        for hi in self.level_end:
            out.append((lo, int(hi) - lo, int((self.table["op"][lo:int(hi)] == CELL_OPS["MUX"]).sum())))
            lo = int(hi)
        return out

    def bind(self, be):
        return BoundPlan(self, be)


class BoundPlan:
    """A plan on one backend: the device copy of its table is made by the first run and lives until close() or the backend's."""

    def __init__(self, plan, be):
        self.plan, self.be, self.handle, self.arena = plan, be, None, None

    def run(self, inputs):
        """inputs int32 [n_inputs][L][W] -> outputs [n_out][L][W]. The whole arena of the run stays in self.arena."""
        import torch
        p, be = self.plan, self.be
        assert inputs.dim() == 3 and inputs.shape[0] == p.n_inputs, "inputs must be [n_inputs][L][W]"
        _, L, W = inputs.shape
        arena = inputs.new_empty((p.wires, L, W))
        arena[:p.n_inputs] = inputs
        if p.cells and L:
            if self.handle is None:
                self.handle = be.circuit_create(p.table, p.level_end, p.n_inputs)
            be.circuit_run(self.handle, arena, L)
        self.arena = arena
        outs = []
        for src, neg in p.outputs:
            if src < 0:
                t = inputs.new_zeros((L, W))
                t[:, W - 1] = E8 if src == -2 else -E8
            else:
                t = be.lincomb(arena[src], -1) if neg else arena[src]
            outs.append(t)
        return torch.stack(outs) if outs else inputs.new_empty((0, L, W))

    def close(self):
        if self.handle is not None and not getattr(self.be, "closed", False):
            self.be.circuit_destroy(self.handle)
        self.handle = None


# ---- generators ----
def _ripple(nl, a, b, carry_op):
    """sum / difference bits and the last carry of the chain XOR3 + carry_op over the bits of a and b"""
    carry, out = nl.const(0), []
    for x, y in zip(a, b):
        out.append(nl.gate("XOR3", x, y, carry))
        carry = nl.gate(carry_op, x, y, carry)
    return out, carry


def _operands(bits):
    nl = Netlist(2 * bits)
    return nl, nl.inputs(0, bits), nl.inputs(bits, bits)


def adder(bits):
    """a + b: bits + 1 outputs (the sum bits, then the carry out)"""
    nl, a, b = _operands(bits)
    s, carry = _ripple(nl, a, b, "MAJ3")
    for w in s + [carry]:
        nl.output(w)
    return nl


def subtractor(bits):
    """a - b mod 2^bits: bits + 1 outputs (the difference bits, then the borrow, set where a < b)"""
    nl, a, b = _operands(bits)
    d, borrow = _ripple(nl, a, b, "MAJ3N")
    for w in d + [borrow]:
        nl.output(w)
    return nl


def _borrow(nl, a, b):
    borrow = nl.const(0)
    for x, y in zip(a, b):
        borrow = nl.gate("MAJ3N", x, y, borrow)
    return borrow


def less_than(bits):
    """a < b (unsigned): one output, the final borrow of a - b"""
    nl, a, b = _operands(bits)
    nl.output(_borrow(nl, a, b))
    return nl


def equal(bits):
    """a == b: one output, an AND tree over the XNORs of the bits"""
    nl, a, b = _operands(bits)
    same = [nl.gate("XNOR", x, y) for x, y in zip(a, b)]
    while len(same) > 1:
        same = [nl.gate("AND", same[i], same[i + 1]) for i in range(0, len(same) - 1, 2)] + same[len(same) & ~1:]
    nl.output(same[0])
    return nl


def select(bits):
    """cond ? x : y with the inputs cond, x bits, y bits: one MUX cell per bit, one level"""
    nl = Netlist(1 + 2 * bits)
    cond, x, y = nl.input(0), nl.inputs(1, bits), nl.inputs(1 + bits, bits)
    for i in range(bits):
        nl.output(nl.mux(cond, x[i], y[i]))
    return nl


def maximum(bits):
    """max(a, b): the borrow chain of a - b, then one level of MUX cells"""
    nl, a, b = _operands(bits)
    lt = _borrow(nl, a, b)
    for i in range(bits):
        nl.output(nl.mux(lt, b[i], a[i]))
    return nl


def multiplier(bits):
    """a * b: 2 bits outputs. Schoolbook: bits^2 AND cells, then bits - 1 ripple rows of XOR3 / MAJ3 full adders; the rows overlap
    in the level schedule (row i's bit j waits for row i-1's bit j+1 only)."""
    nl, a, b = _operands(bits)
    acc = [nl.gate("AND", a[j], b[0]) for j in range(bits)]
    out = []
    for i in range(1, bits):
        out.append(acc[0])
        high = acc[1:] + [nl.const(0)] * (bits - len(acc) + 1)
        row = [nl.gate("AND", a[j], b[i]) for j in range(bits)]
        acc, carry = _ripple(nl, high, row, "MAJ3")
        acc.append(carry)
    out += acc
    for w in out + [nl.const(0)] * (2 * bits - len(out)):
        nl.output(w)
    return nl
