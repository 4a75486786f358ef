"""Independent numpy restatement of the indexed gate batches (include/redsec_hip.h rs_gate_rows_dev / rs_gate3_dev; INTEGRATION.md
section 14). TEST INFRASTRUCTURE ONLY. It builds the combinations x[r] = sum_j c_j row_j + (0, bconst), wrapping in int32, with the
trivial rows and the clamping rule; the expected output of a call is always the EXISTING oracle's ctx.bootstrap_batch(x, mu)."""
import numpy as np

E8, E4 = 1 << 29, 1 << 30
# rs_row_op -> ((c0, c1, c2), bconst): TFHE's boolean-gates.cpp constants for 0..9, the three-input combinations for 10..12
COEF = {
    "NAND": ((-1, -1, 0), E8), "OR": ((1, 1, 0), E8), "AND": ((1, 1, 0), -E8), "NOR": ((-1, -1, 0), -E8),
    "XOR": ((2, 2, 0), E4), "XNOR": ((-2, -2, 0), -E4), "ANDNY": ((-1, 1, 0), -E8), "ANDYN": ((1, -1, 0), -E8),
    "ORNY": ((-1, 1, 0), E8), "ORYN": ((1, -1, 0), E8),
    "MAJ3": ((1, 1, 1), 0), "XOR3": ((-2, -2, -2), 0), "MAJ3N": ((-1, 1, 1), 0),
}
OPS = ["NAND", "OR", "AND", "NOR", "XOR", "XNOR", "ANDNY", "ANDYN", "ORNY", "ORYN", "MAJ3", "XOR3", "MAJ3N"]   # by number
# what each op computes on plaintext bits
TRUTH = {
    "NAND": lambda a, b, c: 1 - (a & b), "OR": lambda a, b, c: a | b, "AND": lambda a, b, c: a & b, "NOR": lambda a, b, c: 1 - (a | b),
    "XOR": lambda a, b, c: a ^ b, "XNOR": lambda a, b, c: 1 - (a ^ b), "ANDNY": lambda a, b, c: (1 - a) & b,
    "ANDYN": lambda a, b, c: a & (1 - b), "ORNY": lambda a, b, c: (1 - a) | b, "ORYN": lambda a, b, c: a | (1 - b),
    "MAJ3": lambda a, b, c: ((a + b + c) >= 2) * 1, "XOR3": lambda a, b, c: a ^ b ^ c, "MAJ3N": lambda a, b, c: (((1 - a) + b + c) >= 2) * 1,
}


def name(op):
    return op if isinstance(op, str) else OPS[int(op)]


def source_rows(inp, index):
    """The rows the indices pick: in[i] for 0 <= i < in_rows, the trivial TRUE sample (0, +1/8) for -2, the trivial FALSE sample
    (0, -1/8) for every other index. int64 [len(index)][W]."""
    inp = np.asarray(inp, np.int64)
    index = np.asarray(index, np.int64)
    in_rows, W = inp.shape
    out = np.zeros((len(index), W), np.int64)
    out[:, W - 1] = np.where(index == -2, E8, -E8)
    ok = (index >= 0) & (index < in_rows)
    out[ok] = inp[index[ok]]
    return out


def op_per_row(groups):
    return [name(op) for op, count in groups for _ in range(int(count))]


def combine(inp, idx, groups):
    """x int32 [B][W] of a call with one input array."""
    return combine3(inp, inp, inp, idx, groups)


def combine3(a, b, c, idx, groups):
    """x int32 [B][W] with three input arrays; idx None = the identity (rs_gate3_dev)."""
    ops = op_per_row(groups)
    B = len(ops)
    idx = np.repeat(np.arange(B)[:, None], 3, 1) if idx is None else np.asarray(idx, np.int64).reshape(B, 3)
    src = [source_rows(s, idx[:, j]) for j, s in enumerate((a, b, c))]
    W = src[0].shape[1]
    x = np.zeros((B, W), np.int64)
    for r, op in enumerate(ops):
        coef, bconst = COEF[op]
        x[r] = sum(cj * src[j][r] for j, cj in enumerate(coef))
        x[r, W - 1] += bconst
    return (x & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
