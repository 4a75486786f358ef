// rs_rows.h -- the row-op table and the per-word arithmetic of the indexed gate batches (rs_gate_rows_dev, rs_gate3_dev;
// include/redsec_hip.h), shared by gate_rows_kernel (rs_rows.hip), the host entry points (rs_api.cpp) and the lane emulator
// (rs_emulate.cpp); restated in numpy by tests/rows_ref.py.
//
// Row r of a call is the linear combination x = c0 s0 + c1 s1 + c2 s2 + (0, bconst) of three SOURCE rows, word-wise mod 2^32,
// which the unchanged bootstrap path then takes as a plain ciphertext. A source is a row of the input array picked by an index,
// or one of the two trivial samples when the index names no row. 32-bit integer arithmetic only.
#pragma once

#include <cstdint>

#include "rs_ntt.h"

namespace rs {

constexpr int kRowOps = 13;          // rs_row_op: 0..9 = rs_gate_op, 10 MAJ3, 11 XOR3, 12 MAJ3N
constexpr int kRowMaxGroups = 16;    // groups of one call (their prefix sums travel by value)
constexpr int32_t kRowIdxTrue = -2;  // index of the trivial TRUE sample; every other index outside [0, in_rows) is trivial FALSE
constexpr uint32_t kRowE8 = 1u << 29, kRowE4 = 1u << 30;   // modSwitchToTorus32(1, 8), (1, 4)

struct RowCoef { int32_t c[3]; uint32_t bconst; };

// ops 0..9: TFHE's boolean-gates.cpp constants (the gate_coef table of rs_api.cpp) with a zero third coefficient;
// 10..12: the three-input combinations, bconst = 0
RS_HD bool row_coef(int op, RowCoef* g) {
  switch (op) {
    case 0:  *g = {{-1, -1, 0}, kRowE8}; return true;        // NAND
    case 1:  *g = {{1, 1, 0}, kRowE8}; return true;          // OR
    case 2:  *g = {{1, 1, 0}, 0u - kRowE8}; return true;     // AND
    case 3:  *g = {{-1, -1, 0}, 0u - kRowE8}; return true;   // NOR
    case 4:  *g = {{2, 2, 0}, kRowE4}; return true;          // XOR
    case 5:  *g = {{-2, -2, 0}, 0u - kRowE4}; return true;   // XNOR
    case 6:  *g = {{-1, 1, 0}, 0u - kRowE8}; return true;    // ANDNY
    case 7:  *g = {{1, -1, 0}, 0u - kRowE8}; return true;    // ANDYN
    case 8:  *g = {{-1, 1, 0}, kRowE8}; return true;         // ORNY
    case 9:  *g = {{1, -1, 0}, kRowE8}; return true;         // ORYN
    case 10: *g = {{1, 1, 1}, 0u}; return true;              // MAJ3:  sign of a + b + c
    case 11: *g = {{-2, -2, -2}, 0u}; return true;           // XOR3:  sign of -2 (a + b + c)
    case 12: *g = {{-1, 1, 1}, 0u}; return true;             // MAJ3N: sign of -a + b + c
  }
  return false;
}

// the groups of a call: rows [end[g-1], end[g]) run ops[g] (end[-1] = 0; an empty group has end[g] = end[g-1])
struct RowGroups {
  long end[kRowMaxGroups];
  int32_t op[kRowMaxGroups];
  int32_t count;
};
// op of row r < end[count - 1]: the first group whose end lies past r
RS_HD int row_op_of(const RowGroups& g, long r) {
  int k = 0;
  while (k + 1 < g.count && r >= g.end[k]) ++k;
  return g.op[k];
}

struct GateRowsArgs {
  const int32_t* src[3];   // base of source j: [in_rows][W] (rs_gate_rows_dev: the same array three times)
  const int32_t* idx;      // [B][3], or nullptr = the identity (source j of row r is row r of src[j])
  long in_rows;
  int32_t* out;            // [B][W] materialised combinations (the lane's staging buffer: never an input)
  long B;
  int W;
  RowGroups groups;
};

// word w of the source an index picks: the row's word when the index names a row -- the ONLY read of the input, so nothing
// outside [0, in_rows) x [0, W) is ever touched -- else word w of the trivial sample (0, +-1/8)
RS_HD uint32_t row_source_word(const int32_t* base, long in_rows, int W, long index, int w) {
  if (index >= 0 && index < in_rows) return (uint32_t)base[index * W + w];
  if (w != W - 1) return 0u;
  return index == kRowIdxTrue ? kRowE8 : 0u - kRowE8;
}

// word w of row r
RS_HD uint32_t row_word(const GateRowsArgs& a, const RowCoef& g, const long (&index)[3], int w) {
  uint32_t x = w == a.W - 1 ? g.bconst : 0u;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (g.c[j] != 0) x += (uint32_t)g.c[j] * row_source_word(a.src[j], a.in_rows, a.W, index[j], w);
  return x;
}

// lane L of the wave that owns row r: words L, L + 64, ... (consecutive lanes read and write consecutive words)
RS_HD void row_lane(const GateRowsArgs& a, long r, int lane) {
  RowCoef g;
  if (!row_coef(row_op_of(a.groups, r), &g)) return;   // (ops are validated on the host)
  long index[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) index[j] = a.idx ? (long)a.idx[3 * r + j] : r;
  for (int w = lane; w < a.W; w += 64) a.out[r * a.W + w] = (int32_t)row_word(a, g, index, w);
}

}  // namespace rs
