// rs_circuit.h -- the cell table, its host validation and the per-word arithmetic of the compiled circuits (rs_circuit_create,
// rs_circuit_run_dev; include/redsec_hip.h), shared by circuit_rows_kernel and circuit_fold_kernel (rs_circuit.hip), the host entry
// points (rs_api.cpp) and the lane emulator (rs_emulate.cpp); restated in numpy by tests/circuit_ref.py.
//
// A circuit is a table of cells sorted by level. Cell i defines wire n_inputs + i; wire w of lane l is row w * lanes + l of the
// arena. One level of C cells, the last M of them MUX, is staged as C * lanes + M * lanes combinations
//   x = +-c0 s0 +- c1 s1 +- c2 s2 + (0, bconst), word-wise mod 2^32,
// with the coefficients of rs_rows.h for ops 0..12 and, for a MUX cell (a, b, c), a + b - 1/8 at its own row and -a + c - 1/8 at
// row C * lanes + (its row among the MUX rows). The unchanged blind rotation takes them as plain ciphertexts; circuit_fold_kernel
// then adds the second extracted sample and (0, 1/8) to the first. 32-bit integer arithmetic only.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rs_rows.h"

namespace rs {

constexpr int kCellMux = 13;            // rs_cell_op: 0..12 = the row ops of rs_rows.h, 13 MUX
constexpr int kCellOps = 14;
constexpr int32_t kCellFalse = -1;      // a source that is the trivial FALSE sample (0, -1/8); kRowIdxTrue = -2 is the TRUE one

struct Cell { int32_t src[3]; uint8_t op; uint8_t neg; uint16_t reserved; };   // = rs_cell
static_assert(sizeof(Cell) == 16, "rs_cell is 16 bytes");

// coefficients of a cell's combination: `second` picks the second combination of a MUX cell; bit j of `neg` flips c[j]
RS_HD bool cell_coef(int op, int neg, bool second, RowCoef* g) {
  if (op == kCellMux) {
    if (second) *g = {{-1, 0, 1}, 0u - kRowE8};   // u2 = woKS(-a + c - 1/8)
    else *g = {{1, 1, 0}, 0u - kRowE8};           // u1 = woKS( a + b - 1/8)
  } else if (second || !row_coef(op, g)) {
    return false;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if ((neg >> j) & 1) g->c[j] = -g->c[j];
  return true;
}

// ---- host validation (rs_circuit_create): after it the device reads nothing outside the table and the arena ----
// 0, or -1 with *why naming the first fault. Every one of a cell's three sources is held to the rule, read or not.
inline int circuit_check(const Cell* cells, size_t n_cells, const uint32_t* level_end, size_t n_levels, size_t n_inputs, const char** why) {
  const char* unused;
  if (!why) why = &unused;
  *why = "";
  if (!cells || !level_end) { *why = "null pointer"; return -1; }
  if (n_levels == 0) { *why = "no level"; return -1; }
  // wires are int32 and the cell count travels in the uint32 level table
  if (n_cells > (size_t)INT32_MAX || n_inputs > (size_t)INT32_MAX || n_inputs + n_cells > (size_t)INT32_MAX) { *why = "too many wires for int32 sources"; return -1; }
  if ((size_t)level_end[n_levels - 1] != n_cells) { *why = "the last level does not end at n_cells"; return -1; }
  size_t lo = 0;
  for (size_t v = 0; v < n_levels; ++v) {
    const size_t hi = level_end[v];
    if (hi <= lo) { *why = v == 0 ? "empty first level" : "level_end does not increase (an empty level)"; return -1; }
    if (hi > n_cells) { *why = "level_end passes n_cells"; return -1; }
    bool mux_seen = false;
    for (size_t i = lo; i < hi; ++i) {
      const Cell& c = cells[i];
      if (c.op >= kCellOps) { *why = "op outside 0..13"; return -1; }
      if (c.reserved != 0) { *why = "reserved must be 0"; return -1; }
      if (c.op == kCellMux) mux_seen = true;
      else if (mux_seen) { *why = "the MUX cells of a level come last"; return -1; }
      for (int j = 0; j < 3; ++j) {
        const int64_t s = c.src[j];
        if (s < -2) { *why = "source below -2"; return -1; }
        if (s >= (int64_t)(n_inputs + lo)) { *why = "source is no input, constant or cell of an earlier level"; return -1; }
      }
    }
    lo = hi;
  }
  return 0;
}

// the rows of lanes * (n_inputs + n_cells) wires and the staged rows of the widest level, in words and bytes, fit a long
inline bool circuit_sizes_ok(size_t n_wires, size_t widest_rows_per_lane, size_t lanes, size_t W, size_t sample_words) {
  const size_t limit = (size_t)INT64_MAX / 8;
  const size_t rows = n_wires > widest_rows_per_lane ? n_wires : widest_rows_per_lane;
  const size_t words = W > sample_words ? W : sample_words;
  if (lanes == 0 || rows == 0 || words == 0) return true;
  if (rows > limit / lanes) return false;
  return rows * lanes <= limit / words;
}

// ---- one level on the device ----
struct CircuitLevelArgs {
  const Cell* cells;       // the whole table (DEVICE)
  const int32_t* arena;    // [n_wires][lanes][W]: only rows of inputs and of earlier levels are read
  int32_t* out;            // staged combinations [(C + M) lanes][W] (the lane's staging buffer: never part of the arena)
  long first;              // first cell of the level
  long C, M;               // its cells, and how many of them (the last ones) are MUX
  long lanes;
  int W;
};
RS_HD long circuit_level_rows(const CircuitLevelArgs& a) { return (a.C + a.M) * a.lanes; }

// word w of source `src` in lane `ct`: the wire's row, or the trivial sample (0, +-1/8)
RS_HD uint32_t cell_source_word(const CircuitLevelArgs& a, int32_t src, long ct, int w) {
  if (src >= 0) return (uint32_t)a.arena[((long)src * a.lanes + ct) * a.W + w];
  if (w != a.W - 1) return 0u;
  return src == kRowIdxTrue ? kRowE8 : 0u - kRowE8;
}

RS_HD uint32_t cell_word(const CircuitLevelArgs& a, const Cell& c, const RowCoef& g, long ct, int w) {
  uint32_t x = w == a.W - 1 ? g.bconst : 0u;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (g.c[j] != 0) x += (uint32_t)g.c[j] * cell_source_word(a, c.src[j], ct, w);
  return x;
}

// lane L of the wave that owns staged row r: words L, L + 64, ... Rows [0, C lanes) are the cells' own, cell-major; row
// C lanes + m is the second combination of MUX row m = the staged row (C - M) lanes + m.
RS_HD void circuit_row_lane(const CircuitLevelArgs& a, long r, int lane) {
  const long B = a.C * a.lanes;
  const bool second = r >= B;
  const long own = second ? r - a.M * a.lanes : r;
  const long k = own / a.lanes, ct = own - k * a.lanes;
  const Cell c = a.cells[a.first + k];
  RowCoef g;
  if (!cell_coef(c.op, c.neg, second, &g)) return;   // (cells are validated on the host)
  for (int w = lane; w < a.W; w += 64) a.out[r * a.W + w] = (int32_t)cell_word(a, c, g, ct, w);
}

// ---- the fold of the MUX rows on the extracted samples u[(C + M) lanes][words]: u[r] += u[B + m(r)] + (0, 1/8) ----
struct CircuitFoldArgs {
  int32_t* u;
  long B;          // C lanes
  long mux_rows;   // M lanes
  int words;       // k N + 1
};
RS_HD void circuit_fold_lane(const CircuitFoldArgs& a, long m, int lane) {
  int32_t* dst = a.u + (a.B - a.mux_rows + m) * a.words;
  const int32_t* add = a.u + (a.B + m) * a.words;
  for (int w = lane; w < a.words; w += 64)
    dst[w] = (int32_t)((uint32_t)dst[w] + (uint32_t)add[w] + (w == a.words - 1 ? kRowE8 : 0u));
}

}  // namespace rs
