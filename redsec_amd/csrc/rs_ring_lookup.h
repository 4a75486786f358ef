// rs_ring_lookup.h -- batched encrypted lookup (rs_ring_lookup_rows_dev, rs_ring_lookup_rows_alt_dev; include/redsec_hip.h;
// INTEGRATION.md section 28): the index arithmetic shared by the kernels of rs_ring_lookup.hip and the lane emulator
// (rs_emulate.cpp), restated in numpy by redsec_amd/keygen.py (ring_lookup_rows) as a loop over ring_lookup.
//
// R CMUX trees (rs_ring_cmux.h) side by side, one level of ALL of them per launch. Row q has a table of `entries` ciphertexts,
// entry e at word (q row_stride + e entry_stride) 2N of `table`, and a hidden index given as `depth` RGSW samples, one set for all
// rows or one per row. Level k of row q pairs the rows (2i, 2i + 1) of its previous level under sample k of its set,
//     next_q[i] = prev_q[2i] + sum_j Da_j(X) S_qk[j] + sum_j Db_j(X) S_qk[l + j]  over the digits of  prev_q[2i + 1] - prev_q[2i],
// an unpaired last row meeting the all-zero ciphertext (the difference is -prev_q[2i]): the arithmetic of rs_ring_lookup_dev row by
// row, word for word. Level k writes its P_k = ceil(rows_k / 2) ciphertexts per row contiguously as [R][P_k][2][N]; the next level
// reads that with row stride P_k and entry stride 1. Output ciphertext g of a level is (q, i) = (g / P, g mod P). The placement
// inside a ciphertext, the window, the sweep and the atomics are those of ring_cmux_kernel. Integer arithmetic only, exact in any
// order.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rs_ring_cmux.h"

namespace rs {

constexpr int kLkMaxDepth = kRcMaxDepth;
constexpr int kLkInitThreads = kRcInitThreads;

// rows a level with `rows` input rows per table leaves: its pairs and, for an odd count, the unpaired last row
RS_HD long lk_level_rows(long rows) { return rc_level_rows(rows); }
// rows entering level k of a tree over `entries`
RS_HD long lk_rows_at(long entries, int k) {
  long rows = entries;
  for (int i = 0; i < k; ++i) rows = lk_level_rows(rows);
  return rows;
}

// output ciphertext g of a level that leaves P ciphertexts per row: row q, pair i (g < 2^31, so one 32-bit division, on the
// scalar unit where g is uniform)
struct LkPlace {
  long q, i;
};
RS_HD LkPlace lk_place(long g, long P) {
  const unsigned q = (unsigned)g / (unsigned)P;
  return {(long)q, (long)((unsigned)g - q * (unsigned)P)};
}
// whether pair i of a level with `rows` input rows has its second row; otherwise it meets the all-zero ciphertext
RS_HD bool lk_paired(long i, long rows) { return 2 * i + 1 < rows; }
// the first source ciphertext d0 of pair i of row q, in ciphertexts from the level's input; d1 is entry_stride further
RS_HD size_t lk_source(long q, long i, size_t row_stride, size_t entry_stride) {
  return (size_t)q * row_stride + 2 * (size_t)i * entry_stride;
}
// sample k of row q's selector set, in words from sel (sel_row_stride = 0: one set serves every row)
RS_HD size_t lk_sel_words(int N, int l) { return (size_t)2 * l * 2 * (size_t)N; }
RS_HD size_t lk_sel_offset(long q, size_t sel_row_stride, int k, int N, int l) {
  return (size_t)q * sel_row_stride + (size_t)k * lk_sel_words(N, l);
}

// workgroups of the sweep and of the init kernel of a level that leaves P ciphertexts per row
RS_HD long lk_groups(long R, long P, int N, int l) { return R * P * rc_groups_per_ct(N, l); }
RS_HD long lk_init_groups(long R, long P, int N) { return R * P * (2 * (long)N / kLkInitThreads); }

// The scratch plan: two ping-pong halves of R ceil(E / 2) and R ceil(E / 4) ciphertexts. Level k < depth - 1 writes half k & 1
// from its start; the last level writes out.
RS_HD long lk_scratch_rows(long R, long entries) { return R * rc_scratch_rows(entries); }
RS_HD long lk_scratch_half(long R, long entries, int second) { return second ? R * lk_level_rows(entries) : 0; }     // first ciphertext

}  // namespace rs
