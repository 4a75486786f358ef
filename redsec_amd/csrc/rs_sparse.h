// rs_sparse.h -- the row arithmetic and the host validation of the sparse bootstraps (rs_bootstrap_sparse_dev; include/redsec_hip.h),
// shared by sparse_gather_kernel, sparse_fill_kernel and sparse_scatter_kernel (rs_sparse.hip), the host entry point (rs_api.cpp)
// and the lane emulator (rs_emulate.cpp); restated in numpy by tests/test_sparse_cpu.py.
//
// A call names the rows of a batch that are really bootstrapped (`live`); every other row is the caller's promise of a trivial
// sample (0, ..., 0, b) and gets the trivial sample the dense path yields for it: no CMUX runs (every mod-switched mask word is 0),
// so the extracted sample is (0, ..., 0, coefficient 0 of X^rot * testvector), and the keyswitch of a zero mask subtracts nothing.
// The live rows are gathered into a compact batch, bootstrapped by the unchanged path, and scattered back. 32-bit integer
// arithmetic only.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rs_general.h"
#include "rs_ntt.h"

namespace rs {

// The b word of the bootstrapped trivial sample (0, ..., 0, b): the first lines of every blind-rotation kernel (the mod-switch
// of the b word, rot = 2N - barb, the rotated constant test vector) read at coefficient 0, with the kernels' own helpers.
RS_HD int32_t sparse_trivial_word(int32_t b, int32_t mu, int logn) {
  if (logn == 10) return rotated_const(mu, 0, 2 * kN - modswitch_2N(b));
  return gen_rotated_const(mu, 0, (2 << logn) - gen_modswitch(b, logn), logn);
}

struct SparseArgs {
  const int32_t* in;     // [B][W]; may be `out`
  int32_t* out;          // [B][W]
  const int32_t* live;   // [n_live] rows of the batch; entries outside [0, B) are ignored
  int32_t* rows;         // staged inputs [n_live][W] (the lane's staging buffer: never `in` or `out`)
  const int32_t* boot;   // their bootstrapped rows [n_live][W] (the second region of the staging buffer)
  long B, n_live;
  int W;
  int32_t mu;
  int logn;
};

// the row entry i names, or -1
RS_HD long sparse_live_row(const SparseArgs& a, long i) {
  const long r = (long)a.live[i];
  return (r >= 0 && r < a.B) ? r : -1;
}

// lane L of the wave that owns staged row i: words L, L + 64, ... of in[live[i]]; an ignored entry stages the zero sample (the
// compact batch bootstraps defined words, and its row is never scattered)
RS_HD void sparse_gather_lane(const SparseArgs& a, long i, int lane) {
  const long r = sparse_live_row(a, i);
  for (int w = lane; w < a.W; w += 64) a.rows[i * a.W + w] = r >= 0 ? a.in[r * a.W + w] : 0;
}

// lane L of the wave that owns row r of the batch. `b` is word n of in[r], read by the wave BEFORE any of its lanes stores (out may be
// in, and the last word is one lane's to overwrite): the kernel and the emulator both read it once per row and hand it in.
RS_HD void sparse_fill_lane(const SparseArgs& a, long r, int lane, int32_t b) {
  const int32_t t = sparse_trivial_word(b, a.mu, a.logn);
  for (int w = lane; w < a.W; w += 64) a.out[r * a.W + w] = w == a.W - 1 ? t : 0;
}

// lane L of the wave that owns staged row i: boot[i] to out[live[i]]; an ignored entry writes nothing
RS_HD void sparse_scatter_lane(const SparseArgs& a, long i, int lane) {
  const long r = sparse_live_row(a, i);
  if (r < 0) return;
  for (int w = lane; w < a.W; w += 64) a.out[r * a.W + w] = a.boot[i * a.W + w];
}

// ---- host validation (rs_bootstrap_sparse_dev): 0, or -1 with *why naming the fault ----
// B rows of W words, and the two staged regions of n_live <= B rows, in words and bytes, fit a long
inline bool sparse_sizes_ok(size_t B, size_t W) {
  const size_t limit = (size_t)INT64_MAX / 8;   // two regions of four-byte words
  if (B == 0 || W == 0) return true;
  return B <= limit / W;
}
inline int sparse_check(const void* out, const void* in, const void* live, size_t B, size_t n_live, size_t W, const char** why) {
  const char* unused;
  if (!why) why = &unused;
  *why = "";
  if (n_live > B) { *why = "n_live passes B"; return -1; }
  if (B == 0) return 0;
  if (!out || !in) { *why = "null ciphertext pointer"; return -1; }
  if (n_live > 0 && !live) { *why = "null live list"; return -1; }
  if (!sparse_sizes_ok(B, W)) { *why = "batch too large"; return -1; }
  return 0;
}

}  // namespace rs
