// rs_ring_selector.h -- the selector keyswitch of circuit bootstrapping (rs_ring_selector_dev, rs_circuit_bootstrap_dev;
// include/redsec_hip.h): the placement and the index arithmetic shared by the kernels of rs_ring_selector.hip and the lane emulator
// (rs_emulate.cpp), restated in numpy by redsec_amd/keygen.py (ring_selector_switch).
//
// depth l LWE samples ct[k l + j] = (a, b) of dimension n_src, the bootstraps of bit k at level j with phase +-h_j/2,
// h_j = 2^(32-(j+1) basebit), become depth RGSW samples sel[k] [2l][2][N] under the ring key S: with x = (a, b + h_j/2),
//     d_iq = ((x_i + off) >> (32-(q+1) ks_basebit)) & (2^ks_basebit - 1),   off = pa_offset(ks_basebit, ks_t),
//     sel[k][f l + j] = - sum_{i <= n_src, q < ks_t} d_iq K[f][i][q],        f = 0, 1,
// K [2][n_src+1][ks_t][2][N] the selector key: K[f][i][q] is a ring sample of M_f sg_i 2^(32-(q+1) ks_basebit), sg = (s, -1), M_1 = 1
// and M_0 = -S(X). Every sample lands on X^0: there is no rotation, and every key word is shared by all depth l rows of a call, so the
// call is a small exact GEMM of the digit matrix [rows][(n_src+1) ks_t] against the key stream. 32-bit integer arithmetic mod 2^32,
// exact in any order. No floating point and no transform. Keys are made on the host (keygen.py selector_key): none of it is here.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rs_pack.h"

namespace rs {

// Placement of ring_selector_kernel: a workgroup of kSeThreads threads owns kSeTile = 4 kSeThreads consecutive coefficients of ONE
// polynomial p of ONE family f (thread t the four coefficients k0 + 4t .. k0 + 4t + 3), ONE chunk of kSeChunk consecutive coordinates
// i and ONE block of kSeRows consecutive sample rows: 4 x kSeRows accumulators per thread, in registers over the whole chunk. Each key
// word of the chunk is loaded once, 16 bytes a thread, and applied to all rows of the block. The grid runs over (tile, polynomial,
// family, chunk, row block); the partial sums of the chunks meet in the output by atomic adds on the words ring_selector_init_kernel
// has zeroed. N is a power of two in kSeMinN .. kSeMaxN.
constexpr int kSeThreads = 128, kSeKpt = 4, kSeTile = kSeThreads * kSeKpt;
constexpr int kSeMinN = 1024, kSeMaxN = 8192;
constexpr int kSeChunk = 8;             // coordinates of a workgroup: (n_src + 1) / 8 chunks keep every CU busy at n = 350
constexpr int kSeRows = 8;              // sample rows of a register block
constexpr int kSePre = 4;               // key words (16 bytes each) a thread keeps in flight
constexpr int kSeInitThreads = 256;     // threads of a workgroup of ring_selector_init_kernel (one output word each)
constexpr int kSeMaxBits = 31;          // l basebit <= 31: the half step h_j / 2 is an integer
constexpr int kSeMaxDepth = 30;
constexpr int kSeMaxSrc = 65536;

// x + se_offset rounds the digits to nearest: rs_pack_dev's offset
RS_HD uint32_t se_offset(int ks_basebit, int ks_t) { return pa_offset(ks_basebit, ks_t); }
// what is added to b of row r = k l + j: h_j / 2 = 2^(31 - (j+1) basebit)
RS_HD uint32_t se_half_step(int basebit, int j) { return 1u << (31 - (j + 1) * basebit); }
RS_HD uint32_t se_digit(uint32_t xbar, int ks_basebit, int q) { return (xbar >> (32 - (q + 1) * ks_basebit)) & ((1u << ks_basebit) - 1u); }

RS_HD int se_tiles(int N) { return N / kSeTile; }
RS_HD int se_chunks(int n_src) { return (n_src + 1 + kSeChunk - 1) / kSeChunk; }
RS_HD long se_row_blocks(long rows) { return (rows + kSeRows - 1) / kSeRows; }
RS_HD long se_groups_per_block(int N, int n_src) { return 4L * se_tiles(N) * se_chunks(n_src); }
RS_HD long se_groups(long rows, int N, int n_src) { return se_row_blocks(rows) * se_groups_per_block(N, n_src); }

// polynomial p of K[f][i][q] of the key [2][n_src+1][ks_t][2][N]
RS_HD size_t se_key_offset(int N, int n_src, int ks_t, int f, int i, int q, int p) {
  return ((((size_t)f * ((size_t)n_src + 1) + (size_t)i) * (size_t)ks_t + (size_t)q) * 2 + (size_t)p) * (size_t)N;
}
// polynomial p of the output row of sample row r = k l + j and family f: row f l + j of sel[k] [2l][2][N]
RS_HD size_t se_out_offset(int N, int l, int r, int f, int p) {
  const int k = r / l, j = r - k * l;
  return ((((size_t)k * 2 + (size_t)f) * (size_t)l + (size_t)j) * 2 + (size_t)p) * (size_t)N;
}

// Placement of ring_selector_wide_kernel (rs_ring_selector_wide.hip; rs_ring_selector_batch_dev, rs_circuit_bootstrap_batch_dev): the
// same kSeThreads threads on the same kSeTile coefficients of one polynomial of one family, but ALL n_src + 1 coordinates and one
// block of kSwRows consecutive sample rows: 4 x kSwRows accumulators per thread over the whole key stream, stored once. The words
// x_i + off of the block are staged in LDS kSwPiece coordinates at a time. The grid runs over (tile, polynomial, family, row block),
// the first three fastest: at N = 1024 they are the 8 residues of the workgroup index, so the workgroups that share key words follow
// each other at a distance of 8.
constexpr int kSwRows = 16;             // sample rows of a register block (the arithmetic: header of rs_ring_selector_wide.hip)
constexpr int kSwPiece = 64;            // coordinates staged at a time: kSwPiece x kSwRows words = 4 KB of LDS
constexpr int kSwPre = 4;               // key words (16 bytes each) a thread keeps in flight, across the pieces
constexpr int kSwLdsBytes = kSwPiece * kSwRows * 4;
static_assert(kSwPiece % kSwPre == 0, "a full piece holds whole rounds of the key ring, so every piece starts at ring slot 0");
static_assert((kSwPiece * kSwRows) % kSeThreads == 0 && kSwRows % 4 == 0, "staging and the 16-byte reads of the staged words");

RS_HD long sw_row_blocks(long rows) { return (rows + kSwRows - 1) / kSwRows; }
RS_HD long sw_groups_per_block(int N) { return 4L * se_tiles(N); }
RS_HD long sw_groups(long rows, int N) { return sw_row_blocks(rows) * sw_groups_per_block(N); }
RS_HD int sw_pieces(int n_src) { return (n_src + 1 + kSwPiece - 1) / kSwPiece; }

// ---- which kernel a batch selector keyswitch runs (rs_ring_selector_batch_dev only dispatches on this; CPU-tested through the
// emulator library) ----
//   kSeChunked  ring_selector_kernel: chunks of kSeChunk coordinates that meet by atomic adds, ceil((n_src+1)/8) adds per output word
//   kSeWide     ring_selector_wide_kernel: every output word stored once
// Wide as soon as its own grid gives every CU of the context a workgroup: below that the chunks are what keeps the device busy, from
// there on the rows do and the atomic adds (n_src + 1) / 8 times the size of the result are pure cost. Derived; the sweep that
// confirms it is in INTEGRATION.md section 27. `force` is the diagnostic switch RS_SEL_FORM read once in rs_create.
enum SeForm { kSeAuto = -1, kSeChunked = 0, kSeWide = 1 };
struct SePlan { int form; long groups; };
RS_HD SePlan selector_form(long rows, int N, int n_src, int num_cus, int force) {
  SePlan p = {kSeChunked, 0};
  if (rows <= 0) return p;
  const long wide = sw_groups(rows, N);
  if (force == kSeWide || (force == kSeAuto && wide >= (long)num_cus)) { p.form = kSeWide; p.groups = wide; }
  else p.groups = se_groups(rows, N, n_src);
  return p;
}

// rs_circuit_bootstrap_dev's scratch, in words: the l test polynomials [l][N], the row index [rows] of the gather, the replicated
// bits [rows][n+1] and their bootstraps [rows][n+1], rows = depth l
RS_HD size_t se_scratch_index(int N, int l, long) { return (size_t)l * (size_t)N; }
RS_HD size_t se_scratch_bits(int N, int l, long rows) { return se_scratch_index(N, l, rows) + (size_t)rows; }
RS_HD size_t se_scratch_boot(int N, int l, long rows, int n) { return se_scratch_bits(N, l, rows) + (size_t)rows * ((size_t)n + 1); }
RS_HD size_t se_scratch_words(int N, int l, long rows, int n) { return se_scratch_boot(N, l, rows, n) + (size_t)rows * ((size_t)n + 1); }

}  // namespace rs
