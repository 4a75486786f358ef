// rs_pack.h -- packed results (rs_pack_dev; include/redsec_hip.h): the placement and the index arithmetic shared by the kernels of
// rs_pack.hip and the lane emulator (rs_emulate.cpp), restated in numpy by redsec_amd/keygen.py (pack).
//
// The public keyswitch from the LWE key s to the ring key S with the identity function: up to N LWE samples (a, b) go into the
// coefficients of one ciphertext over Z[X]/(X^N + 1) mod 2^32,
//     rlwe[r] = (0, sum_c b_c X^c) - sum_{i < n, j < t} D_ij(X) K[i][j],    D_ij(X) = sum_c digit_j(a_i of sample rN + c) X^c,
// K[i][j] = (a_ij, a_ij*S + e_ij + s_i 2^(32 - (j+1) basebit)) the packing key. Everything is 32-bit integer arithmetic: a
// basebit-bit digit times a 32-bit word, accumulated mod 2^32, exact in any order. No floating point and no transform.
// Streams of the key (owner's side only: redsec_amd/keygen.py pack_key and, on the device, rs_packkey.h; none of it is in this file):
//     domain 14  packing-key mask    row i t + j   mask seed (public)             a_ij[k] = word k, k < N
//     domain 15  packing-key noise   row i t + j   owner's noise seed (private)   e_ij[k] = Gaussian k (words 4k .. 4k+3, kg_noise32)
#pragma once

#include <cstdint>

#include "rs_ring_sweep.h"

namespace rs {

enum { kKgPackMask = 14, kKgPackNoise = 15 };

// Placement of pack_kernel: a workgroup of kPaThreads threads owns kPaTile = 4 kPaThreads consecutive output coefficients of one
// polynomial of one ciphertext (thread t the four coefficients k0 + 4t .. k0 + 4t + 3, in registers), a block of at most kPaSlots
// slots c and a chunk of kPaSeg consecutive LWE indices i (all t digits of each; the last chunk has n mod kPaSeg); per key row it
// runs the sweep of rs_ring_sweep.h over the block's slots. The grid runs
// over (tile, polynomial, slot block, index chunk, ciphertext); the partial sums meet in the output by atomic adds. The chunk has
// ONE size, so there is one path and one split per n: a workgroup stages its samples' words once, and more indices per workgroup
// would save nothing but some of the 4-byte atomic adds (one per output word and workgroup against 4 kPaSeg t slots multiply-adds).
constexpr int kPaThreads = 128, kPaKpt = kSweepKpt, kPaTile = kPaThreads * kPaKpt;
constexpr int kPaMinN = 1024, kPaMaxN = 8192;
constexpr int kPaSlots = 1024;          // slots of a slot block: bounds the LDS of a workgroup on every ring
constexpr int kPaSeg = 8;               // LWE indices of a chunk: their sample words are staged (transposed) in LDS, 32 bytes a sample
constexpr int kPaInitThreads = 256;     // threads of a workgroup of pack_init_kernel (one output word each)

// abar = a + pa_offset: the digits then round to nearest instead of down (lweKeySwitch's prec_offset); 0 when all 32 bits are used
RS_HD uint32_t pa_offset(int basebit, int t) { return t * basebit >= 32 ? 0u : 1u << (31 - t * basebit); }
// digit j of abar: bits 32 - (j+1) basebit .. 31 - j basebit
RS_HD uint32_t pa_digit(uint32_t abar, int basebit, int j) { return (abar >> (32 - (j + 1) * basebit)) & ((1u << basebit) - 1u); }

// slots of ciphertext r: min(N, count - rN)
RS_HD int pa_slots(long count, int N, long r) {
  const long left = count - r * (long)N;
  return left >= N ? N : (int)left;
}
RS_HD int pa_pad4(int c) { return (c + 3) & ~3; }
// slot blocks of the fullest ciphertext of a call (the grid is rectangular; a block past a ciphertext's slots has nothing to do)
RS_HD int pa_slot_blocks(long count, int N) { return (int)(((count < N ? count : (long)N) + kPaSlots - 1) / kPaSlots); }
RS_HD int pa_chunks(int n) { return (n + kPaSeg - 1) / kPaSeg; }
// workgroups of a call
RS_HD long pa_groups(long count, int n, int N) {
  return (count + N - 1) / N * 2 * (N / kPaTile) * pa_slot_blocks(count, N) * pa_chunks(n);
}

// A workgroup with first coefficient k0, first slot c0 and cpad = pa_pad4(its slots) stages the words ext[pa_window_base + i],
// i < cpad + kPaTile, of ext = (-p, p) (rs_rlwe.h): coefficient k0 + x of X^(c0 + cc) p is window word x - cc + cpad.
RS_HD int pa_window_base(int N, int k0, int c0, int cpad) { return rl_term_index(N, k0, c0) - cpad; }
RS_HD int pa_window_index(int cpad, int x, int cc) { return x - cc + cpad; }

// key row (i, j), polynomial poly of pack_key [n][t][2][N]
RS_HD size_t pa_key_offset(int N, int t, int i, int j, int poly) { return (((size_t)i * t + j) * 2 + poly) * (size_t)N; }

}  // namespace rs
