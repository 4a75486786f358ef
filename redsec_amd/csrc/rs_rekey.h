// rs_rekey.h -- re-keying (rs_rekey_dev; include/redsec_hip.h): the placement and the index arithmetic shared by the kernels of
// rs_rekey.hip and the lane emulator (rs_emulate.cpp), restated in numpy by redsec_amd/keygen.py (rekey).
//
// The public keyswitch from an LWE key s of dimension n_src to an LWE key s' of dimension n_dst under a caller-supplied key,
//     out[r] = (0, b_r) - sum_{i < n_src, j < t} d_ij(r) K[i][j],    d_ij(r) = digit j of (a_i of sample r) + offset,
// K[i][j] = (a_ij, <a_ij, s'> + e_ij + s_i 2^(32 - (j+1) basebit)) row i t + j of the re-keying key, n_dst + 1 words. Everything is
// 32-bit integer arithmetic: a basebit-bit digit times a 32-bit word, accumulated mod 2^32, exact in any order. No floating point
// and no transform. The key is made by the calls that exist (seeded rows under s', or rows extracted from ciphertexts under the
// recipient's RLWE public key): none of it is in this file.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rs {

// The helpers are constexpr, so the host compiler of the emulator and both sides of the device compiler take them as they are.
// Placement of rekey_kernel: a workgroup of kRkWaves waves owns kRkWords consecutive output words (lane l the word w0 + l) of
// kRkTile = kRkWaves kRkWaveCts consecutive ciphertexts (wave v the ciphertexts r0 + v kRkWaveCts .., one accumulator each in
// registers) and a run of rk_span index chunks of kRkSeg source indices each (the last chunk has n_src mod kRkSeg). The t key rows
// of one source index, kRkWords words each, are staged once in LDS and serve all kRkTile ciphertexts; the mask words of a chunk
// are staged (transposed) once per chunk and wave. The grid runs over (word tile, index split, ciphertext tile); the partial sums
// meet in the output by atomic adds on the words rekey_init_kernel has set.
constexpr int kRkWords = 64, kRkWaves = 4, kRkThreads = kRkWords * kRkWaves;
constexpr int kRkWaveCts = 32, kRkTile = kRkWaves * kRkWaveCts;
constexpr int kRkSeg = 8;               // source indices of a chunk: 32 contiguous bytes of a sample
constexpr int kRkGroup = 8;             // ciphertexts of a wave skipped together when the tile is ragged
constexpr int kRkMaxT = 32;             // t basebit <= 32
constexpr int kRkPre = kRkMaxT * kRkWords / kRkThreads;   // key words a thread stages per source index, at most
constexpr int kRkFill = 2048;           // workgroups a launch aims for before it stops splitting the source indices
constexpr int kRkInitThreads = 256;     // threads of a workgroup of rekey_init_kernel (one output word each)
constexpr int kRkMinDim = 1, kRkMaxDim = 65536;

// abar = a + rk_offset: the digits then round to nearest instead of down (lweKeySwitch's prec_offset); 0 when all 32 bits are used
constexpr uint32_t rk_offset(int basebit, int t) { return t * basebit >= 32 ? 0u : 1u << (31 - t * basebit); }
// digit j of abar: bits 32 - (j+1) basebit .. 31 - j basebit
constexpr uint32_t rk_digit(uint32_t abar, int basebit, int j) { return (abar >> (32 - (j + 1) * basebit)) & ((1u << basebit) - 1u); }

constexpr int rk_chunks(int n_src) { return (n_src + kRkSeg - 1) / kRkSeg; }
constexpr long rk_ct_tiles(long B) { return (B + kRkTile - 1) / kRkTile; }
constexpr int rk_word_tiles(int n_dst) { return (n_dst + 1 + kRkWords - 1) / kRkWords; }
// index chunks one workgroup walks: all of them once the tiles alone fill the device, else as few as give kRkFill workgroups
constexpr int rk_span(long B, int n_src, int n_dst) {
  const int chunks = rk_chunks(n_src);
  const long base = rk_ct_tiles(B) * rk_word_tiles(n_dst);
  if (base >= kRkFill) return chunks;
  long want = (kRkFill + base - 1) / base;
  if (want > chunks) want = chunks;
  return (int)((chunks + want - 1) / want);
}
constexpr int rk_splits(long B, int n_src, int n_dst) {
  const int span = rk_span(B, n_src, n_dst);
  return (rk_chunks(n_src) + span - 1) / span;
}
// workgroups of a call
constexpr long rk_groups(long B, int n_src, int n_dst) { return rk_ct_tiles(B) * rk_word_tiles(n_dst) * rk_splits(B, n_src, n_dst); }

// word w of key row (i, j) of rekey_key [n_src][t][n_dst+1]
constexpr size_t rk_key_offset(int n_dst, int t, int i, int j) { return ((size_t)i * t + j) * ((size_t)n_dst + 1); }
// staged mask word of source index i0 + ii and ciphertext c of a wave's tile: s_a[ii][c]
constexpr int rk_mask_index(int ii, int c) { return ii * kRkWaveCts + c; }

}  // namespace rs
