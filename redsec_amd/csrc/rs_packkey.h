// rs_packkey.h -- the packing key on the device (rs_pack_keygen_dev, rs_pack_expand_dev; include/redsec_hip.h): the streams, the
// placement and the index arithmetic shared by the kernels of rs_packkey.hip and the lane emulator (rs_emulate.cpp), restated in numpy
// by redsec_amd/keygen.py (pack_key_mask, pack_key).
//
// Row i t + j of the key is the ring sample K[i][j] = (a, b = a*S + e + s_i g_j X^0) over Z[X]/(X^N + 1) mod 2^32, g_j =
// 2^(32 - (j+1) basebit). Streams (rs_pack.h), both of row i t + j:
//     domain 14  mask   mask seed (public)     a[k] = word k, k < N
//     domain 15  noise  noise seed (private)   e[k] = Gaussian k (words 4k .. 4k+3, kg_noise32)
// The noise is why this is not part of rs_pack.h / rs_pack.hip: those sources stay integer-only.
#pragma once

#include <cstdint>

#include "rs_keygen.h"
#include "rs_pack.h"

namespace rs {

// Placement of pack_keygen_kernel, that of rlwe_pk_encrypt_kernel (rs_rlwe.h): a workgroup of kPgThreads threads owns kPgTile = 4
// kPgThreads consecutive coefficients of one row's body, thread t the four coefficients k0 + 4t .. k0 + 4t + 3 in registers; the grid
// runs over (row, tile). The window ext[k0 .. k0 + N + kPgTile) of ext = (-a, a) is staged in LDS straight from the row's ChaCha
// blocks: k0 and N are multiples of 16, so window block wb (words 16 wb .. 16 wb + 15 of the window) is one whole mask block.
constexpr int kPgThreads = kRlThreads, kPgKpt = kRlKpt, kPgTile = kRlTile;
constexpr int kPgMinN = kPaMinN, kPgMaxN = kPaMaxN;
// Placement of pack_expand_kernel: thread `item` = row N/16 + blk of the flat grid stores mask block blk of the row and copies the
// body words blk + (N/16) r, r < 16 (consecutive threads copy consecutive words).
constexpr int kPgExThreads = 256;

RS_HD void pg_row(uint64_t row, int t, int& i, int& j) {
  i = (int)(row / (uint64_t)t);
  j = (int)(row - (uint64_t)i * (uint64_t)t);
}
RS_HD uint32_t pg_gadget(int j, int basebit) { return 1u << (32 - (j + 1) * basebit); }
// bit k of a secret key packed 32 bits per word (bit k & 31 of word k >> 5)
RS_HD uint32_t pg_key_bit(const uint32_t* packed, int k) { return (packed[k >> 5] >> (k & 31)) & 1u; }

// mask words 16 blk .. 16 blk + 15 of row `row`: block blk of stream (14, row) of the mask seed
RS_HD void pg_mask_block(const uint32_t (&key)[8], uint64_t row, int blk, uint32_t (&w)[16]) {
  kg_chacha_block(key, kKgPackMask, row, (uint32_t)blk, w);
}
// window block wb of the tile at k0: ext words k0 + 16 wb .. + 15, i.e. mask block ((k0 + 16 wb) mod N) / 16, negated below N
RS_HD void pg_window_block(const uint32_t (&key)[8], uint64_t row, int N, int k0, int wb, uint32_t (&w)[16]) {
  const int x0 = k0 + 16 * wb;                  // < 2N: k0 <= N - kPgTile and 16 wb < N + kPgTile
  pg_mask_block(key, row, (x0 & (N - 1)) >> 4, w);
  const uint32_t neg = x0 < N ? 0xffffffffu : 0u;   // -w = (w ^ neg) - neg
#pragma unroll
  for (int q = 0; q < 16; ++q) w[q] = (w[q] ^ neg) - neg;
}
RS_HD int pg_window_blocks(int N) { return (N + kPgTile) / 16; }

// the four noise words of coefficients k .. k + 3 (k a multiple of 4): Gaussians k .. k + 3 of stream (15, row) of the noise seed,
// i.e. the 16 words of block k / 4
RS_HD void pg_noise4(const uint32_t (&nkey)[8], uint64_t row, int k, double sigma, int32_t (&e)[4]) {
  e[0] = e[1] = e[2] = e[3] = 0;
  if (sigma == 0.0) return;
  uint32_t w[16];
  kg_chacha_block(nkey, kKgPackNoise, row, (uint32_t)(k >> 2), w);
#pragma unroll
  for (int q = 0; q < 4; ++q) e[q] = kg_noise32(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3], sigma);
}

// body row `row` of the bodies [n][t][N]
RS_HD size_t pg_body_offset(int N, uint64_t row) { return (size_t)row * (size_t)N; }
// items of pack_expand_kernel's flat grid
RS_HD long pg_expand_items(long rows, int N) { return rows * (long)(N / 16); }

}  // namespace rs
