// rs_keygen.h -- the random streams of evaluation-key generation (rs_keygen_dev, include/redsec_hip.h), shared by the device
// kernels (rs_general.hip), the lane emulator (rs_emulate.cpp) and restated in numpy by redsec_amd/keygen.py.
//
// Stream (domain, row) of a 32-byte seed: word w is word w & 15 of the ChaCha20 block (RFC 8439 section 2.3, 20 rounds, input
// added back) whose state is
//     words 0-3    "expand 32-byte k"
//     words 4-11   the seed as 8 little-endian words
//     word 12      the block counter w >> 4 within the row
//     words 13-15  domain, row & 0xffffffff, row >> 32
// Gaussian g of a row consumes words 4g .. 4g+3:
//     u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) 2^-53   in (0, 1]
//     u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53       in [0, 1)
//     z  = sqrt(-2 ln u1) cos(2 pi u2)               (2 pi as the double 6.283185307179586)
// and the noise word is TFHE's dtot32(sigma z): the fractional part of sigma z (truncated toward zero) times 2^32, converted to
// int64, wrapped to 32 bits.
#pragma once

#include <cmath>
#include <cstdint>

#include "rs_ntt.h"

namespace rs {

// domains (the table of include/redsec_hip.h, rs_keygen_dev)
enum { kKgLweSecret = 1, kKgTlweSecret = 2, kKgBkMask = 3, kKgBkNoise = 4, kKgKsMask = 5, kKgKsNoise = 6, kKgCtMask = 7, kKgCtNoise = 8, kKgPkSelect = 9 };

RS_HD uint32_t kg_rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
RS_HD void kg_quarter(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  a += b; d ^= a; d = kg_rotl(d, 16);
  c += d; b ^= c; b = kg_rotl(b, 12);
  a += b; d ^= a; d = kg_rotl(d, 8);
  c += d; b ^= c; b = kg_rotl(b, 7);
}

// the 16 words of block `block` of stream (domain, row)
RS_HD void kg_chacha_block(const uint32_t (&key)[8], uint32_t domain, uint64_t row, uint32_t block, uint32_t (&out)[16]) {
  uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                     block, domain, (uint32_t)row, (uint32_t)(row >> 32)};
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll 1
  for (int r = 0; r < 10; ++r) {
    kg_quarter(x[0], x[4], x[8], x[12]);
    kg_quarter(x[1], x[5], x[9], x[13]);
    kg_quarter(x[2], x[6], x[10], x[14]);
    kg_quarter(x[3], x[7], x[11], x[15]);
    kg_quarter(x[0], x[5], x[10], x[15]);
    kg_quarter(x[1], x[6], x[11], x[12]);
    kg_quarter(x[2], x[7], x[8], x[13]);
    kg_quarter(x[3], x[4], x[9], x[14]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = x[i] + in[i];
}

RS_HD double kg_u1(uint32_t w0, uint32_t w1) {
  return (double)((((uint64_t)(w0 >> 5)) << 26) + (uint64_t)(w1 >> 6) + 1u) * 0x1p-53;
}
RS_HD double kg_u2(uint32_t w2, uint32_t w3) {
  return (double)((((uint64_t)(w2 >> 5)) << 26) + (uint64_t)(w3 >> 6)) * 0x1p-53;
}
// dtot32(sigma z) of the Gaussian made from four stream words; sigma = 0 gives 0 without evaluating anything
RS_HD int32_t kg_noise32(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, double sigma) {
  if (sigma == 0.0) return 0;
  const double z = sqrt(-2.0 * log(kg_u1(w0, w1))) * cos(6.283185307179586 * kg_u2(w2, w3));
  const double e = sigma * z;
  return (int32_t)(uint32_t)(uint64_t)(int64_t)((e - trunc(e)) * 4294967296.0);
}

// ---- the mask streams of a key, shared by key generation and expansion (rs_keygen_dev, rs_keygen_compressed_dev,
// rs_expand_keys_dev) so that the words of the two paths cannot drift apart; the lane emulator runs them for the CPU tests ----

// bk row `row`, thread t of the row's N / 16: mask words 16 t .. 16 t + 15 = block t of stream (3, row)
RS_HD void kg_bk_mask_block(const uint32_t (&key)[8], uint64_t row, int t, uint32_t (&w)[16]) {
  kg_chacha_block(key, kKgBkMask, row, (uint32_t)t, w);
}

// ksk sample s, lane L of its wave, chunk k0 (a multiple of 1024) of the n mask words: block k0 / 16 + L of stream (5, s),
// i.e. words k0 + 16 L .. k0 + 16 L + 15; false (w untouched) when that block lies past the mask
RS_HD bool kg_ksk_mask_block(const uint32_t (&key)[8], uint64_t s, int k0, int lane, int n, uint32_t (&w)[16]) {
  const int blk = k0 / 16 + lane;
  if (16 * blk >= n) return false;
  kg_chacha_block(key, kKgKsMask, s, (uint32_t)blk, w);
  return true;
}
// the LDS transpose of a chunk: lane L writes its block to buf[16 L + q]; the coalesced read of round q at lane L takes buf[64 q + L],
// mask word k0 + 64 q + L
constexpr int kKgChunk = 64 * 16;
RS_HD int kg_ksk_chunk_word(int q, int lane) { return 64 * q + lane; }

// ---- seeded LWE ciphertexts (rs_encrypt_seeded_dev, rs_expand_ciphertexts_dev), shared by seeded_lwe_kernel, the lane emulator
// and the TFHE shim's host writer and reader ----

// ciphertext row `row`: mask words 16 blk .. 16 blk + 15 = block blk of stream (7, row) of the mask seed
RS_HD void kg_ct_mask_block(const uint32_t (&key)[8], uint64_t row, int blk, uint32_t (&w)[16]) {
  kg_chacha_block(key, kKgCtMask, row, (uint32_t)blk, w);
}
// its noise word: Gaussian 0 (words 0-3) of stream (8, row) of the noise seed
RS_HD int32_t kg_ct_noise(const uint32_t (&nkey)[8], uint64_t row, double sigma) {
  if (sigma == 0.0) return 0;
  uint32_t w[16];
  kg_chacha_block(nkey, kKgCtNoise, row, 0u, w);
  return kg_noise32(w[0], w[1], w[2], w[3], sigma);
}
// the 16 key bits of block blk (words 16 blk .. 16 blk + 15) from the key packed 32 bits per word, bit k & 31 of word k >> 5
RS_HD uint32_t kg_ct_key_bits(const uint32_t* packed, int blk) { return (packed[blk >> 1] >> ((blk & 1) * 16)) & 0xffffu; }

// Placement of seeded_lwe_kernel: a workgroup of kCtThreads threads owns a tile of C whole ciphertexts and walks the flat index
// item = c nblk + blk (nblk = ceil(n / 16) ChaCha blocks per mask) in strides of kCtThreads; word k of tile ciphertext c is staged
// at LDS word c (n + 1) + k, the tile is then stored as one contiguous span of C (n + 1) words. C is the tile size <= kCtMaxTile
// whose staging fits kCtLdsWords and whose C nblk items leave the fewest lanes idle in the last stride (ties: the larger tile).
constexpr int kCtThreads = 256, kCtLdsWords = 12800, kCtMaxTile = 64;
RS_HD int kg_ct_blocks(int n) { return (n + 15) / 16; }
RS_HD int kg_ct_tile(int n) {
  const int nblk = kg_ct_blocks(n);
  int cap = kCtLdsWords / (n + 1);
  if (cap > kCtMaxTile) cap = kCtMaxTile;
  if (cap < 1) cap = 1;
  int best = 0;
  long best_idle = 0, best_slots = 1;
  for (int C = 1; C <= cap; ++C) {
    const long items = (long)C * nblk, slots = (items + kCtThreads - 1) / kCtThreads * kCtThreads;
    if ((slots - items) * best_slots <= best_idle * slots || best == 0) { best = C; best_idle = slots - items; best_slots = slots; }
  }
  return best;
}
RS_HD int kg_ct_lds_word(int c, int k, int n) { return c * (n + 1) + k; }

// ---- public-key encryption (rs_pk_encrypt_dev), shared by pk_encrypt_kernel (rs_pubkey.hip) and the lane emulator ----

// Selection bits of ciphertext row `row` for the public-key rows 512 chunk .. 512 chunk + 511: block `chunk` of stream (9, row) of
// the encryptor's private rand seed. Bit j of the ciphertext (row j of the key is added when it is set) is bit j & 31 of stream word
// j >> 5, i.e. of w[(j >> 5) & 15] of chunk j >> 9; bits at j >= m are never looked at.
constexpr int kPkChunk = 512;
RS_HD void kg_pk_select_block(const uint32_t (&key)[8], uint64_t row, uint32_t chunk, uint32_t (&w)[16]) {
  kg_chacha_block(key, kKgPkSelect, row, chunk, w);
}
// Placement of pk_encrypt_kernel: a workgroup of kPkThreads threads owns kPkTile ciphertexts x kPkThreads words of the row (lane =
// word), one accumulator per ciphertext in registers; the grid runs over (ciphertext tile, word tile).
constexpr int kPkTile = 16, kPkThreads = 256;

// seed bytes -> the 8 little-endian key words
RS_HD void kg_seed_words(const uint8_t* seed, uint32_t (&key)[8]) {
  for (int k = 0; k < 8; ++k)
    key[k] = (uint32_t)seed[4 * k] | ((uint32_t)seed[4 * k + 1] << 8) | ((uint32_t)seed[4 * k + 2] << 16) | ((uint32_t)seed[4 * k + 3] << 24);
}

}  // namespace rs
