// rs_rlwe.h -- compact RLWE public keys (rs_rlwe_pk_encrypt_dev, rs_rlwe_extract_dev; include/redsec_hip.h): the streams and the
// index arithmetic shared by the kernels of rs_rlwe.hip and the lane emulator (rs_emulate.cpp), restated in numpy by
// redsec_amd/keygen.py (rlwe_pk_selector, rlwe_pk_encrypt, rlwe_extract).
//
// A public key is (a, b = a*S + e) over Z[X]/(X^N + 1) mod 2^32; ciphertext r of a call is (a*u + e1, b*u + e2 + m) with u a
// uniform binary polynomial. Streams (rs_keygen.h), all of row first + r of the encryptor's PRIVATE rand seed:
//     domain 12  selector   u_k = (word k >> 5 >> (k & 31)) & 1, k < N
//     domain 13  noise      Gaussian g from words 4g .. 4g+3: Gaussians 0 .. N-1 are e1, N .. 2N-1 are e2
// (domains 10 and 11, the key's mask and noise, are used on the owner's side only: redsec_amd/keygen.py.)
#pragma once

#include <cstdint>

#include "rs_keygen.h"

namespace rs {

enum { kKgRlweMask = 10, kKgRlweNoise = 11, kKgRlweSelect = 12, kKgRlweEncNoise = 13 };

// Placement of rlwe_pk_encrypt_kernel: a workgroup of kRlThreads threads owns kRlTile = 4 kRlThreads consecutive output
// coefficients of one polynomial of one ciphertext, thread t the four coefficients k0 + 4t .. k0 + 4t + 3 in registers; the grid
// runs over (ciphertext, polynomial, tile). N is a power of two in kRlMinN .. kRlMaxN, so a tile never straddles a polynomial.
constexpr int kRlThreads = 128, kRlKpt = 4, kRlTile = kRlThreads * kRlKpt;
constexpr int kRlMinN = 1024, kRlMaxN = 8192;
constexpr int kRlExThreads = 256;   // threads of a workgroup of rlwe_extract_kernel (one output row each)

// selector words 16 blk .. 16 blk + 15 of ciphertext row `row` (bits 512 blk .. 512 blk + 511 of u): block blk of stream (12, row)
RS_HD void rl_select_block(const uint32_t (&key)[8], uint64_t row, uint32_t blk, uint32_t (&w)[16]) {
  kg_chacha_block(key, kKgRlweSelect, row, blk, w);
}
RS_HD uint32_t rl_select_bit(const uint32_t* words, int k) { return (words[k >> 5] >> (k & 31)) & 1u; }

// the four noise words of coefficients k .. k + 3 (k a multiple of 4) of polynomial `poly` (0: e1, 1: e2): Gaussians poly N + k ..
// of stream (13, row), i.e. the 16 words of block (poly N + k) / 4
RS_HD void rl_noise4(const uint32_t (&key)[8], uint64_t row, int poly, int N, int k, double sigma, int32_t (&e)[4]) {
  e[0] = e[1] = e[2] = e[3] = 0;
  if (sigma == 0.0) return;
  uint32_t w[16];
  kg_chacha_block(key, kKgRlweEncNoise, row, (uint32_t)((poly * N + k) >> 2), w);
  for (int q = 0; q < 4; ++q) e[q] = kg_noise32(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3], sigma);
}

// The key polynomial p is staged as the 2N words ext = (-p, p): coefficient k of X^j p (negacyclic) is ext[rl_term_index(N, k, j)],
// the wrapped part (j > k) already negated.
RS_HD int rl_term_index(int N, int k, int j) { return k - j + N; }
RS_HD uint32_t rl_ext_word(const uint32_t* p, int N, int i) { return i < N ? 0u - p[i] : p[i - N]; }

// Sample extraction: word j < N of the LWE sample of coefficient c is a[c - j] for j <= c and -a[N + c - j] for j > c, word N is
// b[c] (the convention of rs_bootstrap_wo_ks_dev's output, so that the phase under S read as an LWE key is that of coefficient c).
RS_HD int rl_extract_index(int N, int c, int j, bool& negate) {
  negate = j > c;
  return (c - j) & (N - 1);
}
RS_HD uint32_t rl_extract_word(const uint32_t* a, const uint32_t* b, int N, int c, int j) {
  if (j == N) return b[c];
  bool neg;
  const uint32_t v = a[rl_extract_index(N, c, j, neg)];
  return neg ? 0u - v : v;
}

}  // namespace rs
