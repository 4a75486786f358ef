// rs_ring_rekey.h -- ring re-keying (rs_ring_rekey_dev; include/redsec_hip.h): the placement and the index arithmetic shared by the
// kernels of rs_ring_rekey.hip and the lane emulator (rs_emulate.cpp), restated in numpy by redsec_amd/keygen.py (ring_rekey).
//
// The public keyswitch from a ring key S to a ring key S' of the same degree N under a caller-supplied key of t + 1 ring samples,
//     out[r] = (0, b_r) - K[t] - sum_{j < t} D_j(X) K[j],    D_j(X) = sum_k d_j(k) X^k,
// K[j] = (a_j, a_j*S' + e_j + h_j S), h_j = 2^(31 - (j+1) basebit), for j < t and K[t] = (a_t, a_t*S' + e_t + c0 (1 + X + .. +
// X^(N-1)) S), c0 = (2^basebit - 1) sum_j h_j. The digits are ODD and symmetric about zero,
//     d_j(k) = 2 ((abar_k >> (32 - (j+1) basebit)) & (2^basebit - 1)) - (2^basebit - 1),    abar_k = a_k + 2^(31 - t basebit),
// so that sum_j d_j(k) h_j + c0 = abar_k rounded down to t basebit bits: the constant row carries what the centring took away, and no
// digit polynomial has a mean for the rows' common noise to add up along the coefficients. Everything
// is 32-bit integer arithmetic mod 2^32, exact in any order. No floating point and no transform. The key is made on the host
// (redsec_amd/keygen.py ring_rekey_key, or t + 1 ciphertexts of rs_rlwe_pk_encrypt_dev): none of it is in this file.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rs_ring_sweep.h"

namespace rs {

// Placement of ring_rekey_kernel: the ring placement of rs_ring_sweep.h (kRr* and rr_* name it here), the key row the digit j < t
// and the digit source the input's own a polynomial. The grid runs over (tile, polynomial, source block, digit, ciphertext):
// 2 (N / 512) (N / 1024) t workgroups per ciphertext, 4 t at N = 1024 and 256 t at N = 8192; the partial sums meet in the output by
// atomic adds on the words ring_rekey_init_kernel has set.
constexpr int kRrThreads = kRingThreads, kRrTile = kRingTile, kRrSlots = kRingSlots;
constexpr int kRrMinN = kRingMinN, kRrMaxN = kRingMaxN;
constexpr int kRrInitThreads = 256;     // threads of a workgroup of ring_rekey_init_kernel (one output word each)
constexpr int kRrMaxBits = 31;          // t basebit <= 31: h_j = 2^(31 - (j+1) basebit) is an integer

// abar = a + rr_offset: the kept bits then round to nearest instead of down
RS_HD uint32_t rr_offset(int basebit, int t) { return 1u << (31 - t * basebit); }
// the odd digit j of abar, as a word mod 2^32: 2 u - (2^basebit - 1) for u the bits 32 - (j+1) basebit .. 31 - j basebit
RS_HD uint32_t rr_digit(uint32_t abar, int basebit, int j) {
  const uint32_t mask = (1u << basebit) - 1u;
  return 2u * ((abar >> (32 - (j + 1) * basebit)) & mask) - mask;
}

// workgroups of one ciphertext and of a call
RS_HD long rr_groups_per_ct(int N, int t) { return ring_groups_per_ct(N, t); }
RS_HD long rr_groups(long R, int N, int t) { return R * rr_groups_per_ct(N, t); }

// polynomial poly of key row j of ring_key [t+1][2][N]
RS_HD size_t rr_key_offset(int N, int j, int poly) { return ((size_t)j * 2 + poly) * (size_t)N; }

}  // namespace rs
