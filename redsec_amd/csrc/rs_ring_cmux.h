// rs_ring_cmux.h -- encrypted selection on packed ciphertexts (rs_ring_cmux_dev, rs_ring_lookup_dev; include/redsec_hip.h): the
// placement and the index arithmetic shared by the kernels of rs_ring_cmux.hip and the lane emulator (rs_emulate.cpp), restated in
// numpy by redsec_amd/keygen.py (ring_cmux, ring_lookup).
//
// The external product of the difference x = d1 - d0 of two ring ciphertexts with one RGSW sample sel [2l][2][N] of a bit m,
//     out[r] = d0[r] + sum_{j < l} Da_j(X) sel[j] + sum_{j < l} Db_j(X) sel[l + j],
//     Da_j(X) = sum_k dig_j(x.a_k) X^k,  Db_j(X) = sum_k dig_j(x.b_k) X^k,
// with the signed digits of TFHE's tGswTorus32PolynomialDecompH,
//     u_j(w) = ((w + off) >> (32 - (j+1) basebit)) & (B - 1),  dig_j(w) = u_j(w) - B/2,  B = 2^basebit,
//     off = sum_j (B/2) h_j + 2^(31 - l basebit),  h_j = 2^(32 - (j+1) basebit),
// so that sum_j dig_j(w) h_j = w rounded to l basebit bits. Rows j < l of sel are ring samples of zero with m h_j added to a, rows
// l + j have m h_j added to b: phase(out) = phase(d0) + m (phase(d1) - phase(d0)) + noise. Everything is 32-bit integer arithmetic
// mod 2^32, exact in any order. No floating point and no transform. Selectors are made on the host (redsec_amd/keygen.py
// ring_selector_rows): none of it is in this file.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rs_ring_rekey.h"

namespace rs {

// Placement of ring_cmux_kernel: the ring placement of rs_ring_sweep.h (kRc* name it here), the key row the selector row jr < 2l,
// which takes digit jr mod l of polynomial jr / l of x. The grid runs over (tile, polynomial, source block, row, ciphertext):
// 2 (N / 512) (N / 1024) 2l workgroups per ciphertext; the partial sums meet in the output by atomic adds on the words
// ring_cmux_init_kernel has set.
constexpr int kRcThreads = kRingThreads, kRcTile = kRingTile, kRcSlots = kRingSlots;
constexpr int kRcMinN = kRingMinN, kRcMaxN = kRingMaxN;
constexpr int kRcInitThreads = 256;     // threads of a workgroup of ring_cmux_init_kernel (one output word each)
constexpr int kRcMaxBits = 31;          // l basebit <= 31: the half step 2^(31 - l basebit) is an integer
constexpr int kRcMaxDepth = 30;         // levels of a lookup: 2^depth entries stay below 2^31

// xbar = x + rc_offset: every digit u_j then stands B/2 above the signed digit, and the kept bits round to nearest
RS_HD uint32_t rc_offset(int basebit, int l) {
  uint32_t off = 1u << (31 - l * basebit);
  for (int j = 0; j < l; ++j) off += 1u << (31 - j * basebit);     // (B/2) h_j = 2^(31 - j basebit)
  return off;
}
// the signed digit j of xbar, as a word mod 2^32: u - B/2 for u the bits 32 - (j+1) basebit .. 31 - j basebit
RS_HD uint32_t rc_digit(uint32_t xbar, int basebit, int j) {
  return ((xbar >> (32 - (j + 1) * basebit)) & ((1u << basebit) - 1u)) - (1u << (basebit - 1));
}

// The alternating form (rs_ring_cmux_alt_dev, rs_ring_lookup_alt_dev; ring_cmux_alt_kernel, rs_ring_cmux_alt.hip): the sign of
// every other source coefficient is flipped before and after the decomposition,
//     eps_k = +1 for even k, -1 for odd k,    dig'_j(x_k) = eps_k dig_j(eps_k x_k),
// with dig_j, off and h_j those above. sum_j dig'_j(x_k) h_j is still x_k rounded to l basebit bits within the same half step, so
// the same RGSW samples select; the digit at position k has mean -eps_k / 2 instead of -1/2, and the digits lie in -B/2 .. B/2.
// The forms of RingCmuxArgs (rs_kernels.h); zero, the value-initialised one, is the signed digit.
constexpr int kRcSigned = 0, kRcAlternating = 1;
// the word staged for source coefficient k of x = d1 - d0: eps_k x + off (odd: the parity of k, 0 or 1)
RS_HD uint32_t rc_stage_alt(uint32_t x, uint32_t off, int odd) { return (odd ? 0u - x : x) + off; }
// digit j of that staged word: eps_k dig_j
RS_HD uint32_t rc_digit_alt(uint32_t xbar, int basebit, int j, int odd) {
  const uint32_t d = rc_digit(xbar, basebit, j);
  return odd ? 0u - d : d;
}

// workgroups of one ciphertext and of a launch
RS_HD long rc_groups_per_ct(int N, int l) { return ring_groups_per_ct(N, 2 * l); }
RS_HD long rc_groups(long R, int N, int l) { return R * rc_groups_per_ct(N, l); }

// polynomial poly of selector row jr of sel [2l][2][N]
RS_HD size_t rc_sel_offset(int N, int jr, int poly) { return ((size_t)jr * 2 + poly) * (size_t)N; }

// rs_ring_lookup_dev: level k halves the rows. rows -> pairs (2r, 2r + 1) and, for an odd count, one unpaired last row
RS_HD long rc_level_rows(long rows) { return (rows + 1) / 2; }
// rows of scratch: ceil(E / 2) of the first half and ceil(E / 4) of the second
RS_HD long rc_scratch_rows(long entries) { return rc_level_rows(entries) + rc_level_rows(rc_level_rows(entries)); }

}  // namespace rs
