// rs_ring_rotate.h -- encrypted rotation of packed ciphertexts (rs_ring_rotate_dev, rs_ring_rotate_alt_dev, rs_ring_heads_dev;
// include/redsec_hip.h): the index arithmetic shared by the kernels of rs_ring_rotate.hip and the lane
// emulator (rs_emulate.cpp), restated in numpy by redsec_amd/keygen.py (ring_monomial, ring_rotate, ring_heads).
//
// A chain of `depth` CMUXes (rs_ring_cmux.h) whose second input is never stored: level k selects between acc and X^(e_k) acc,
//     e_k = (step 2^k) mod 2N,    x_k = X^(e_k) acc_k - acc_k,    acc_(k+1) = acc_k + sum_j Da_j(X) S_k[j] + sum_j Db_j(X) S_k[l+j]
// over the digits of x_k (rc_digit, or rc_stage_alt / rc_digit_alt in the alternating form), so that phase(acc_depth) =
// X^(step index) phase(acc_0) + noise for the index whose bits the selectors S_k encrypt, least significant first. The placement,
// the window, the sweep and the atomics are those of ring_cmux_kernel; what is this file's own is where coefficient c of X^e acc
// is read from. Integer arithmetic only, exact in any order.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rs_ring_cmux.h"
#include "rs_rlwe.h"

namespace rs {

constexpr int kRoMaxDepth = kRcMaxDepth;     // levels of a chain: step 2^k stays inside 64 bits
constexpr int kRoInitThreads = kRcInitThreads;
constexpr int kRoHeadThreads = kRlExThreads; // threads of a workgroup of ring_heads_kernel (one output row each)

// the exponent of level k: (step 2^k) mod 2N in 0 .. 2N - 1 (N a power of two; |step 2^k| < 2^62)
RS_HD int ro_exponent(int32_t step, int k, int N) {
  return (int)((uint64_t)((int64_t)step * ((int64_t)1 << k)) & (uint64_t)(2 * N - 1));
}

// Coefficient c of X^e v, 0 <= e < 2N, is v[ro_source] negated where `negate`: with e = q N + s, 0 <= s < N, it is (-1)^q times
// word c - s + N of ext = (-v, v) (rl_ext_word), whose lower half is the negated wrap.
RS_HD int ro_source(int N, int e, int c, bool& negate) {
  const int i = c - (e & (N - 1)) + N;       // 1 .. 2N - 1
  negate = (e >= N) != (i < N);
  return i & (N - 1);
}
RS_HD uint32_t ro_rotated_word(const uint32_t* v, int N, int e, int c) {
  bool neg;
  const uint32_t w = v[ro_source(N, e, c, neg)];
  return neg ? 0u - w : w;
}

// words of one selector sample [2l][2][N] and of one row's set [depth][2l][2][N]
RS_HD size_t ro_sel_words(int N, int l) { return (size_t)2 * l * 2 * (size_t)N; }

}  // namespace rs
