// rs_audit.h -- the per-word arithmetic of device decryption and of the exact noise audit of evaluation keys (rs_phase_dev,
// rs_audit_keys_dev, rs_audit_compressed_keys_dev; include/redsec_hip.h), shared by the kernels of rs_audit.hip and the lane
// emulator (rs_emulate.cpp), restated in numpy by redsec_amd/keygen.py (bk_noise, ksk_noise, audit).
//
// Everything here is 32-bit integer arithmetic mod 2^32: a'*S is a signed sum of rotated copies of a' over the set bits of the
// binary S. No floating point, no transform, no rounding certificate: the audit shares nothing with the split-key FP64 product
// that generated the key (rs_general.h), only the ChaCha20 mask streams of rs_keygen.h for a compressed key.
#pragma once

#include <cstdint>

#include "rs_keygen.h"

namespace rs {

constexpr int kAuThreads = 256;   // threads of a workgroup of every audit kernel
constexpr int kAuKpt = 4;         // bk: coefficients a thread holds in registers per sweep of the listed bits (N >= 1024 = 256 * 4)

// ---- secret keys packed 32 bits per word (bit k & 31 of word k >> 5), zero past the key ----
RS_HD uint32_t au_key_bit(const uint32_t* packed, int k) { return (packed[k >> 5] >> (k & 31)) & 1u; }

// ---- report fields ----
// |e| of a noise word read as signed 32-bit; |INT32_MIN| = 2^31
RS_HD uint32_t au_abs(uint32_t e) { return (e & 0x80000000u) ? 0u - e : e; }
RS_HD bool au_over(uint32_t e, uint32_t limit) { return au_abs(e) > limit; }
struct AuTally { uint32_t max_abs; unsigned long long over; };
RS_HD void au_tally_word(AuTally& t, uint32_t e, uint32_t limit) {
  const uint32_t m = au_abs(e);
  if (m > t.max_abs) t.max_abs = m;
  t.over += m > limit ? 1u : 0u;
}
// all integer: the order of the merges does not matter
RS_HD void au_tally_merge(AuTally& t, const AuTally& o) {
  if (o.max_abs > t.max_abs) t.max_abs = o.max_abs;
  t.over += o.over;
}

// ---- LWE phase: b - sum_k a_k key_k of a sample of dim + 1 words ----
// lane L of a wave of 64 takes words L, L + 64, ...: consecutive lanes read consecutive words. The lane's share of the sum.
RS_HD uint32_t au_lane_dot(const uint32_t* sample, int dim, const uint32_t* key_bits, int lane) {
  uint32_t acc = 0u;
#pragma unroll 4
  for (int k = lane; k < dim; k += 64) acc += au_key_bit(key_bits, k) ? sample[k] : 0u;
  return acc;
}
// the same for a sample that is all zero by construction (ksk, v = 0): the OR of the lane's words, body included
RS_HD uint32_t au_lane_or(const uint32_t* sample, int dim, int lane) {
  uint32_t acc = 0u;
#pragma unroll 4
  for (int k = lane; k <= dim; k += 64) acc |= sample[k];
  return acc;
}

// ---- bootstrapping key ----
// row i 2l + p, p = c l + j
RS_HD void au_bk_row(uint64_t row, int l, int& i, int& c, int& j) {
  i = (int)(row / (uint64_t)(2 * l));
  const int p = (int)(row - (uint64_t)i * (uint64_t)(2 * l));
  c = p / l;
  j = p - c * l;
}
RS_HD uint32_t au_gadget(int j, int bgbit) { return 1u << (32 - (j + 1) * bgbit); }
// the set bits of word `w` of the packed S (bits 32 w .. 32 w + 31) appended to the list from position `at`; returns the new end
RS_HD int au_list_word(uint32_t bits, int w, int at, uint16_t* list) {
  for (int q = 0; q < 32; ++q)
    if ((bits >> q) & 1u) list[at++] = (uint16_t)(32 * w + q);
  return at;
}
// coefficient k of X^m a (negacyclic): a shifted up by m, the wrapped part negated
RS_HD uint32_t au_rot_term(const uint32_t* a, int N, int k, int m) {
  const uint32_t v = a[(k - m) & (N - 1)];
  return k >= m ? v : 0u - v;
}
// coefficients k0, k0 + kAuThreads, ... (kAuKpt of them) of a*S: one sweep of the `cnt` listed bits of S. Consecutive threads hold
// consecutive k0, so every read of the rotated mask is a contiguous span of words.
RS_HD void au_bk_products(const uint32_t* a, int N, const uint16_t* list, int cnt, int k0, uint32_t (&acc)[kAuKpt]) {
#pragma unroll
  for (int q = 0; q < kAuKpt; ++q) acc[q] = 0u;
  for (int b = 0; b < cnt; ++b) {
    const int m = list[b];
#pragma unroll
    for (int q = 0; q < kAuKpt; ++q) acc[q] += au_rot_term(a, N, k0 + kAuThreads * q, m);
  }
}
// the message of coefficient k of row (c, j) of key bit s: s g_j X^0 for c = 1, - s g_j S for c = 0 (the stored mask of a full
// key's c = 0 row carries the gadget term, a' = a + s g_j X^0, so b - a'*S = e - s g_j S; a compressed body holds it outright)
RS_HD uint32_t au_bk_message(int c, uint32_t s, uint32_t g, int k, uint32_t S_k) {
  return c ? (k == 0 ? s * g : 0u) : 0u - s * g * S_k;
}
RS_HD uint32_t au_bk_noise(uint32_t b, uint32_t a_times_S, uint32_t message) { return b - a_times_S - message; }

// ---- packing key (rs_audit_pack_key_dev): row i t + j is (a, b = a*S + e + s_i g_j X^0), the c = 1 formula above with t digits of
// basebit bits; a seeded key's mask is the domain-14 stream of the mask seed (kKgPackMask of rs_pack.h, restated here so that the
// audit includes nothing of the generator's) ----
constexpr uint32_t kAuPackMask = 14;
RS_HD void au_pack_row(uint64_t row, int t, int& i, int& j) {
  i = (int)(row / (uint64_t)t);
  j = (int)(row - (uint64_t)i * (uint64_t)t);
}
RS_HD void au_pack_mask_block(const uint32_t (&key)[8], uint64_t row, int blk, uint32_t (&w)[16]) {
  kg_chacha_block(key, kAuPackMask, row, (uint32_t)blk, w);
}

// ---- keyswitching key ----
// sample s = (i t + j) 2^basebit + v
RS_HD void au_ksk_sample(uint64_t s, int t, int basebit, int& i, int& j, int& v) {
  v = (int)(s & ((1ull << basebit) - 1ull));
  const uint64_t ij = s >> basebit;
  i = (int)(ij / (uint64_t)t);
  j = (int)(ij - (uint64_t)i * (uint64_t)t);
}
RS_HD uint32_t au_ksk_message(uint32_t S_i, int v, int j, int basebit) { return (S_i * (uint32_t)v) << (32 - (j + 1) * basebit); }
RS_HD uint32_t au_ksk_noise(uint32_t b, uint32_t dot, uint32_t message) { return b - dot - message; }
// compressed key: lane L's share of sum_k a_k s_k for chunk k0 of the domain-5 mask, regenerated through kg_ksk_mask_block
RS_HD uint32_t au_ksk_seeded_lane_dot(const uint32_t (&key)[8], uint64_t s, int k0, int lane, int n, const uint32_t* key_bits) {
  uint32_t w[16];
  if (!kg_ksk_mask_block(key, s, k0, lane, n, w)) return 0u;
  const uint32_t bits = kg_ct_key_bits(key_bits, k0 / 16 + lane);   // zero past n
  uint32_t acc = 0u;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc += ((bits >> q) & 1u) ? w[q] : 0u;
  return acc;
}

}  // namespace rs
