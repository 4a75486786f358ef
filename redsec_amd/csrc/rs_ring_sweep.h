// rs_ring_sweep.h -- the negacyclic digit sweep of the ring pipeline, written once: ring_rekey_kernel (rs_ring_rekey.hip),
// ring_cmux_kernel (rs_ring_cmux.hip) and the lane emulators rs_emu_pack, rs_emu_ring_rekey and rs_emu_ring_cmux (rs_emulate.cpp)
// all compile the functions below, so the CPU tests run the loop that the device runs. pack_kernel (rs_pack.hip) keeps ring_sweep
// written out, the one copy left: as a call it measured slower there (see that file's header).
// Integer only: a digit times a 32-bit word, accumulated mod 2^32, exact in any order. ring_sweep_parity is the same loop for a
// digit that depends on the parity of its slot: ring_cmux_alt_kernel (rs_ring_cmux_alt.hip) and rs_emu_ring_cmux_alt compile it.
//
// The sweep adds D(X) p to four coefficients of a thread, D(X) = sum_cc digit(src[cc]) X^(c0 + cc) over `slots` source words and p
// one key polynomial mod X^N + 1. The workgroup has staged the window of ext = (-p, p) (rs_rlwe.h) that its tile of coefficients
// and its slots read: coefficient k0 + x of X^(c0 + cc) p is window word x - cc + slots, the wrapped part already negated, so the
// sweep has neither a sign nor a wrap in it. Thread t keeps coefficients k0 + 4t .. k0 + 4t + 3 in acc. Four consecutive slots need
// seven window words: two aligned 16-byte chunks, of which the upper one is the previous step's lower one, so ONE 16-byte LDS read
// per thread (the compiler splits it into two or three narrower ds_read instructions) serves 16 multiply-adds. The four source words of
// a step are one more 16-byte read at the same address in every lane (ds_read_b128, a broadcast); each is made a scalar
// (readfirstlane) and the digit functor then runs on the scalar unit: shift, mask and whatever centring the caller's digit has.
// Multiply-add form (tools/isa_scan.py on rs_pack, rs_ring_rekey and rs_ring_cmux): per four slots and lane 16 v_mul_lo_u32 with the scalar digit as one
// operand and 8 v_add3_u32 that fold the adds pairwise; no v_mad_u64_u32, whose 64-bit accumulator would double the registers of
// acc for the same 4.3-cycle issue (MEASUREMENTS.md section 4.1).
//
// The ring placement below is what ring_rekey_kernel and ring_cmux_kernel share beyond the sweep: one tile of kRingTile coefficients
// of one polynomial of one output ciphertext, ONE full block of kRingSlots source coefficients and ONE key row per workgroup.
#pragma once

#include <cstdint>
#include <type_traits>

#include "rs_rlwe.h"

namespace rs {

constexpr int kSweepKpt = 4;            // coefficients a thread keeps in registers: one 16-byte chunk of the window

// a word that is the same in every lane, handed to the scalar unit; the identity on the host
RS_HD uint32_t sweep_uniform(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
  return v;
#endif
}

// the four words of the 16-byte chunk at p, p 16-byte aligned: a copy that every compiler may turn into one 16-byte load (on the
// device it is the load of a uint4) and that reads no word through a pointer to another type
RS_HD void sweep_load4(const uint32_t* p, uint32_t (&o)[4]) {
  __builtin_memcpy(o, __builtin_assume_aligned(p, 16), sizeof(o));
}

// Thread t of `step` stages its words of the window win[x] = ext[wb + x], x < words (the host walks it with t = 0, step = 1 or
// thread by thread: the words are the same).
RS_HD void sweep_stage_window(uint32_t* win, const uint32_t* p, int N, int wb, int words, int t, int step) {
  for (int x = t; x < words; x += step) win[x] = rl_ext_word(p, N, wb + x);
}

// acc[q] += sum_{cc < slots} win[4t + q - cc + slots] digit(src[cc]); slots a multiple of 4, win and src 16-byte aligned,
// win of slots + 4 (threads of the workgroup) words
template <class Digit>
RS_HD void ring_sweep(const uint32_t* win, const uint32_t* src, int slots, int t, Digit digit, uint32_t (&acc)[kSweepKpt]) {
  int c4 = t + slots / 4;                                   // chunk of window words 4t + slots - cc .. + 3, cc = 0
  uint32_t lo[4], hi[4], s[4];                              // window words 4 c4 .. + 3 and 4 c4 + 4 .. + 7
  sweep_load4(win + 4 * c4, hi);
  for (int q4 = 0; q4 < slots / 4; ++q4) {                  // slots cc = 4 q4 .. 4 q4 + 3
    sweep_load4(src + 4 * q4, s);                           // the same four words in every lane: scalars
    const uint32_t d[4] = {digit(sweep_uniform(s[0])), digit(sweep_uniform(s[1])), digit(sweep_uniform(s[2])), digit(sweep_uniform(s[3]))};
    sweep_load4(win + 4 * --c4, lo);
#pragma unroll
    for (int b = 0; b < 4; ++b) {                           // slot cc = 4 q4 + b: coefficient 4t + q takes window word 4 c4 + 4 + q - b
#pragma unroll
      for (int q = 0; q < kSweepKpt; ++q) acc[q] += (q >= b ? hi[q - b] : lo[4 + q - b]) * d[b];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) hi[q] = lo[q];              // the upper chunk of the next step
  }
}

// The sibling of ring_sweep for a digit that depends on the parity of its slot: acc[q] += sum_cc win[..] digit(src[cc], cc & 1),
// the alternating digit of ring_cmux_alt_kernel (rs_ring_cmux_alt.hip) and rs_emu_ring_cmux_alt. The slot index of a step is a
// constant of the unrolled loop, so the functor receives the parity as a std::integral_constant: the form of the digit is chosen at
// compile time and costs no select. A second copy of the loop and not ring_sweep as a call of this one: as such a call,
// ring_rekey_kernel and ring_cmux_kernel changed instructions (tools/codeobj_digest.py), and they are to keep them.
template <class Digit>
RS_HD void ring_sweep_parity(const uint32_t* win, const uint32_t* src, int slots, int t, Digit digit, uint32_t (&acc)[kSweepKpt]) {
  const std::integral_constant<int, 0> even{};
  const std::integral_constant<int, 1> odd{};
  int c4 = t + slots / 4;
  uint32_t lo[4], hi[4], s[4];
  sweep_load4(win + 4 * c4, hi);
  for (int q4 = 0; q4 < slots / 4; ++q4) {
    sweep_load4(src + 4 * q4, s);
    const uint32_t d[4] = {digit(sweep_uniform(s[0]), even), digit(sweep_uniform(s[1]), odd), digit(sweep_uniform(s[2]), even),
                           digit(sweep_uniform(s[3]), odd)};
    sweep_load4(win + 4 * --c4, lo);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
      for (int q = 0; q < kSweepKpt; ++q) acc[q] += (q >= b ? hi[q - b] : lo[4 + q - b]) * d[b];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) hi[q] = lo[q];
  }
}

// ---- the placement of ring_rekey_kernel and ring_cmux_kernel ----
// A workgroup of kRingThreads threads owns kRingTile = 4 kRingThreads consecutive output coefficients of one polynomial of one
// ciphertext, one block of kRingSlots consecutive source coefficients and one key row. N is a power of two in kRingMinN ..
// kRingMaxN, so a source block is always full and a tile never straddles a polynomial.
constexpr int kRingThreads = 128, kRingTile = kRingThreads * kSweepKpt;
constexpr int kRingMinN = 1024, kRingMaxN = 8192;
constexpr int kRingSlots = 1024;        // source coefficients of a block: bounds the LDS of a workgroup on every ring
constexpr int kRingWindow = kRingSlots + kRingTile;   // words of the staged window

RS_HD int ring_tiles(int N) { return N / kRingTile; }
RS_HD int ring_blocks(int N) { return N / kRingSlots; }
// workgroups of one ciphertext with `rows` key rows
RS_HD long ring_groups_per_ct(int N, int rows) { return 2L * ring_tiles(N) * ring_blocks(N) * rows; }

// workgroup g of the grid over (tile, polynomial, source block, row, ciphertext)
struct RingPlace {
  int tile, poly, sb, row;
  long r;
};
RS_HD RingPlace ring_place(unsigned g, int N, int rows) {
  const unsigned tiles = (unsigned)ring_tiles(N), blocks = (unsigned)ring_blocks(N);
  RingPlace pl;
  pl.tile = (int)(g % tiles); g /= tiles;
  pl.poly = (int)(g & 1u); g >>= 1;
  pl.sb = (int)(g % blocks); g /= blocks;
  pl.row = (int)(g % (unsigned)rows);
  pl.r = (long)(g / (unsigned)rows);
  return pl;
}

// A workgroup with first coefficient k0 and first source coefficient c0 stages the words ext[ring_window_base + i], i < kRingWindow.
// 0 <= ring_window_base and ring_window_base + kRingWindow <= 2 N for every tile and block.
RS_HD int ring_window_base(int N, int k0, int c0) { return rl_term_index(N, k0, c0) - kRingSlots; }

}  // namespace rs
