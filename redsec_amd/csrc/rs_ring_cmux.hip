// rs_ring_cmux.hip -- encrypted selection on packed ciphertexts (rs_ring_cmux_dev, rs_ring_lookup_dev; include/redsec_hip.h):
//   ring_cmux_init_kernel   out[r] = d0[r stride]
//   ring_cmux_kernel        out[r] += D_jr(X) sel[jr] over one block of source coefficients,  D_jr(X) = sum_k dig_j(x_k) X^k,
//                           x = d1[r stride] - d0[r stride], polynomial jr / l of it, digit j = jr mod l
// An object of its own, so that every earlier kernel keeps its instructions. Integer only: a signed digit of basebit bits times a
// 32-bit word, accumulated mod 2^32, exact in any order, so neither the tiling nor the number of blocks can change a word.
//
// ring_cmux_kernel is the ring placement and ring_sweep of rs_ring_sweep.h (the LDS read pattern, the scalar digit and the
// multiply-add form are described there) with one workgroup per (tile, polynomial, source block, selector row jr < 2l, ciphertext):
// the grid is 2 (N / 512) (N / 1024) 2l workgroups per ciphertext, 8 l at N = 1024 and 512 l at N = 8192. What is this kernel's
// own: the staged source words are d1 - d0 + off of polynomial jr / l (1,024 words, beside the 1,024 + 512 of the window of
// selector row jr; -d0 + off under a null d1, the same choice in every workgroup of a launch); the digit is rc_digit, digit jr mod l
// with B/2 taken off; and the partial sums are ADDED to the output. They meet by vector atomicAdd (global_atomic_add_u32, no
// return) on the words ring_cmux_init_kernel has set on the same stream just before; every call initialises again, so a second
// call into the same buffer gives the same words. rs_emu_ring_cmux (rs_emulate.cpp) walks the same workgroups on the CPU through
// the same ring_place and ring_sweep.
// Resources (-Rpass-analysis=kernel-resource-usage): ring_cmux_kernel 28 VGPRs, 38 SGPRs, 10.0 KB of dynamic LDS, no scratch, no
// static LDS, eight waves per SIMD; ring_cmux_init_kernel 4 VGPRs, 21 SGPRs, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_ring_cmux.h"

namespace rs {

// one workgroup per kRcInitThreads words of one ciphertext (2 N is a multiple of kRcInitThreads): the row is a scalar
__global__ __launch_bounds__(kRcInitThreads) void ring_cmux_init_kernel(RingCmuxArgs a) {
  const unsigned per_ct = 2u * (unsigned)a.N / kRcInitThreads;
  const unsigned r = blockIdx.x / per_ct, w = (blockIdx.x - r * per_ct) * kRcInitThreads + threadIdx.x;
  const size_t ct = 2 * (size_t)a.N;
  a.out[(size_t)r * ct + w] = a.d0[(size_t)r * (size_t)a.stride * ct + w];
}

__global__ __launch_bounds__(kRcThreads) void ring_cmux_kernel(RingCmuxArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, t = threadIdx.x, basebit = a.basebit;
  const RingPlace pl = ring_place(blockIdx.x, N, 2 * a.l);
  const int jr = pl.row, j = jr < a.l ? jr : jr - a.l, spoly = jr < a.l ? 0 : 1;
  uint32_t* s_win = s_lds;                                  // [kRingWindow]: ext[wb + x]
  uint32_t* s_x = s_lds + kRingWindow;                      // [kRingSlots]: x_k + offset of source coefficient c0 + cc
  const int c0 = pl.sb * kRingSlots, k0 = pl.tile * kRingTile;
  const uint32_t off = rc_offset(basebit, a.l);
  const size_t src_at = ((size_t)pl.r * (size_t)a.stride * 2 + (size_t)spoly) * (size_t)N + (size_t)c0;
  const uint32_t* s0 = reinterpret_cast<const uint32_t*>(a.d0) + src_at;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.sel) + rc_sel_offset(N, jr, pl.poly);
  sweep_stage_window(s_win, p, N, ring_window_base(N, k0, c0), kRingWindow, t, kRingThreads);
  if (a.d1) {
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(a.d1) + src_at;
    for (int cc = t; cc < kRingSlots; cc += kRingThreads) s_x[cc] = s1[cc] - s0[cc] + off;
  } else {
    for (int cc = t; cc < kRingSlots; cc += kRingThreads) s_x[cc] = off - s0[cc];
  }
  __syncthreads();
  uint32_t acc[kSweepKpt] = {0u, 0u, 0u, 0u};
  ring_sweep(s_win, s_x, kRingSlots, t, [=](uint32_t xbar) { return rc_digit(xbar, basebit, j); }, acc);
  unsigned int* out = reinterpret_cast<unsigned int*>(a.out) + ((size_t)pl.r * 2 + (size_t)pl.poly) * (size_t)N + k0 + kSweepKpt * t;
#pragma unroll
  for (int q = 0; q < kSweepKpt; ++q) atomicAdd(out + q, acc[q]);
}

hipError_t launch_ring_cmux(const RingCmuxArgs& a, hipStream_t st) {
  if (a.R <= 0) return hipSuccess;
  const long init_groups = a.R * (2 * (long)a.N / kRcInitThreads);
  hipLaunchKernelGGL(ring_cmux_init_kernel, dim3((unsigned)init_groups), dim3(kRcInitThreads), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.form == kRcAlternating) return launch_ring_cmux_alt(a, st);      // the alternating digit: a kernel in an object of its own
  const size_t lds = ((size_t)2 * kRcSlots + kRcTile) * sizeof(uint32_t);
  hipLaunchKernelGGL(ring_cmux_kernel, dim3((unsigned)rc_groups(a.R, a.N, a.l)), dim3(kRcThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace rs
