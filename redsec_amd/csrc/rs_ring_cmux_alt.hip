// rs_ring_cmux_alt.hip -- the alternating form of encrypted selection (rs_ring_cmux_alt_dev, rs_ring_lookup_alt_dev;
// include/redsec_hip.h):
//   ring_cmux_alt_kernel    out[r] += D'_jr(X) sel[jr] over one block of source coefficients,  D'_jr(X) = sum_k dig'_j(x_k) X^k,
//                           dig'_j(x_k) = eps_k dig_j(eps_k x_k), eps_k = +1 for even k and -1 for odd k (rs_ring_cmux.h)
// An object of its own, so that ring_cmux_kernel and every earlier kernel keep their instructions. The placement, the window, the
// LDS plan and the atomics are those of ring_cmux_kernel (rs_ring_cmux.hip), and ring_cmux_init_kernel of that file sets out = d0
// first (launch_ring_cmux). What differs is the digit, in two places:
//   - the staged source word is eps_k (d1 - d0) + off (-eps_k d0 + off under a null d1). The parity of k is the parity of the slot
//     cc, because the block base c0 is a multiple of kRingSlots = 1,024; a thread stages the slots t, t + 128, .., so it is the
//     parity of t, one choice per thread outside the loop;
//   - the digit of an odd slot is negated. ring_sweep_parity (rs_ring_sweep.h) hands the functor the parity of the slot as a
//     compile-time constant of its unrolled step, and the digit is a scalar, so the sign is one subtraction on the scalar unit for
//     two of the four slots of a step and nothing on the vector unit.
// The multiply-add count is that of ring_cmux_kernel. rs_emu_ring_cmux_alt (rs_emulate.cpp) walks the same workgroups on the CPU
// through the same ring_place and ring_sweep_parity.
// Resources (-Rpass-analysis=kernel-resource-usage): ring_cmux_alt_kernel 28 VGPRs, 38 SGPRs, 10.0 KB of dynamic LDS, no scratch, no
// static LDS, eight waves per SIMD: the figures of ring_cmux_kernel.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_ring_cmux.h"

namespace rs {

__global__ __launch_bounds__(kRcThreads) void ring_cmux_alt_kernel(RingCmuxArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, t = threadIdx.x, basebit = a.basebit;
  const RingPlace pl = ring_place(blockIdx.x, N, 2 * a.l);
  const int jr = pl.row, j = jr < a.l ? jr : jr - a.l, spoly = jr < a.l ? 0 : 1;
  uint32_t* s_win = s_lds;                                  // [kRingWindow]: ext[wb + x]
  uint32_t* s_x = s_lds + kRingWindow;                      // [kRingSlots]: eps x_k + offset of source coefficient c0 + cc
  const int c0 = pl.sb * kRingSlots, k0 = pl.tile * kRingTile;
  const uint32_t off = rc_offset(basebit, a.l);
  const size_t src_at = ((size_t)pl.r * (size_t)a.stride * 2 + (size_t)spoly) * (size_t)N + (size_t)c0;
  const uint32_t* s0 = reinterpret_cast<const uint32_t*>(a.d0) + src_at;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.sel) + rc_sel_offset(N, jr, pl.poly);
  sweep_stage_window(s_win, p, N, ring_window_base(N, k0, c0), kRingWindow, t, kRingThreads);
  const int odd = t & 1;                                    // of every slot cc = t + i kRingThreads, and of k = c0 + cc
  if (a.d1) {
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(a.d1) + src_at;
    for (int cc = t; cc < kRingSlots; cc += kRingThreads) s_x[cc] = rc_stage_alt(s1[cc] - s0[cc], off, odd);
  } else {
    for (int cc = t; cc < kRingSlots; cc += kRingThreads) s_x[cc] = rc_stage_alt(0u - s0[cc], off, odd);
  }
  __syncthreads();
  uint32_t acc[kSweepKpt] = {0u, 0u, 0u, 0u};
  ring_sweep_parity(s_win, s_x, kRingSlots, t, [=](uint32_t xbar, auto slot_odd) { return rc_digit_alt(xbar, basebit, j, decltype(slot_odd)::value); }, acc);
  unsigned int* out = reinterpret_cast<unsigned int*>(a.out) + ((size_t)pl.r * 2 + (size_t)pl.poly) * (size_t)N + k0 + kSweepKpt * t;
#pragma unroll
  for (int q = 0; q < kSweepKpt; ++q) atomicAdd(out + q, acc[q]);
}

hipError_t launch_ring_cmux_alt(const RingCmuxArgs& a, hipStream_t st) {
  if (a.R <= 0) return hipSuccess;
  const size_t lds = ((size_t)2 * kRcSlots + kRcTile) * sizeof(uint32_t);
  hipLaunchKernelGGL(ring_cmux_alt_kernel, dim3((unsigned)rc_groups(a.R, a.N, a.l)), dim3(kRcThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace rs
