// rs_ring_lookup.hip -- batched encrypted lookup (rs_ring_lookup_rows_dev, rs_ring_lookup_rows_alt_dev; include/redsec_hip.h;
// INTEGRATION.md section 28): ONE level of R CMUX trees per pair of launches,
//   ring_lookup_init_kernel       out[q][i] = prev_q[2i]
//   ring_lookup_level_kernel      out[q][i] += D_jr(X) sel_qk[jr] over one block of source coefficients, D_jr(X) = sum_c dig_j(x_c) X^c,
//                                 x = prev_q[2i + 1] - prev_q[2i] (-prev_q[2i] where row 2i + 1 does not exist), polynomial jr / l
//                                 of it, digit j = jr mod l
//   ring_lookup_level_alt_kernel  the same with the alternating digit dig'_j(x_c) = eps_c dig_j(eps_c x_c) (rs_ring_cmux.h)
// An object of its own, so that every earlier kernel keeps its instructions. Integer only, exact in any order.
//
// The sweep kernels are ring_cmux_kernel / ring_cmux_alt_kernel (rs_ring_cmux.hip, rs_ring_cmux_alt.hip) with another addressing:
// the same ring_place over (tile, polynomial, source block, selector row jr < 2l, ciphertext), the same staged window of selector
// row jr, the same ring_sweep with rc_digit (ring_sweep_parity with rc_stage_alt and rc_digit_alt, the parity that of the thread)
// and the same atomic adds onto the words the init kernel has set on the same stream just before. What is this file's own
// (rs_ring_lookup.h): the output ciphertext g of ring_place is (q, i) = (g / P, g mod P), one scalar division per workgroup; d0 is
// entry 2i of row q's table at (q row_stride + 2i entry_stride) 2N words and d1 one entry_stride further; the selector sample is
// sel + q sel_row_stride + k sel_words; and whether d1 exists (2i + 1 < rows) is a scalar branch between the two staging loops
// ring_cmux_kernel chooses between by its null d1, so the unpaired last row of every table rides in the same launch.
// rs_emu_ring_lookup_rows / rs_emu_ring_lookup_rows_alt (rs_emulate.cpp) walk the same workgroups on the CPU through the same
// functions.
// Resources (-Rpass-analysis=kernel-resource-usage): ring_lookup_level_kernel and ring_lookup_level_alt_kernel 28 VGPRs, 47 SGPRs
// (nine more than the CMUX kernels: the three strides, the level and the row count), 10.0 KB of dynamic LDS, no scratch, no static
// LDS, eight waves per SIMD; ring_lookup_init_kernel 4 VGPRs, 22 SGPRs, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_ring_lookup.h"

namespace rs {

// one workgroup per kLkInitThreads words of one output ciphertext (2 N is a multiple of kLkInitThreads): (q, i) is a scalar
__global__ __launch_bounds__(kLkInitThreads) void ring_lookup_init_kernel(RingLookupArgs a) {
  const unsigned per_ct = 2u * (unsigned)a.N / kLkInitThreads;
  const unsigned g = blockIdx.x / per_ct, w = (blockIdx.x - g * per_ct) * kLkInitThreads + threadIdx.x;
  const LkPlace at = lk_place((long)g, lk_level_rows(a.rows));
  const size_t ct = 2 * (size_t)a.N;
  a.out[(size_t)g * ct + w] = a.in[lk_source(at.q, at.i, a.row_stride, a.entry_stride) * ct + w];
}

__global__ __launch_bounds__(kRcThreads) void ring_lookup_level_kernel(RingLookupArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, t = threadIdx.x, basebit = a.basebit;
  const RingPlace pl = ring_place(blockIdx.x, N, 2 * a.l);
  const LkPlace at = lk_place(pl.r, lk_level_rows(a.rows));
  const int jr = pl.row, j = jr < a.l ? jr : jr - a.l, spoly = jr < a.l ? 0 : 1;
  uint32_t* s_win = s_lds;                                  // [kRingWindow]: ext[wb + x]
  uint32_t* s_x = s_lds + kRingWindow;                      // [kRingSlots]: x_c + offset of source coefficient c0 + cc
  const int c0 = pl.sb * kRingSlots, k0 = pl.tile * kRingTile;
  const uint32_t off = rc_offset(basebit, a.l);
  const size_t src_at = (lk_source(at.q, at.i, a.row_stride, a.entry_stride) * 2 + (size_t)spoly) * (size_t)N + (size_t)c0;
  const uint32_t* s0 = reinterpret_cast<const uint32_t*>(a.in) + src_at;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.sel) + lk_sel_offset(at.q, a.sel_row_stride, a.k, N, a.l) + rc_sel_offset(N, jr, pl.poly);
  sweep_stage_window(s_win, p, N, ring_window_base(N, k0, c0), kRingWindow, t, kRingThreads);
  if (lk_paired(at.i, a.rows)) {
    const uint32_t* s1 = s0 + a.entry_stride * 2 * (size_t)N;
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

__global__ __launch_bounds__(kRcThreads) void ring_lookup_level_alt_kernel(RingLookupArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, t = threadIdx.x, basebit = a.basebit;
  const RingPlace pl = ring_place(blockIdx.x, N, 2 * a.l);
  const LkPlace at = lk_place(pl.r, lk_level_rows(a.rows));
  const int jr = pl.row, j = jr < a.l ? jr : jr - a.l, spoly = jr < a.l ? 0 : 1;
  uint32_t* s_win = s_lds;                                  // [kRingWindow]: ext[wb + x]
  uint32_t* s_x = s_lds + kRingWindow;                      // [kRingSlots]: eps x_c + offset of source coefficient c0 + cc
  const int c0 = pl.sb * kRingSlots, k0 = pl.tile * kRingTile;
  const uint32_t off = rc_offset(basebit, a.l);
  const size_t src_at = (lk_source(at.q, at.i, a.row_stride, a.entry_stride) * 2 + (size_t)spoly) * (size_t)N + (size_t)c0;
  const uint32_t* s0 = reinterpret_cast<const uint32_t*>(a.in) + src_at;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.sel) + lk_sel_offset(at.q, a.sel_row_stride, a.k, N, a.l) + rc_sel_offset(N, jr, pl.poly);
  sweep_stage_window(s_win, p, N, ring_window_base(N, k0, c0), kRingWindow, t, kRingThreads);
  const int odd = t & 1;                                    // of every slot cc = t + i kRingThreads, and of c = c0 + cc
  if (lk_paired(at.i, a.rows)) {
    const uint32_t* s1 = s0 + a.entry_stride * 2 * (size_t)N;
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

// one level of every tree: out[q][i] = prev_q[2i], then the sweep of a.form
hipError_t launch_ring_lookup_level(const RingLookupArgs& a, hipStream_t st) {
  if (a.R <= 0) return hipSuccess;
  const long P = lk_level_rows(a.rows);
  hipLaunchKernelGGL(ring_lookup_init_kernel, dim3((unsigned)lk_init_groups(a.R, P, a.N)), dim3(kLkInitThreads), 0, st, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const size_t lds = ((size_t)2 * kRcSlots + kRcTile) * sizeof(uint32_t);
  const dim3 grid((unsigned)lk_groups(a.R, P, a.N, a.l));
  if (a.form == kRcAlternating)
    hipLaunchKernelGGL(ring_lookup_level_alt_kernel, grid, dim3(kRcThreads), lds, st, a);
  else
    hipLaunchKernelGGL(ring_lookup_level_kernel, grid, dim3(kRcThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace rs
