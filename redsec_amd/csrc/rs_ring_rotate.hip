// rs_ring_rotate.hip -- encrypted rotation of packed ciphertexts (rs_ring_rotate_dev, rs_ring_rotate_alt_dev, rs_ring_heads_dev;
// include/redsec_hip.h):
//   ring_rotate_init_kernel  out[r] = in[r stride]                                    (stride 0: every row starts from in[0])
//   ring_rotate_kernel       out[r] += D_jr(X) sel_r[jr] over one block of source coefficients, D_jr(X) = sum_k dig_j(x_k) X^k,
//                            x = X^e in[r stride] - in[r stride], polynomial jr / l of it, digit j = jr mod l
//   ring_rotate_alt_kernel   the same with the alternating digit dig'_j(x_k) = eps_k dig_j(eps_k x_k) (rs_ring_cmux.h)
//   ring_heads_kernel        u[r width + c] = the LWE sample of coefficient c < width of rlwe[r]
// An object of its own, so that every earlier kernel keeps its instructions. Integer only, exact in any order.
//
// One level of a rotation is a CMUX between acc and X^e acc. ring_rotate_kernel is ring_cmux_kernel (rs_ring_cmux.hip) with another
// source: the same ring_place over (tile, polynomial, source block, selector row jr < 2l, ciphertext), the same staged window of
// selector row jr, the same ring_sweep with rc_digit and the same atomic adds onto the words the init kernel has set on the same
// stream just before. The staged word of source coefficient c is (X^e acc)_c - acc_c + off: the rotated word is read straight from
// the level's input at ro_source (rs_ring_rotate.h; one shifted, sign-flipped read beside the plain one, both consecutive across
// the lanes but for the one wrap), so X^e acc is never written to memory. The selector row pointer takes sel_stride words per
// ciphertext (zero: one hidden index for all rows). ring_rotate_alt_kernel stages rc_stage_alt of the same difference, the parity
// that of the thread as in ring_cmux_alt_kernel, and sweeps with ring_sweep_parity and rc_digit_alt. rs_emu_ring_rotate /
// rs_emu_ring_rotate_alt (rs_emulate.cpp) walk the same workgroups on the CPU through the same functions.
// Resources (-Rpass-analysis=kernel-resource-usage): ring_rotate_kernel and ring_rotate_alt_kernel 28 VGPRs, 41 SGPRs (three more
// than the CMUX kernels: the exponent and the selector stride), 10.0 KB of dynamic LDS, no scratch, no static LDS, eight waves per
// SIMD; ring_rotate_init_kernel 4 VGPRs, 21 SGPRs; ring_heads_kernel 8 VGPRs, 29 SGPRs; neither with LDS or scratch.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_ring_rotate.h"

namespace rs {

// one workgroup per kRoInitThreads words of one ciphertext (2 N is a multiple of kRoInitThreads): the row is a scalar
__global__ __launch_bounds__(kRoInitThreads) void ring_rotate_init_kernel(RingRotateArgs a) {
  const unsigned per_ct = 2u * (unsigned)a.N / kRoInitThreads;
  const unsigned r = blockIdx.x / per_ct, w = (blockIdx.x - r * per_ct) * kRoInitThreads + threadIdx.x;
  const size_t ct = 2 * (size_t)a.N;
  a.out[(size_t)r * ct + w] = a.in[(size_t)r * (size_t)a.stride * ct + w];
}

__global__ __launch_bounds__(kRcThreads) void ring_rotate_kernel(RingRotateArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, t = threadIdx.x, basebit = a.basebit, e = a.e;
  const RingPlace pl = ring_place(blockIdx.x, N, 2 * a.l);
  const int jr = pl.row, j = jr < a.l ? jr : jr - a.l, spoly = jr < a.l ? 0 : 1;
  uint32_t* s_win = s_lds;                                  // [kRingWindow]: ext[wb + x]
  uint32_t* s_x = s_lds + kRingWindow;                      // [kRingSlots]: x_k + offset of source coefficient c0 + cc
  const int c0 = pl.sb * kRingSlots, k0 = pl.tile * kRingTile;
  const uint32_t off = rc_offset(basebit, a.l);
  const uint32_t* v = reinterpret_cast<const uint32_t*>(a.in) + ((size_t)pl.r * (size_t)a.stride * 2 + (size_t)spoly) * (size_t)N;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.sel) + (size_t)pl.r * a.sel_stride + rc_sel_offset(N, jr, pl.poly);
  sweep_stage_window(s_win, p, N, ring_window_base(N, k0, c0), kRingWindow, t, kRingThreads);
  for (int cc = t; cc < kRingSlots; cc += kRingThreads) s_x[cc] = ro_rotated_word(v, N, e, c0 + cc) - v[c0 + cc] + off;
  __syncthreads();
  uint32_t acc[kSweepKpt] = {0u, 0u, 0u, 0u};
  ring_sweep(s_win, s_x, kRingSlots, t, [=](uint32_t xbar) { return rc_digit(xbar, basebit, j); }, acc);
  unsigned int* out = reinterpret_cast<unsigned int*>(a.out) + ((size_t)pl.r * 2 + (size_t)pl.poly) * (size_t)N + k0 + kSweepKpt * t;
#pragma unroll
  for (int q = 0; q < kSweepKpt; ++q) atomicAdd(out + q, acc[q]);
}

__global__ __launch_bounds__(kRcThreads) void ring_rotate_alt_kernel(RingRotateArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, t = threadIdx.x, basebit = a.basebit, e = a.e;
  const RingPlace pl = ring_place(blockIdx.x, N, 2 * a.l);
  const int jr = pl.row, j = jr < a.l ? jr : jr - a.l, spoly = jr < a.l ? 0 : 1;
  uint32_t* s_win = s_lds;                                  // [kRingWindow]: ext[wb + x]
  uint32_t* s_x = s_lds + kRingWindow;                      // [kRingSlots]: eps x_k + offset of source coefficient c0 + cc
  const int c0 = pl.sb * kRingSlots, k0 = pl.tile * kRingTile;
  const uint32_t off = rc_offset(basebit, a.l);
  const uint32_t* v = reinterpret_cast<const uint32_t*>(a.in) + ((size_t)pl.r * (size_t)a.stride * 2 + (size_t)spoly) * (size_t)N;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.sel) + (size_t)pl.r * a.sel_stride + rc_sel_offset(N, jr, pl.poly);
  sweep_stage_window(s_win, p, N, ring_window_base(N, k0, c0), kRingWindow, t, kRingThreads);
  const int odd = t & 1;                                    // of every slot cc = t + i kRingThreads, and of k = c0 + cc
  for (int cc = t; cc < kRingSlots; cc += kRingThreads) s_x[cc] = rc_stage_alt(ro_rotated_word(v, N, e, c0 + cc) - v[c0 + cc], off, odd);
  __syncthreads();
  uint32_t acc[kSweepKpt] = {0u, 0u, 0u, 0u};
  ring_sweep_parity(s_win, s_x, kRingSlots, t, [=](uint32_t xbar, auto slot_odd) { return rc_digit_alt(xbar, basebit, j, decltype(slot_odd)::value); }, acc);
  unsigned int* out = reinterpret_cast<unsigned int*>(a.out) + ((size_t)pl.r * 2 + (size_t)pl.poly) * (size_t)N + k0 + kSweepKpt * t;
#pragma unroll
  for (int q = 0; q < kSweepKpt; ++q) atomicAdd(out + q, acc[q]);
}

// one workgroup per output row: sample r width + c is coefficient c of ciphertext r (rl_extract_word, the formula of
// rlwe_extract_kernel with the slot index replaced)
__global__ __launch_bounds__(kRoHeadThreads) void ring_heads_kernel(RingHeadsArgs x) {
  const int N = x.N;
  const long i = (long)blockIdx.x;
  const long r = i / x.width;
  const int c = (int)(i - r * x.width);
  const uint32_t* a = reinterpret_cast<const uint32_t*>(x.rlwe) + (size_t)r * 2 * (size_t)N;
  uint32_t* u = reinterpret_cast<uint32_t*>(x.u) + (size_t)i * ((size_t)N + 1);
  for (int j = threadIdx.x; j <= N; j += kRoHeadThreads) u[j] = rl_extract_word(a, a + N, N, c, j);
}

// one level: out = in, then the sweep of a.form unless the exponent is zero (x = 0, and every digit of 0 is 0 in both forms)
hipError_t launch_ring_rotate_level(const RingRotateArgs& a, hipStream_t st) {
  if (a.R <= 0) return hipSuccess;
  const long init_groups = a.R * (2 * (long)a.N / kRoInitThreads);
  hipLaunchKernelGGL(ring_rotate_init_kernel, dim3((unsigned)init_groups), dim3(kRoInitThreads), 0, st, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || a.e == 0) return err;
  const size_t lds = ((size_t)2 * kRcSlots + kRcTile) * sizeof(uint32_t);
  const dim3 grid((unsigned)rc_groups(a.R, a.N, a.l));
  if (a.form == kRcAlternating)
    hipLaunchKernelGGL(ring_rotate_alt_kernel, grid, dim3(kRcThreads), lds, st, a);
  else
    hipLaunchKernelGGL(ring_rotate_kernel, grid, dim3(kRcThreads), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_ring_heads(const RingHeadsArgs& x, hipStream_t st) {
  if (x.R <= 0) return hipSuccess;
  hipLaunchKernelGGL(ring_heads_kernel, dim3((unsigned)(x.R * x.width)), dim3(kRoHeadThreads), 0, st, x);
  return hipGetLastError();
}

}  // namespace rs
