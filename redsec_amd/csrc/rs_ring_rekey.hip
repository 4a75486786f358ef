// rs_ring_rekey.hip -- ring re-keying (rs_ring_rekey_dev; include/redsec_hip.h):
//   ring_rekey_init_kernel   out[r] = (-K[t].a, b_r - K[t].b)
//   ring_rekey_kernel        out[r] -= D_j(X) K[j] over one block of source coefficients,  D_j(X) = sum_k d_j(k) X^k
// An object of its own, so that every earlier kernel keeps its instructions. Integer only: an odd digit of basebit + 1 bits times a
// 32-bit word, accumulated mod 2^32, exact in any order, so neither the tiling nor the number of blocks can change a word.
//
// ring_rekey_kernel is the ring placement and ring_sweep of rs_ring_sweep.h (the LDS read pattern, the scalar digit and the
// multiply-add form are described there) with one workgroup per (tile, polynomial, source block, digit j, ciphertext): the grid is
// 2 (N / 512) (N / 1024) t workgroups per ciphertext, 4 t at N = 1024 and 256 t at N = 8192, so that one ciphertext of the large
// ring alone fills the device. What is this kernel's own: the staged source words are the input's a polynomial, a_k + offset
// (1,024 words, beside the 1,024 + 512 of the window of key row j); the digit is rr_digit, odd and centred (2 u - (B - 1)); and the
// partial sums are NEGATED into the output. They meet by vector atomicAdd (global_atomic_add_u32, no return) on the words
// ring_rekey_init_kernel has set on the same stream just before; every call initialises again, so a second call into the same
// buffer gives the same words. rs_emu_ring_rekey (rs_emulate.cpp) walks the same workgroups on the CPU through the same ring_place
// and ring_sweep.
// Resources (-Rpass-analysis=kernel-resource-usage): ring_rekey_kernel 28 VGPRs, 28 SGPRs, 10.0 KB of dynamic LDS, no scratch, no
// static LDS, eight waves per SIMD; ring_rekey_init_kernel 6 VGPRs, 16 SGPRs, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_ring_rekey.h"

namespace rs {

__global__ __launch_bounds__(kRrInitThreads) void ring_rekey_init_kernel(RingRekeyArgs a, long words) {
  const long idx = (long)blockIdx.x * kRrInitThreads + threadIdx.x;
  if (idx >= words) return;
  const int N = a.N;
  const int w = (int)(idx & (2 * (long)N - 1));             // word of the ciphertext: polynomial w / N, coefficient w mod N
  const uint32_t kw = (uint32_t)a.key[rr_key_offset(N, a.t, 0) + (size_t)w];
  a.out[idx] = (int32_t)((w >= N ? (uint32_t)a.rlwe[idx] : 0u) - kw);
}

__global__ __launch_bounds__(kRrThreads) void ring_rekey_kernel(RingRekeyArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, t = threadIdx.x, basebit = a.basebit;
  const RingPlace pl = ring_place(blockIdx.x, N, a.t);
  const int j = pl.row;
  uint32_t* s_win = s_lds;                                  // [kRingWindow]: ext[wb + x]
  uint32_t* s_a = s_lds + kRingWindow;                      // [kRingSlots]: a_k + offset of source coefficient c0 + cc
  const int c0 = pl.sb * kRingSlots, k0 = pl.tile * kRingTile;
  const uint32_t off = rr_offset(basebit, a.t);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.rlwe) + (size_t)pl.r * 2 * (size_t)N + (size_t)c0;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.key) + rr_key_offset(N, j, pl.poly);
  sweep_stage_window(s_win, p, N, ring_window_base(N, k0, c0), kRingWindow, t, kRingThreads);
  for (int cc = t; cc < kRingSlots; cc += kRingThreads) s_a[cc] = src[cc] + off;
  __syncthreads();
  uint32_t acc[kSweepKpt] = {0u, 0u, 0u, 0u};
  ring_sweep(s_win, s_a, kRingSlots, t, [=](uint32_t abar) { return rr_digit(abar, basebit, j); }, acc);
  unsigned int* out = reinterpret_cast<unsigned int*>(a.out) + ((size_t)pl.r * 2 + (size_t)pl.poly) * (size_t)N + k0 + kSweepKpt * t;
#pragma unroll
  for (int q = 0; q < kSweepKpt; ++q) atomicAdd(out + q, 0u - acc[q]);
}

hipError_t launch_ring_rekey(const RingRekeyArgs& a, hipStream_t st) {
  if (a.R <= 0) return hipSuccess;
  const long words = a.R * 2 * (long)a.N;
  hipLaunchKernelGGL(ring_rekey_init_kernel, dim3((unsigned)((words + kRrInitThreads - 1) / kRrInitThreads)), dim3(kRrInitThreads), 0, st, a, words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t lds = ((size_t)2 * kRrSlots + kRrTile) * sizeof(uint32_t);
  hipLaunchKernelGGL(ring_rekey_kernel, dim3((unsigned)rr_groups(a.R, a.N, a.t)), dim3(kRrThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace rs
