// rs_ring_rekey.hip -- ring re-keying (rs_ring_rekey_dev; include/redsec_hip.h):
//   ring_rekey_init_kernel   out[r] = (-K[t].a, b_r - K[t].b)
//   ring_rekey_kernel        out[r] -= D_j(X) K[j] over one block of source coefficients,  D_j(X) = sum_k d_j(k) X^k
// An object of its own, so that every earlier kernel keeps its instructions. Integer only: an odd digit of basebit + 1 bits times a
// 32-bit word, accumulated mod 2^32, exact in any order, so neither the tiling nor the number of blocks can change a word.
//
// ring_rekey_kernel has pack_kernel's shape (rs_pack.hip) with the digit source replaced by the input's own a polynomial. A workgroup
// of kRrThreads threads owns kRrTile consecutive coefficients of one polynomial of one output ciphertext, one block of kRrSlots =
// 1,024 source coefficients c0 .. c0 + 1023 and one digit j (rs_ring_rekey.h): the grid is 2 (N / 512) (N / 1024) t workgroups per
// ciphertext, 4 t at N = 1024 and 256 t at N = 8192, so that one ciphertext of the large ring alone fills the device. It stages the
// window of ext = (-p, p) of its key row that its coefficients and source block read (1,024 + 512 words) and the block's words
// a_k + offset (1,024 words) once; thread t keeps coefficients k0 + 4t .. k0 + 4t + 3 in registers, and ONE 16-byte LDS read per thread
// serves the 16 multiply-adds of four source coefficients. The word a_k + offset is the same in every lane: it is made a scalar
// (readfirstlane), the digit is cut out by scalar shift and mask and centred (2 u - (B - 1)) on the scalar unit, and the multiply is
// v_mul_lo_u32 with the scalar digit as one operand. The partial sums of the source blocks and digits meet by vector atomicAdd
// (global_atomic_add_u32, no return) on the words ring_rekey_init_kernel has set on the same stream just before; every call
// initialises again, so a second call into the same buffer gives the same words.
// rs_emu_ring_rekey (rs_emulate.cpp) walks the same workgroup / four-slot loop on the CPU as a second copy, not as shared code: a
// change to the loop below has to be made there too, or tests/test_ring_rekey_cpu.py stops pinning this kernel.
// Multiply-add form (disassembly of this object): per four source coefficients and lane 16 v_mul_lo_u32 with the scalar digit as one
// operand and 8 v_add3_u32, as in pack_kernel; no v_mad_u64_u32.
// Resources (-Rpass-analysis=kernel-resource-usage): ring_rekey_kernel 29 VGPRs, 28 SGPRs, 10.0 KB of dynamic LDS, no scratch, no
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
  const int N = a.N, tiles = rr_tiles(N), blocks = rr_blocks(N), t = threadIdx.x;
  unsigned g = blockIdx.x;
  const int tile = (int)(g % (unsigned)tiles); g /= (unsigned)tiles;
  const int poly = (int)(g & 1u); g >>= 1;
  const int sb = (int)(g % (unsigned)blocks); g /= (unsigned)blocks;
  const int j = (int)(g % (unsigned)a.t);
  const long r = (long)(g / (unsigned)a.t);
  uint32_t* s_win = s_lds;                                  // [kRrSlots + kRrTile]: ext[wb + x]
  uint32_t* s_a = s_lds + kRrSlots + kRrTile;               // [kRrSlots]: a_k + offset of source coefficient c0 + cc
  const int c0 = sb * kRrSlots, k0 = tile * kRrTile, wb = rr_window_base(N, k0, c0);
  const uint32_t off = rr_offset(a.basebit, a.t), mask = (1u << a.basebit) - 1u;
  const int shift = 32 - (j + 1) * a.basebit;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.rlwe) + (size_t)r * 2 * (size_t)N + (size_t)c0;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.key) + rr_key_offset(N, j, poly);
  for (int x = t; x < kRrSlots + kRrTile; x += kRrThreads) s_win[x] = rl_ext_word(p, N, wb + x);
  for (int cc = t; cc < kRrSlots; cc += kRrThreads) s_a[cc] = src[cc] + off;
  __syncthreads();
  const uint4* win4 = reinterpret_cast<const uint4*>(s_win);
  const uint4* a4 = reinterpret_cast<const uint4*>(s_a);
  uint32_t acc[kRrKpt] = {0u, 0u, 0u, 0u};
  int c4 = t + kRrSlots / 4;                                // chunk of window words 4t + kRrSlots - cc .. + 3, cc = 0
  uint4 hi = win4[c4];
  for (int q4 = 0; q4 < kRrSlots / 4; ++q4) {               // source coefficients cc = 4 q4 .. 4 q4 + 3
    const uint4 av = a4[q4];                                // the same four words in every lane: scalars
    const uint32_t d[4] = {2u * (((uint32_t)__builtin_amdgcn_readfirstlane((int)av.x) >> shift) & mask) - mask,
                           2u * (((uint32_t)__builtin_amdgcn_readfirstlane((int)av.y) >> shift) & mask) - mask,
                           2u * (((uint32_t)__builtin_amdgcn_readfirstlane((int)av.z) >> shift) & mask) - mask,
                           2u * (((uint32_t)__builtin_amdgcn_readfirstlane((int)av.w) >> shift) & mask) - mask};
    const uint4 lo = win4[--c4];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int b = 0; b < 4; ++b) {                           // cc = 4 q4 + b: coefficient 4t + q takes window word 4 c4' + q - b
#pragma unroll
      for (int q = 0; q < kRrKpt; ++q) acc[q] += w[4 + q - b] * d[b];
    }
    hi = lo;
  }
  unsigned int* out = reinterpret_cast<unsigned int*>(a.out) + ((size_t)r * 2 + (size_t)poly) * (size_t)N + k0 + kRrKpt * t;
#pragma unroll
  for (int q = 0; q < kRrKpt; ++q) atomicAdd(out + q, 0u - acc[q]);
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
