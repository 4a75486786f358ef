// rs_ring_cmux.hip -- encrypted selection on packed ciphertexts (rs_ring_cmux_dev, rs_ring_lookup_dev; include/redsec_hip.h):
//   ring_cmux_init_kernel   out[r] = d0[r stride]
//   ring_cmux_kernel        out[r] += D_jr(X) sel[jr] over one block of source coefficients,  D_jr(X) = sum_k dig_j(x_k) X^k,
//                           x = d1[r stride] - d0[r stride], polynomial jr / l of it, digit j = jr mod l
// An object of its own, so that every earlier kernel keeps its instructions. Integer only: a signed digit of basebit bits times a
// 32-bit word, accumulated mod 2^32, exact in any order, so neither the tiling nor the number of blocks can change a word.
//
// ring_cmux_kernel has ring_rekey_kernel's shape (rs_ring_rekey.hip) with the digit source replaced by the difference of two
// ciphertexts and 2l selector rows in place of t key rows. A workgroup of kRcThreads threads owns kRcTile consecutive coefficients
// of one polynomial of one output ciphertext, one block of kRcSlots = 1,024 source coefficients and one selector row jr
// (rs_ring_cmux.h): the grid is 2 (N / 512) (N / 1024) 2l workgroups per ciphertext, 8 l at N = 1024 and 512 l at N = 8192. It
// stages the window of ext = (-p, p) of its selector row that its coefficients and source block read (1,024 + 512 words) and the
// block's words d1 - d0 + off (1,024 words; -d0 + off under a null d1, the same choice in every workgroup of a launch) once;
// thread t keeps coefficients k0 + 4t .. k0 + 4t + 3 in registers, and ONE 16-byte LDS read per thread serves the 16 multiply-adds
// of four source coefficients. The staged word is the same in every lane: it is made a scalar (readfirstlane), the digit is cut out
// by scalar shift and mask and B/2 taken off on the scalar unit, and the multiply is v_mul_lo_u32 with the scalar digit as one
// operand. The partial sums of the source blocks and rows meet by vector atomicAdd (global_atomic_add_u32, no return) on the words
// ring_cmux_init_kernel has set on the same stream just before; every call initialises again, so a second call into the same
// buffer gives the same words.
// rs_emu_ring_cmux (rs_emulate.cpp) walks the same workgroup / four-slot loop on the CPU as a second copy, not as shared code: a
// change to the loop below has to be made there too, or tests/test_ring_cmux_cpu.py stops pinning this kernel.
// Multiply-add form (disassembly of this object): per four source coefficients and lane 16 v_mul_lo_u32 with the scalar digit as one
// operand and 8 v_add3_u32, as in ring_rekey_kernel; no v_mad_u64_u32.
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
  const int N = a.N, tiles = rc_tiles(N), blocks = rc_blocks(N), t = threadIdx.x;
  unsigned g = blockIdx.x;
  const int tile = (int)(g % (unsigned)tiles); g /= (unsigned)tiles;
  const int poly = (int)(g & 1u); g >>= 1;
  const int sb = (int)(g % (unsigned)blocks); g /= (unsigned)blocks;
  const int jr = (int)(g % (unsigned)(2 * a.l));
  const long r = (long)(g / (unsigned)(2 * a.l));
  const int j = jr < a.l ? jr : jr - a.l, spoly = jr < a.l ? 0 : 1;
  uint32_t* s_win = s_lds;                                  // [kRcSlots + kRcTile]: ext[wb + x]
  uint32_t* s_x = s_lds + kRcSlots + kRcTile;               // [kRcSlots]: x_k + offset of source coefficient c0 + cc
  const int c0 = sb * kRcSlots, k0 = tile * kRcTile, wb = rc_window_base(N, k0, c0);
  const uint32_t off = rc_offset(a.basebit, a.l), mask = (1u << a.basebit) - 1u, bias = 1u << (a.basebit - 1);
  const int shift = 32 - (j + 1) * a.basebit;
  const size_t src_at = ((size_t)r * (size_t)a.stride * 2 + (size_t)spoly) * (size_t)N + (size_t)c0;
  const uint32_t* s0 = reinterpret_cast<const uint32_t*>(a.d0) + src_at;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.sel) + rc_sel_offset(N, jr, poly);
  for (int x = t; x < kRcSlots + kRcTile; x += kRcThreads) s_win[x] = rl_ext_word(p, N, wb + x);
  if (a.d1) {
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(a.d1) + src_at;
    for (int cc = t; cc < kRcSlots; cc += kRcThreads) s_x[cc] = s1[cc] - s0[cc] + off;
  } else {
    for (int cc = t; cc < kRcSlots; cc += kRcThreads) s_x[cc] = off - s0[cc];
  }
  __syncthreads();
  const uint4* win4 = reinterpret_cast<const uint4*>(s_win);
  const uint4* x4 = reinterpret_cast<const uint4*>(s_x);
  uint32_t acc[kRcKpt] = {0u, 0u, 0u, 0u};
  int c4 = t + kRcSlots / 4;                                // chunk of window words 4t + kRcSlots - cc .. + 3, cc = 0
  uint4 hi = win4[c4];
  for (int q4 = 0; q4 < kRcSlots / 4; ++q4) {               // source coefficients cc = 4 q4 .. 4 q4 + 3
    const uint4 xv = x4[q4];                                // the same four words in every lane: scalars
    const uint32_t d[4] = {(((uint32_t)__builtin_amdgcn_readfirstlane((int)xv.x) >> shift) & mask) - bias,
                           (((uint32_t)__builtin_amdgcn_readfirstlane((int)xv.y) >> shift) & mask) - bias,
                           (((uint32_t)__builtin_amdgcn_readfirstlane((int)xv.z) >> shift) & mask) - bias,
                           (((uint32_t)__builtin_amdgcn_readfirstlane((int)xv.w) >> shift) & mask) - bias};
    const uint4 lo = win4[--c4];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int b = 0; b < 4; ++b) {                           // cc = 4 q4 + b: coefficient 4t + q takes window word 4 c4' + q - b
#pragma unroll
      for (int q = 0; q < kRcKpt; ++q) acc[q] += w[4 + q - b] * d[b];
    }
    hi = lo;
  }
  unsigned int* out = reinterpret_cast<unsigned int*>(a.out) + ((size_t)r * 2 + (size_t)poly) * (size_t)N + k0 + kRcKpt * t;
#pragma unroll
  for (int q = 0; q < kRcKpt; ++q) atomicAdd(out + q, acc[q]);
}

hipError_t launch_ring_cmux(const RingCmuxArgs& a, hipStream_t st) {
  if (a.R <= 0) return hipSuccess;
  const long init_groups = a.R * (2 * (long)a.N / kRcInitThreads);
  hipLaunchKernelGGL(ring_cmux_init_kernel, dim3((unsigned)init_groups), dim3(kRcInitThreads), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t lds = ((size_t)2 * kRcSlots + kRcTile) * sizeof(uint32_t);
  hipLaunchKernelGGL(ring_cmux_kernel, dim3((unsigned)rc_groups(a.R, a.N, a.l)), dim3(kRcThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace rs
