// rs_packkey.hip -- the packing key on the device (rs_pack_keygen_dev, rs_pack_expand_dev; include/redsec_hip.h):
//   pack_keygen_kernel   body[i t + j] = a*S + e + s_i g_j X^0 for the domain-14 mask a of the row and the binary ring secret S   (mod 2^32)
//   pack_expand_kernel   key[i t + j] = (a, body[i t + j]): the masks regenerated from the public seed, the bodies copied beside them
// An object of its own, so that every earlier kernel keeps its instructions.
//
// The generator is the product of rlwe_pk_encrypt_kernel (rs_rlwe.hip) with the roles turned round: there the key polynomial is
// public and the binary selector secret, here the mask a is public and the binary S is the secret. out[k] = sum over the set bits m
// of S of coefficient k of X^m a, in plain 32-bit integer adds, exact in any order. A workgroup of kPgThreads threads owns kPgTile
// consecutive coefficients k0 .. k0 + kPgTile - 1 of one row (grid: row x tile) for the whole sweep of m, so there are no atomics.
// The window ext[k0 .. k0 + N + kPgTile) of ext = (-a, a) is filled in LDS straight from the row's ChaCha blocks (pg_window_block):
// the mask never reaches global memory. S is staged once per workgroup as N / 32 words from the caller's private packed copy; bit m
// is the same in every lane, so its word is made a scalar and the add is masked (x & -bit): no divergent branch, and the time of a
// row does not depend on S. Thread t holds coefficients k0 + 4t .. k0 + 4t + 3 in registers; four consecutive m need the seven
// words ext[k - m0 - 3 + N .. k + 3 + N], two aligned 16-byte chunks of which the upper one is the lower one of the previous four
// m: ONE 16-byte LDS read per thread serves 16 adds. The noise (domain 15, four Gaussians per thread) and the gadget word s_i g_j
// (coefficient 0, hence tile 0 only) enter once, at the store.
// rs_emu_pack_keygen_row / rs_emu_pack_expand_row (rs_emulate.cpp) walk the same loops on the CPU as a second copy, not as shared
// code: a change to a loop below has to be made there too, or tests/test_pack_key_cpu.py stops pinning these kernels.
// Dynamic LDS of pack_keygen_kernel: (N + 512 + N / 32) 4 bytes (6.1 KB at N = 1024, 35.8 KB at N = 8192); no static LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_packkey.h"

namespace rs {

__global__ __launch_bounds__(kPgThreads) void pack_keygen_kernel(PackKeygenArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, tiles = N / kPgTile, t = threadIdx.x;
  uint32_t* s_win = s_lds;                      // [N + kPgTile]: ext[k0 + i]
  uint32_t* s_S = s_lds + N + kPgTile;          // [N / 32]: the ring secret, 32 bits per word
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const uint64_t row = (uint64_t)(blockIdx.x / (unsigned)tiles);
  const int k0 = tile * kPgTile;
  uint32_t key[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) key[q] = a.seed[q];
  uint4* win_out = reinterpret_cast<uint4*>(s_win);
  for (int wb = t; wb < pg_window_blocks(N); wb += kPgThreads) {
    uint32_t w[16];
    pg_window_block(key, row, N, k0, wb, w);
#pragma unroll
    for (int q = 0; q < 4; ++q) win_out[4 * wb + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
  for (int i = t; i < N / 32; i += kPgThreads) s_S[i] = a.tlwe_bits[i];
  __syncthreads();
  uint32_t acc[kPgKpt] = {0u, 0u, 0u, 0u};
  const uint4* win4 = reinterpret_cast<const uint4*>(s_win);
  int c4 = t + N / 4;                           // chunk of window words 4t + N - m0 .. + 3, m0 = 0
  uint4 hi = win4[c4];
  for (int wd = 0; wd < N / 32; ++wd) {
    const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_S[wd]);   // the same word in every lane: a scalar
#pragma unroll
    for (int g = 0; g < 8; ++g) {               // m0 = 32 wd + 4 g
      const uint4 lo = win4[--c4];
      const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int b = 0; b < 4; ++b) {             // m = m0 + b: coefficient k + q takes window word 4 c4' + q - b, c4' the chunk of hi
        const uint32_t m = (uint32_t)((int32_t)(s << (31 - (4 * g + b))) >> 31);
#pragma unroll
        for (int q = 0; q < kPgKpt; ++q) acc[q] += w[4 + q - b] & m;
      }
      hi = lo;
    }
  }
  const int k = k0 + kPgKpt * t;
  uint32_t nkey[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) nkey[q] = a.noise_seed[q];
  int32_t e[4];
  pg_noise4(nkey, row, k, a.sigma, e);
  uint32_t v[kPgKpt];
#pragma unroll
  for (int q = 0; q < kPgKpt; ++q) v[q] = acc[q] + (uint32_t)e[q];
  if (k == 0) {                                 // thread 0 of tile 0: the gadget word at X^0
    int i, j;
    pg_row(row, a.t, i, j);
    v[0] += pg_key_bit(a.lwe_bits, i) * pg_gadget(j, a.basebit);
  }
  int32_t* out = a.body + pg_body_offset(N, row) + k;
#pragma unroll
  for (int q = 0; q < kPgKpt; ++q) out[q] = (int32_t)v[q];
}

// flat grid over (row, mask block): 16 mask words and 16 body words per thread
__global__ __launch_bounds__(kPgExThreads) void pack_expand_kernel(PackExpandArgs a) {
  const int N = a.N, T = N / 16;
  const long item = (long)blockIdx.x * kPgExThreads + threadIdx.x;
  if (item >= pg_expand_items(a.rows, N)) return;
  const long row = item / T;
  const int blk = (int)(item - row * T);
  uint32_t key[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) key[q] = a.seed[q];
  uint32_t w[16];
  pg_mask_block(key, (uint64_t)row, blk, w);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.key) + (size_t)row * 2 * (size_t)N;
  if (((uintptr_t)a.key & 15u) == 0) {          // uniform over the grid: 16-byte vector stores where the caller's buffer allows them
    uint4* d4 = reinterpret_cast<uint4*>(dst + 16 * blk);
#pragma unroll
    for (int q = 0; q < 4; ++q) d4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) dst[16 * blk + q] = w[q];
  }
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.body) + pg_body_offset(N, (uint64_t)row);
#pragma unroll
  for (int r = 0; r < 16; ++r) dst[N + blk + T * r] = src[blk + T * r];
}

hipError_t launch_pack_keygen(const PackKeygenArgs& a, hipStream_t st) {
  const long rows = (long)a.n * a.t;
  if (rows <= 0) return hipSuccess;
  if (a.N < kPgMinN || a.N > kPgMaxN || (a.N & (a.N - 1)) != 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(rows * (a.N / kPgTile))), block(kPgThreads);
  const size_t lds = ((size_t)a.N + kPgTile + (size_t)a.N / 32) * sizeof(uint32_t);
  hipLaunchKernelGGL(pack_keygen_kernel, grid, block, lds, st, a);
  return hipGetLastError();
}

hipError_t launch_pack_expand(const PackExpandArgs& a, hipStream_t st) {
  if (a.rows <= 0) return hipSuccess;
  if (a.N < kPgMinN || a.N > kPgMaxN || (a.N & (a.N - 1)) != 0) return hipErrorInvalidValue;
  const long items = pg_expand_items(a.rows, a.N);
  hipLaunchKernelGGL(pack_expand_kernel, dim3((unsigned)((items + kPgExThreads - 1) / kPgExThreads)), dim3(kPgExThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
