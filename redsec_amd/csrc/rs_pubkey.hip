// rs_pubkey.hip -- public-key encryption (rs_pk_encrypt_dev; include/redsec_hip.h):
//   pk_encrypt_kernel   ct[i] = base[i] + (0, mu[i]) + sum over the set selection bits j of ciphertext i of pk[j]   (mod 2^32)
// An object of its own, so that every earlier kernel keeps its instructions.
//
// A 0/1 matrix [B][m] times the row matrix [m][n + 1] in plain 32-bit integer adds: sums mod 2^32 are exact in any order, so the
// tiling cannot change a word. Lane = word of the row; a workgroup owns kPkTile ciphertexts x kPkThreads words with one accumulator
// per ciphertext in registers. The rows go in chunks of kPkChunk: one ChaCha block per ciphertext and chunk (kg_pk_select_block, the
// function the lane emulator runs) gives the chunk's selection bits, which live in LDS for the length of the chunk and in SGPRs while
// they are used -- they are the encryptor's secret randomness and are never written to global memory. The chunk's rows then stream
// past as coalesced dword loads, 32 rows at a time in registers, each of them offered to every ciphertext of the tile. A ciphertext's
// bit is the same for all lanes, so the add is masked by a scalar (x & -bit): no divergent branch. n + 1 is odd, so the last word
// tile of a row is ragged: its lanes past word n neither load nor store.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_keygen.h"
#include "rs_kernels.h"

namespace rs {

namespace {

// rows j .. j + ROWS - 1 of the key (word column `col`, row stride W), offered to every ciphertext of the tile; word g of the chunk's
// selection words holds their bits from bit 0 up. Rows at or past `rows` (a ragged last group) read as zero.
template <bool FULL>
__device__ __forceinline__ void pk_add_group(uint32_t (&acc)[kPkTile], const uint32_t* col, size_t W, int rows,
                                             const uint32_t (*sel)[kPkChunk / 32], int g) {
  uint32_t x[32];
#pragma unroll
  for (int r = 0; r < 32; ++r) x[r] = (FULL || r < rows) ? col[(size_t)r * W] : 0u;
#pragma unroll
  for (int c = 0; c < kPkTile; ++c) {
    const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)sel[c][g]);   // the same word in every lane: a scalar
#pragma unroll
    for (int r = 0; r < 32; ++r) acc[c] += x[r] & (uint32_t)((int32_t)(s << (31 - r)) >> 31);
  }
}

}  // namespace

__global__ __launch_bounds__(kPkThreads) void pk_encrypt_kernel(PkArgs a) {
  __shared__ uint32_t s_sel[kPkTile][kPkChunk / 32];
  const int t = threadIdx.x;
  const size_t W = (size_t)a.n + 1, w = (size_t)blockIdx.y * kPkThreads + t;
  const bool live = w < W;                                    // false in the ragged tail of the last word tile
  const long i0 = (long)blockIdx.x * kPkTile;
  const int cnt = (int)std::min<long>(kPkTile, a.B - i0);     // ciphertexts of this tile
  uint32_t key[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) key[k] = a.seed[k];
  uint32_t acc[kPkTile];
#pragma unroll
  for (int c = 0; c < kPkTile; ++c) acc[c] = 0u;
  const uint32_t* pk = reinterpret_cast<const uint32_t*>(a.pk);
  for (long j0 = 0; j0 < a.m; j0 += kPkChunk) {
    __syncthreads();   // the previous chunk's bits have been used
    if (t < kPkTile) {
      uint32_t sel[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) sel[q] = 0u;               // a tile past B selects nothing
      if (t < cnt) kg_pk_select_block(key, a.first + (uint64_t)(i0 + t), (uint32_t)(j0 / kPkChunk), sel);
#pragma unroll
      for (int q = 0; q < 16; ++q) s_sel[t][q] = sel[q];
    }
    __syncthreads();
    if (live) {
      const int rows = (int)std::min<long>(kPkChunk, a.m - j0);
      const uint32_t* col = pk + (size_t)j0 * W + w;
      int g = 0;
      for (; 32 * (g + 1) <= rows; ++g) pk_add_group<true>(acc, col + (size_t)(32 * g) * W, W, 32, s_sel, g);
      if (32 * g < rows) pk_add_group<false>(acc, col + (size_t)(32 * g) * W, W, rows - 32 * g, s_sel, g);
    }
  }
  if (!live) return;
  // base and mu enter once, here; ct may be base (every word is read, then written, by the same lane)
#pragma unroll
  for (int c = 0; c < kPkTile; ++c) {
    if (c >= cnt) break;
    const size_t e = (size_t)(i0 + c) * W + w;
    uint32_t v = acc[c];
    if (a.base) v += (uint32_t)a.base[e];
    if (a.mu && w == W - 1) v += (uint32_t)a.mu[i0 + c];
    a.ct[e] = (int32_t)v;
  }
}

hipError_t launch_pk_encrypt(const PkArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const dim3 grid((unsigned)((a.B + kPkTile - 1) / kPkTile), (unsigned)((a.n + 1 + kPkThreads - 1) / kPkThreads)), block(kPkThreads);
  hipLaunchKernelGGL(pk_encrypt_kernel, grid, block, 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
