// rs_seeded.hip -- seeded LWE ciphertexts (rs_encrypt_seeded_dev, rs_expand_ciphertexts_dev; include/redsec_hip.h):
//   seeded_lwe_kernel<true>    encryption: the domain-7 masks of the mask seed, body = sum_k a_k s_k + e + mu, e of domain 8
//   seeded_lwe_kernel<false>   expansion: the same masks beside the given bodies
// An object of its own, so that the kernels of rs_general.hip keep their instructions.
//
// Both directions regenerate the masks through kg_ct_mask_block and place them through the tile of rs_keygen.h, so the words of
// encryption and expansion cannot drift apart; the lane emulator (rs_emulate.cpp) runs the same functions for the CPU tests.
// A workgroup owns kg_ct_tile(n) whole ciphertexts: its threads walk the flat (ciphertext, block) index, so ChaCha keeps nearly
// every lane busy at n = 350 (22 blocks per mask) as at n = 6144; the words are staged in LDS and the tile leaves as one
// contiguous span of coalesced dword stores, whatever the odd row stride n + 1. The secret key stays in LDS, one bit per word.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_keygen.h"
#include "rs_kernels.h"

namespace rs {

namespace {

// dynamic LDS: [tile] sums, [ceil(n / 32)] key words (encryption), [tile][n + 1] staged words (when ct is written)
size_t seeded_lds_bytes(const SeededArgs& a, bool encrypt) {
  const size_t words = (size_t)a.tile + (encrypt ? (size_t)(a.n + 31) / 32 : 0) + (a.ct ? (size_t)a.tile * (a.n + 1) : 0);
  return words * sizeof(uint32_t);
}

}  // namespace

template <bool ENCRYPT>
__global__ __launch_bounds__(kCtThreads) void seeded_lwe_kernel(SeededArgs a) {
  extern __shared__ uint32_t s_lds[];
  const int t = threadIdx.x, n = a.n, C = a.tile, nblk = kg_ct_blocks(n);
  const int kwords = ENCRYPT ? (n + 31) / 32 : 0;
  uint32_t* s_acc = s_lds;
  uint32_t* s_key = s_lds + C;
  uint32_t* s_ct = s_key + kwords;
  const bool stage = a.ct != nullptr;
  uint32_t key[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) key[k] = a.seed[k];
  if (ENCRYPT)
    for (int i = t; i < kwords; i += kCtThreads) s_key[i] = a.key_bits[i];
  const long tiles = (a.B + C - 1) / C;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i0 = tile * C;
    const int cnt = (int)std::min<long>(C, a.B - i0);
    if (t < cnt) {
      if (ENCRYPT) s_acc[t] = 0u;
      else s_ct[kg_ct_lds_word(t, n, n)] = (uint32_t)a.body[i0 + t];
    }
    __syncthreads();   // sums cleared, key staged; the previous tile's span has left LDS
    const int items = cnt * nblk;
    for (int it = t; it < items; it += kCtThreads) {
      const int c = it / nblk, blk = it - c * nblk;
      uint32_t w[16];
      kg_ct_mask_block(key, a.first + (uint64_t)(i0 + c), blk, w);
      if (stage) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (16 * blk + q < n) s_ct[kg_ct_lds_word(c, 16 * blk + q, n)] = w[q];
      }
      if (ENCRYPT) {
        const uint32_t bits = kg_ct_key_bits(s_key, blk);   // zero past n
        uint32_t acc = 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc += ((bits >> q) & 1u) ? w[q] : 0u;
        atomicAdd(&s_acc[c], acc);   // sums mod 2^32: the order of the adds does not matter
      }
    }
    __syncthreads();
    if (ENCRYPT) {
      if (t < cnt) {
        uint32_t nkey[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) nkey[k] = a.noise_seed[k];
        const uint64_t row = a.first + (uint64_t)(i0 + t);
        const uint32_t b = s_acc[t] + (uint32_t)kg_ct_noise(nkey, row, a.sigma) + (uint32_t)a.mu[i0 + t];
        a.body[i0 + t] = (int32_t)b;
        if (stage) s_ct[kg_ct_lds_word(t, n, n)] = b;
      }
      __syncthreads();
    }
    if (stage) {
      int32_t* dst = a.ct + i0 * (n + 1);
      const int span = cnt * (n + 1);
      for (int j = t; j < span; j += kCtThreads) dst[j] = (int32_t)s_ct[j];
    }
    __syncthreads();
  }
}

static hipError_t launch_seeded(const SeededArgs& a, bool encrypt, int num_cus, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const long tiles = (a.B + a.tile - 1) / a.tile;
  // three workgroups of the largest staging (52 KB) fit a CU's 160 KB of LDS, more with bodies only; the grid strides over tiles
  const dim3 grid((unsigned)std::min<long>(tiles, 4L * num_cus)), block(kCtThreads);
  const size_t lds = seeded_lds_bytes(a, encrypt);
  if (encrypt) hipLaunchKernelGGL(seeded_lwe_kernel<true>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(seeded_lwe_kernel<false>, grid, block, lds, st, a);
  return hipGetLastError();
}

hipError_t launch_encrypt_seeded(const SeededArgs& a, int num_cus, hipStream_t st) { return launch_seeded(a, true, num_cus, st); }
hipError_t launch_expand_ciphertexts(const SeededArgs& a, int num_cus, hipStream_t st) { return launch_seeded(a, false, num_cus, st); }

}  // namespace rs
