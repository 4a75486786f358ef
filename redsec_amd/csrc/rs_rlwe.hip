// rs_rlwe.hip -- compact RLWE public keys (rs_rlwe_pk_encrypt_dev, rs_rlwe_extract_dev; include/redsec_hip.h):
//   rlwe_pk_encrypt_kernel   rlwe[r] = (a*u_r + e1, b*u_r + e2 + m_r) for the public key (a, b) and a secret binary u_r   (mod 2^32)
//   rlwe_extract_kernel      u[rN + c] = the LWE sample of coefficient c of rlwe[r]
// An object of its own, so that every earlier kernel keeps its instructions.
//
// Encryption is the negacyclic product of a key polynomial p with a binary polynomial u in plain 32-bit integer adds: out[k] = sum
// over the set bits j of u of coefficient k of X^j p. Sums mod 2^32 are exact in any order, so the tiling cannot change a word. A
// workgroup of kRlThreads threads owns kRlTile consecutive output coefficients k0 .. k0 + kRlTile - 1 of one polynomial of one
// ciphertext (grid: ciphertext x polynomial x tile, so N = 8192 spreads over 32 workgroups per ciphertext). The key polynomial is
// staged once in LDS as the window ext[k0 .. k0 + N + kRlTile) of ext = (-p, p) (rs_rlwe.h): coefficient k of X^j p is ext[k - j + N]
// with the wrapped part already negated, and a tile only ever reads that window. Thread t holds coefficients k0 + 4t .. k0 + 4t + 3
// in registers across the whole sweep of j; four consecutive j need the seven words ext[k - j0 - 3 + N .. k + 3 + N], two aligned
// 16-byte chunks of which the upper one is the lower one of the previous four j: ONE 16-byte LDS read per thread serves 16 adds (the
// compiler emits it as ds_read2_b64, not ds_read_b128), and consecutive threads read consecutive chunks (no bank conflict). The selector bits come from the domain-12 ChaCha blocks
// (rl_select_block, the function the lane emulator runs) and live in LDS; bit j is the same in every lane, so its word is made a
// scalar and the add is masked (x & -bit): no divergent branch. u is the encryptor's secret: it exists only in registers and LDS and
// is never written to global memory. e1 / e2 (domain 13) and the message enter once, at the store.
// rs_emu_rlwe_pk_encrypt / rs_emu_rlwe_extract (rs_emulate.cpp) walk the same chunk-and-carry loop on the CPU as a second copy, not as
// shared code: a change to the loop below has to be made there too, or tests/test_rlwe_pubkey_cpu.py stops pinning this kernel.
// Resources (-Rpass-analysis=kernel-resource-usage): rlwe_pk_encrypt_kernel 92 VGPRs, 66 SGPRs, (N + 512 + N / 32) 4 bytes of
// dynamic LDS (6.1 KB at N = 1024, 35.8 KB at N = 8192), no scratch, five waves per SIMD; rlwe_extract_kernel 8 VGPRs, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_rlwe.h"

namespace rs {

__global__ __launch_bounds__(kRlThreads) void rlwe_pk_encrypt_kernel(RlweEncArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, tiles = N / kRlTile, t = threadIdx.x;
  uint32_t* s_win = s_lds;                      // [N + kRlTile]: ext[k0 + i]
  uint32_t* s_sel = s_lds + N + kRlTile;        // [N / 32]: the selector, 32 bits per word
  const int tile = (int)(blockIdx.x % (unsigned)tiles), poly = (int)((blockIdx.x / (unsigned)tiles) & 1u);
  const long r = (long)(blockIdx.x / (unsigned)(2 * tiles));
  const uint64_t row = a.first + (uint64_t)r;
  const int k0 = tile * kRlTile;
  uint32_t key[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) key[q] = a.seed[q];
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.pk) + (size_t)poly * N;
  for (int i = t; i < N + kRlTile; i += kRlThreads) s_win[i] = rl_ext_word(p, N, k0 + i);
  if (t < N / 512) {
    uint32_t w[16];
    rl_select_block(key, row, (uint32_t)t, w);
#pragma unroll
    for (int q = 0; q < 16; ++q) s_sel[16 * t + q] = w[q];
  }
  __syncthreads();
  uint32_t acc[kRlKpt] = {0u, 0u, 0u, 0u};
  const uint4* win4 = reinterpret_cast<const uint4*>(s_win);
  int c4 = t + N / 4;                           // chunk of window words 4t + N - j0 .. + 3, j0 = 0
  uint4 hi = win4[c4];
  for (int wd = 0; wd < N / 32; ++wd) {
    const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_sel[wd]);   // the same word in every lane: a scalar
#pragma unroll
    for (int g = 0; g < 8; ++g) {               // j0 = 32 wd + 4 g
      const uint4 lo = win4[--c4];
      const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int b = 0; b < 4; ++b) {             // j = j0 + b: coefficient k + q takes window word 4 c4' + q - b, c4' the chunk of hi
        const uint32_t m = (uint32_t)((int32_t)(s << (31 - (4 * g + b))) >> 31);
#pragma unroll
        for (int q = 0; q < kRlKpt; ++q) acc[q] += w[4 + q - b] & m;
      }
      hi = lo;
    }
  }
  const int k = k0 + kRlKpt * t;
  int32_t e[4];
  rl_noise4(key, row, poly, N, k, a.sigma, e);
  int32_t* out = a.rlwe + ((size_t)r * 2 + (size_t)poly) * (size_t)N + k;
#pragma unroll
  for (int q = 0; q < kRlKpt; ++q) {
    uint32_t v = acc[q] + (uint32_t)e[q];
    const long i = r * (long)N + k + q;         // the message of this slot; slots at or past count carry 0
    if (poly == 1 && i < a.count) v += (uint32_t)a.mu[i];
    out[q] = (int32_t)v;
  }
}

// one workgroup per output row i = rN + c: N + 1 coalesced dword stores (the row stride N + 1 is odd)
__global__ __launch_bounds__(kRlExThreads) void rlwe_extract_kernel(RlweExtractArgs x) {
  const int N = x.N;
  const long i = (long)blockIdx.x;
  const long r = i / N;
  const int c = (int)(i - r * N);
  const uint32_t* a = reinterpret_cast<const uint32_t*>(x.rlwe) + (size_t)r * 2 * (size_t)N;
  uint32_t* u = reinterpret_cast<uint32_t*>(x.u) + (size_t)i * ((size_t)N + 1);
  for (int j = threadIdx.x; j <= N; j += kRlExThreads) u[j] = rl_extract_word(a, a + N, N, c, j);
}

hipError_t launch_rlwe_pk_encrypt(const RlweEncArgs& a, hipStream_t st) {
  if (a.count <= 0) return hipSuccess;
  const long R = (a.count + a.N - 1) / a.N;
  const dim3 grid((unsigned)(R * 2 * (a.N / kRlTile))), block(kRlThreads);
  const size_t lds = ((size_t)a.N + kRlTile + (size_t)a.N / 32) * sizeof(uint32_t);
  hipLaunchKernelGGL(rlwe_pk_encrypt_kernel, grid, block, lds, st, a);
  return hipGetLastError();
}

hipError_t launch_rlwe_extract(const RlweExtractArgs& x, hipStream_t st) {
  if (x.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(rlwe_extract_kernel, dim3((unsigned)x.count), dim3(kRlExThreads), 0, st, x);
  return hipGetLastError();
}

}  // namespace rs
