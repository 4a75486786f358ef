// rs_rekey.hip -- re-keying (rs_rekey_dev; include/redsec_hip.h): LWE samples keyswitched from one LWE key to another under a
// caller-supplied key, any source dimension to any destination dimension
//   rekey_init_kernel   out[r] = (0, b_r)
//   rekey_kernel        out[r] -= sum over a run of index chunks of d_ij(r) K[i][j],  d_ij(r) = digit j of abar_i of sample r
// An object of its own, so that every earlier kernel keeps its instructions. Integer only: a basebit-bit digit times a 32-bit word,
// accumulated mod 2^32, exact in any order, so neither the tiling nor the number of index splits can change a word.
//
// The shape (rs_rekey.h): a workgroup of four waves owns kRkWords = 64 consecutive output words, lane l the word w0 + l, and
// kRkTile = 128 consecutive ciphertexts, wave v the 32 from r0 + 32 v on: 32 accumulators per thread, in registers over the whole
// run of source indices. Per source index the t key rows are staged once in LDS (t x 64 words, loaded coalesced: one 256-byte
// run per row) and offered to all 128 ciphertexts, so a key word read from global memory serves 128 multiply-adds and one read
// from LDS (ds_read_b32) serves 32. The words of the next index are fetched into registers before the sweep of the present one
// and written to LDS after it, so the load is in flight under the multiplies. The mask words of a chunk of kRkSeg = 8 source
// indices (32 contiguous bytes a sample) are read once per chunk and wave and transposed through LDS into s_a[ii][c] = a_i + offset,
// zero for the ciphertexts past B. The digit of a ciphertext is the same in every lane: the 32 words of one source index are
// read as eight 16-byte broadcasts, made scalars once (readfirstlane) and serve all t digits, each cut out by a scalar shift and
// mask and handed to v_mul_lo_u32 as its scalar operand. A ragged tile skips its empty waves and, in groups of kRkGroup = 8, its
// empty ciphertexts.
// The partial sums of the index splits meet by vector atomicAdd (global_atomic_add_u32, no return) on the words rekey_init_kernel
// has set on the same stream just before; every call initialises again, so a second call into the same buffer gives the same
// words. One path: a launch whose tiles alone fill the device has one split and still adds atomically. rs_emu_rekey
// (rs_emulate.cpp) walks the same workgroup / chunk / index / wave loop on the CPU through the helpers of rs_rekey.h.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_rekey.h"

namespace rs {

__global__ __launch_bounds__(kRkInitThreads) void rekey_init_kernel(RekeyArgs a, long words) {
  const long idx = (long)blockIdx.x * kRkInitThreads + threadIdx.x;
  if (idx >= words) return;
  const long W = (long)a.n_dst + 1;
  const long r = idx / W;
  const int w = (int)(idx - r * W);
  a.out[idx] = w == a.n_dst ? a.ct[(size_t)r * ((size_t)a.n_src + 1) + (size_t)a.n_src] : 0;
}

// the words of source index i this thread stages: rows j = wave + kRkWaves k, word w of each (zero past the output's width)
__device__ __forceinline__ void rekey_fetch(uint32_t (&pre)[kRkPre], const uint32_t* key, int n_dst, int t, int i, int wave, int w) {
#pragma unroll
  for (int k = 0; k < kRkPre; ++k) {
    const int j = wave + kRkWaves * k;
    if (j < t) pre[k] = w <= n_dst ? key[rk_key_offset(n_dst, t, i, j) + (size_t)w] : 0u;
  }
}

// acc[c] += kw0 digit(abar[c], shift0) (+ kw1 digit(abar[c], shift1)) for the ciphertexts of the wave, in groups of kRkGroup; the
// digits are scalars (abar is)
template <bool kPair>
__device__ __forceinline__ void rekey_sweep(uint32_t (&acc)[kRkWaveCts], const uint32_t (&abar)[kRkWaveCts], int rows, uint32_t kw0,
                                            uint32_t kw1, int shift0, int shift1, uint32_t mask) {
#pragma unroll
  for (int q = 0; q < kRkWaveCts / kRkGroup; ++q) {
    if (q * kRkGroup < rows) {
#pragma unroll
      for (int c = q * kRkGroup; c < (q + 1) * kRkGroup; ++c) {
        if (kPair) acc[c] += kw0 * ((abar[c] >> shift0) & mask) + kw1 * ((abar[c] >> shift1) & mask);
        else {                                              // a lone product would become v_mad_u64_u32 on a register pair
          uint32_t p;
          asm("v_mul_lo_u32 %0, %1, %2" : "=v"(p) : "v"(kw0), "s"((abar[c] >> shift0) & mask));
          acc[c] += p;
        }
      }
    }
  }
}

__global__ __launch_bounds__(kRkThreads) void rekey_kernel(RekeyArgs a, int span, int splits) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int t = a.t, n_src = a.n_src, n_dst = a.n_dst;
  const int lane = threadIdx.x & (kRkWords - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kRkWords));
  const unsigned wtiles = (unsigned)rk_word_tiles(n_dst);
  unsigned g = blockIdx.x;
  const int wt = (int)(g % wtiles); g /= wtiles;
  const int split = (int)(g % (unsigned)splits);
  const long ctile = (long)(g / (unsigned)splits);
  uint32_t* s_a = s_lds + wave * (kRkSeg * kRkWaveCts);     // this wave's [kRkSeg][kRkWaveCts]: a_i + offset, 0 past B
  uint32_t* s_key = s_lds + kRkWaves * kRkSeg * kRkWaveCts; // [t][kRkWords]: the key rows of one source index
  const long r0 = ctile * kRkTile + (long)wave * kRkWaveCts, left = a.B - r0;
  const int rows = left >= kRkWaveCts ? kRkWaveCts : left > 0 ? (int)left : 0;   // the same in every lane of the wave
  const int w = wt * kRkWords + lane;
  const uint32_t off = rk_offset(a.basebit, t), mask = (1u << a.basebit) - 1u;
  const int chunks = rk_chunks(n_src), c_first = split * span, c_last = c_first + span < chunks ? c_first + span : chunks;
  const int i_end = c_last * kRkSeg < n_src ? c_last * kRkSeg : n_src;
  const uint32_t* ct = reinterpret_cast<const uint32_t*>(a.ct) + (size_t)(rows > 0 ? r0 : 0) * ((size_t)n_src + 1);
  const uint32_t* key = reinterpret_cast<const uint32_t*>(a.key);
  uint32_t acc[kRkWaveCts];
#pragma unroll
  for (int c = 0; c < kRkWaveCts; ++c) acc[c] = 0u;
  uint32_t pre[kRkPre];
  rekey_fetch(pre, key, n_dst, t, c_first * kRkSeg, wave, w);
  for (int chunk = c_first; chunk < c_last; ++chunk) {
    const int i0 = chunk * kRkSeg, segn = n_src - i0 < kRkSeg ? n_src - i0 : kRkSeg;
    // the last sweep of the previous chunk has read s_a (the barrier behind it)
    for (int idx = lane; idx < segn * kRkWaveCts; idx += kRkWords) {
      const int c = idx / segn, ii = idx - c * segn;        // consecutive lanes: consecutive words of one sample
      s_a[rk_mask_index(ii, c)] = c < rows ? ct[(size_t)c * ((size_t)n_src + 1) + (size_t)(i0 + ii)] + off : 0u;
    }
    for (int ii = 0; ii < segn; ++ii) {
#pragma unroll
      for (int k = 0; k < kRkPre; ++k) {
        const int j = wave + kRkWaves * k;
        if (j < t) s_key[j * kRkWords + lane] = pre[k];
      }
      __syncthreads();
      if (i0 + ii + 1 < i_end) rekey_fetch(pre, key, n_dst, t, i0 + ii + 1, wave, w);
      if (rows > 0) {
        const uint4* a4 = reinterpret_cast<const uint4*>(s_a + rk_mask_index(ii, 0));
        uint32_t abar[kRkWaveCts];                          // the same words in every lane: scalars
#pragma unroll
        for (int q = 0; q < kRkWaveCts / 4; ++q) {
          const uint4 av = a4[q];
          abar[4 * q + 0] = (uint32_t)__builtin_amdgcn_readfirstlane((int)av.x);
          abar[4 * q + 1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)av.y);
          abar[4 * q + 2] = (uint32_t)__builtin_amdgcn_readfirstlane((int)av.z);
          abar[4 * q + 3] = (uint32_t)__builtin_amdgcn_readfirstlane((int)av.w);
        }
        int j = 0;
#pragma nounroll
        for (; j + 1 < t; j += 2) {                         // two digits a step: the two products and the sum fold into v_add3_u32
          const uint32_t kw0 = s_key[j * kRkWords + lane], kw1 = s_key[(j + 1) * kRkWords + lane];
          const int shift = 32 - (j + 1) * a.basebit;
          rekey_sweep<true>(acc, abar, rows, kw0, kw1, shift, shift - a.basebit, mask);
        }
        if (j < t) rekey_sweep<false>(acc, abar, rows, s_key[j * kRkWords + lane], 0u, 32 - (j + 1) * a.basebit, 0, mask);
      }
      __syncthreads();                                      // the sweep has read s_key (and, at the end of a chunk, s_a)
    }
  }
  if (w > n_dst) return;
  unsigned int* out = reinterpret_cast<unsigned int*>(a.out) + (size_t)(rows > 0 ? r0 : 0) * ((size_t)n_dst + 1) + (size_t)w;
#pragma unroll
  for (int c = 0; c < kRkWaveCts; ++c)
    if (c < rows) atomicAdd(out + (size_t)c * ((size_t)n_dst + 1), 0u - acc[c]);
}

hipError_t launch_rekey(const RekeyArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const long words = a.B * ((long)a.n_dst + 1);
  hipLaunchKernelGGL(rekey_init_kernel, dim3((unsigned)((words + kRkInitThreads - 1) / kRkInitThreads)), dim3(kRkInitThreads), 0, st, a, words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t lds = ((size_t)kRkWaves * kRkSeg * kRkWaveCts + (size_t)a.t * kRkWords) * sizeof(uint32_t);
  hipLaunchKernelGGL(rekey_kernel, dim3((unsigned)rk_groups(a.B, a.n_src, a.n_dst)), dim3(kRkThreads), lds, st, a,
                     rk_span(a.B, a.n_src, a.n_dst), rk_splits(a.B, a.n_src, a.n_dst));
  return hipGetLastError();
}

}  // namespace rs
