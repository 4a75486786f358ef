// rs_ring_selector.hip -- the selector keyswitch of circuit bootstrapping (rs_ring_selector_dev, rs_circuit_bootstrap_dev;
// include/redsec_hip.h):
//   ring_selector_init_kernel      sel = 0
//   ring_selector_kernel           sel[k][f l + j] -= sum over one chunk of coordinates i and all q of d_iq(row k l + j) K[f][i][q]
//   circuit_prepare_kernel         the l constant test polynomials h_j / 2 and the row index r / l of rs_circuit_bootstrap_dev
// An object of its own, so that every earlier kernel keeps its instructions. Integer only: a ks_basebit-bit digit times a 32-bit
// word, accumulated mod 2^32, exact in any order, so neither the chunking nor the row blocks can change a word.
//
// ring_selector_kernel is a small exact GEMM against a key stream (rs_ring_selector.h): every sample lands on X^0, so there is no
// rotation and no (-p, p) window, and every key word serves all rows of a call. A workgroup of kSeThreads = 128 threads owns kSeTile
// = 512 consecutive coefficients of one polynomial of one family, one chunk of kSeChunk = 8 coordinates and one block of kSeRows = 8
// sample rows: thread t keeps 4 coefficients x 8 rows in 32 accumulators. The chunk's key words are a run of cn ks_t polynomials at a
// stride of 2 N words; a thread loads its 16 bytes of each ONCE (global_load_dwordx4), kSePre = 4 loads ahead of the multiplies, and
// applies them to all eight rows. The words x_i + off of the chunk (8 x 8, zero past the rows and coordinates that exist) are staged
// in LDS once; they are the same in every lane, so each is made a scalar (readfirstlane), the digit is cut out by scalar shift and
// mask and handed to the multiply as its scalar operand. Rows past one block run as further workgroups that read the key again (it
// then comes from the cache: 34 MB at n = 350, N = 1024, ks_t = 6). The partial sums of the chunks meet by vector atomicAdd
// (global_atomic_add_u32, no return) on the words ring_selector_init_kernel has zeroed on the same stream just before; every call
// initialises again, so a second call into the same buffer gives the same words.
// rs_emu_ring_selector (rs_emulate.cpp) walks the same workgroup / coordinate / digit loop on the CPU as a second copy, not as
// shared code: a change to the loop below has to be made there too, or tests/test_ring_selector_cpu.py stops pinning this kernel.
// Resources (-Rpass-analysis=kernel-resource-usage): see INTEGRATION.md section 24.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_ring_selector.h"

namespace rs {

__global__ __launch_bounds__(kSeInitThreads) void ring_selector_init_kernel(int32_t* sel, long words) {
  const long idx = (long)blockIdx.x * kSeInitThreads + threadIdx.x;
  if (idx < words) sel[idx] = 0;
}

__global__ __launch_bounds__(kSeInitThreads) void circuit_prepare_kernel(CircuitPrepareArgs a) {
  const long idx = (long)blockIdx.x * kSeInitThreads + threadIdx.x;
  const long lut_words = (long)a.l * a.N;
  if (idx < lut_words) a.lut[idx] = (int32_t)se_half_step(a.basebit, (int)(idx / a.N));
  else if (idx < lut_words + a.rows) a.index[idx - lut_words] = (int32_t)((idx - lut_words) / a.l);
}

__global__ __launch_bounds__(kSeThreads) void ring_selector_kernel(RingSelectorArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_x[kSeChunk * kSeRows];   // [ii][r]: x_i + off of row r0 + r, 0 where none
  const int N = a.N, n_src = a.n_src, ks_t = a.ks_t, t = threadIdx.x;
  const unsigned tiles = (unsigned)se_tiles(N), chunks = (unsigned)se_chunks(n_src);
  unsigned g = blockIdx.x;
  const int tile = (int)(g % tiles); g /= tiles;
  const int p = (int)(g & 1u); g >>= 1;
  const int f = (int)(g & 1u); g >>= 1;
  const int chunk = (int)(g % chunks);
  const int r0 = (int)(g / chunks) * kSeRows, rows = (int)a.rows;           // depth l <= 30 x 31
  const int i0 = chunk * kSeChunk, cn = n_src + 1 - i0 < kSeChunk ? n_src + 1 - i0 : kSeChunk;
  const int rn = rows - r0 < kSeRows ? rows - r0 : kSeRows;
  const uint32_t off = se_offset(a.ks_basebit, ks_t), mask = (1u << a.ks_basebit) - 1u;
  if (t < kSeChunk * kSeRows) {
    const int ii = t / kSeRows, r = t - ii * kSeRows;
    uint32_t x = 0u;
    if (ii < cn && r < rn) {
      const int i = i0 + ii;
      x = reinterpret_cast<const uint32_t*>(a.ct)[(size_t)(r0 + r) * ((size_t)n_src + 1) + (size_t)i] + off;
      if (i == n_src) x += se_half_step(a.basebit, (r0 + r) % a.l);
    }
    s_x[t] = x;
  }
  __syncthreads();
  const int k0 = tile * kSeTile + kSeKpt * t;
  const uint4* kp = reinterpret_cast<const uint4*>(reinterpret_cast<const uint32_t*>(a.key) + se_key_offset(N, n_src, ks_t, f, i0, 0, p) + k0);
  const size_t step = (size_t)N / 2;                          // 2 N words between K[f][i][q] and the next, in 16-byte units
  const int E = cn * ks_t;                                    // the key polynomials of the chunk, (i, q) in storage order
  uint4 pre[kSePre];
#pragma unroll
  for (int k = 0; k < kSePre; ++k) pre[k] = k < E ? kp[(size_t)k * step] : make_uint4(0u, 0u, 0u, 0u);
  uint32_t acc[kSeRows][kSeKpt];
#pragma unroll
  for (int r = 0; r < kSeRows; ++r)
#pragma unroll
    for (int c = 0; c < kSeKpt; ++c) acc[r][c] = 0u;
  int ii = 0, q = 0;
  for (int e = 0; e < E; e += kSePre) {
#pragma unroll
    for (int k = 0; k < kSePre; ++k) {
      if (e + k < E) {                                        // the same in every lane
        const uint4 kw = pre[k];
        if (e + k + kSePre < E) pre[k] = kp[(size_t)(e + k + kSePre) * step];
        const uint4* x4 = reinterpret_cast<const uint4*>(s_x + ii * kSeRows);
        const uint4 xa = x4[0], xb = x4[1];                   // the same eight words in every lane: scalars
        const uint32_t x[kSeRows] = {
            (uint32_t)__builtin_amdgcn_readfirstlane((int)xa.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)xa.y),
            (uint32_t)__builtin_amdgcn_readfirstlane((int)xa.z), (uint32_t)__builtin_amdgcn_readfirstlane((int)xa.w),
            (uint32_t)__builtin_amdgcn_readfirstlane((int)xb.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)xb.y),
            (uint32_t)__builtin_amdgcn_readfirstlane((int)xb.z), (uint32_t)__builtin_amdgcn_readfirstlane((int)xb.w)};
        const int shift = 32 - (q + 1) * a.ks_basebit;
#pragma unroll
        for (int r = 0; r < kSeRows; ++r) {
          const uint32_t d = (x[r] >> shift) & mask;
          acc[r][0] += kw.x * d; acc[r][1] += kw.y * d; acc[r][2] += kw.z * d; acc[r][3] += kw.w * d;
        }
        if (++q == ks_t) { q = 0; ++ii; }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kSeRows; ++r) {
    if (r < rn) {
      unsigned int* out = reinterpret_cast<unsigned int*>(a.sel) + se_out_offset(N, a.l, r0 + r, f, p) + k0;
#pragma unroll
      for (int c = 0; c < kSeKpt; ++c) atomicAdd(out + c, 0u - acc[r][c]);
    }
  }
}

hipError_t launch_ring_selector(const RingSelectorArgs& a, hipStream_t st) {
  if (a.rows <= 0) return hipSuccess;
  const long words = a.rows * 4 * (long)a.N;
  hipLaunchKernelGGL(ring_selector_init_kernel, dim3((unsigned)((words + kSeInitThreads - 1) / kSeInitThreads)), dim3(kSeInitThreads), 0,
                     st, a.sel, words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ring_selector_kernel, dim3((unsigned)se_groups(a.rows, a.N, a.n_src)), dim3(kSeThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_circuit_prepare(const CircuitPrepareArgs& a, hipStream_t st) {
  if (a.rows <= 0) return hipSuccess;
  const long words = (long)a.l * a.N + a.rows;
  hipLaunchKernelGGL(circuit_prepare_kernel, dim3((unsigned)((words + kSeInitThreads - 1) / kSeInitThreads)), dim3(kSeInitThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
