// rs_sparse.hip -- the three kernels of the sparse bootstraps (rs_bootstrap_sparse_dev; include/redsec_hip.h):
//   sparse_gather_kernel    staged row i = in[live[i]] (the zero sample for an entry outside [0, B))
//   sparse_fill_kernel      out[r] = the bootstrapped trivial sample of (0, ..., 0, in[r][n]), for all B rows
//   sparse_scatter_kernel   after the bootstrap of the staged rows: out[live[i]] = its row i
// An object of its own, so that every other kernel keeps its instructions. The blind rotation and the keyswitch between the fill
// and the scatter are the unchanged paths (rs_api.cpp run_bootstrap) over the staged rows.
//
// All three are memory-bound: a row read and a row written (the fill: one word read). A wave owns a row at a time, so the live
// entry and the b word are wave-uniform loads and every load and store of ciphertext words is a run of consecutive dwords (W = n + 1
// is odd: rows are not 16-byte aligned, nothing wider is used). No LDS, no atomics; the row arithmetic is that of rs_sparse.h, which
// the lane emulator runs on the CPU.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_kernels.h"
#include "rs_sparse.h"

namespace rs {

namespace {

constexpr int kSparseThreads = 256;
constexpr int kSparseWaves = kSparseThreads / 64;

// a wave per row at a time; eight workgroups of four waves fill a CU's 32 wave slots, the grid strides over the rows
dim3 sparse_grid(long rows, int num_cus) {
  return dim3((unsigned)std::min<long>((rows + kSparseWaves - 1) / kSparseWaves, 8L * num_cus));
}

bool sparse_args_ok(const SparseArgs& a) { return a.W >= 1 && a.B > 0 && a.n_live >= 0 && a.n_live <= a.B && a.in && a.out; }
bool sparse_staged_ok(const SparseArgs& a) { return sparse_args_ok(a) && a.live && a.rows && a.boot; }

}  // namespace

__global__ __launch_bounds__(kSparseThreads) void sparse_gather_kernel(SparseArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // the row is the wave's: the entry load and its branch are scalar
  const long waves = (long)gridDim.x * kSparseWaves;
  for (long i = (long)blockIdx.x * kSparseWaves + wave; i < a.n_live; i += waves) sparse_gather_lane(a, i, lane);
}

__global__ __launch_bounds__(kSparseThreads) void sparse_fill_kernel(SparseArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long waves = (long)gridDim.x * kSparseWaves;
  for (long r = (long)blockIdx.x * kSparseWaves + wave; r < a.B; r += waves) {
    const int32_t b = a.in[r * a.W + a.W - 1];   // before the stores of this row: out may be in
    sparse_fill_lane(a, r, lane, b);
  }
}

__global__ __launch_bounds__(kSparseThreads) void sparse_scatter_kernel(SparseArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long waves = (long)gridDim.x * kSparseWaves;
  for (long i = (long)blockIdx.x * kSparseWaves + wave; i < a.n_live; i += waves) sparse_scatter_lane(a, i, lane);
}

hipError_t launch_sparse_gather(const SparseArgs& a, int num_cus, hipStream_t st) {
  if (a.n_live == 0) return hipSuccess;
  if (!sparse_staged_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sparse_gather_kernel, sparse_grid(a.n_live, num_cus), dim3(kSparseThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sparse_fill(const SparseArgs& a, int num_cus, hipStream_t st) {
  if (a.B == 0) return hipSuccess;
  if (!sparse_args_ok(a) || a.logn < kGenMinLogN || a.logn > kGenMaxLogN) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sparse_fill_kernel, sparse_grid(a.B, num_cus), dim3(kSparseThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sparse_scatter(const SparseArgs& a, int num_cus, hipStream_t st) {
  if (a.n_live == 0) return hipSuccess;
  if (!sparse_staged_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sparse_scatter_kernel, sparse_grid(a.n_live, num_cus), dim3(kSparseThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
