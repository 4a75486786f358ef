// rs_rows.hip -- the pre-pass of the indexed gate batches (rs_gate_rows_dev, rs_gate3_dev; include/redsec_hip.h):
//   gate_rows_kernel   row r of the staging buffer = c0 s0 + c1 s1 + c2 s2 + (0, bconst), the op of r's group applied to the three
//                      source rows its indices pick (or the trivial samples), word-wise mod 2^32
// An object of its own, so that every other kernel keeps its instructions. The bootstrap that follows reads the staging buffer
// through the unchanged path (rs_api.cpp run_bootstrap).
//
// Memory-bound: up to three rows read and one written per row, 4 B W 4 bytes per call (0.66 GB at B = 65,536, n = 630: a fraction
// of a millisecond beside a 300-ms bootstrap batch). A wave owns a row at a time, so the group, the op and the three indices are
// wave-uniform and every load and store is a run of consecutive dwords (W = n + 1 is odd: rows are not 16-byte aligned, nothing
// wider is used). No LDS, no atomics; the per-word arithmetic is that of rs_rows.h, which the lane emulator runs on the CPU.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_kernels.h"
#include "rs_rows.h"

namespace rs {

namespace {

constexpr int kRowsThreads = 256;
constexpr int kRowsWaves = kRowsThreads / 64;

}  // namespace

__global__ __launch_bounds__(kRowsThreads) void gate_rows_kernel(GateRowsArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // the row is the wave's: index loads and branches are scalar
  const long waves = (long)gridDim.x * kRowsWaves;
  for (long r = (long)blockIdx.x * kRowsWaves + wave; r < a.B; r += waves) row_lane(a, r, lane);
}

hipError_t launch_gate_rows(const GateRowsArgs& a, int num_cus, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.W < 1 || a.groups.count < 1 || a.groups.count > kRowMaxGroups || a.groups.end[a.groups.count - 1] != a.B) return hipErrorInvalidValue;
  // a wave per row at a time; eight workgroups of four waves fill a CU's 32 wave slots, the grid strides over the rows
  const dim3 grid((unsigned)std::min<long>((a.B + kRowsWaves - 1) / kRowsWaves, 8L * num_cus)), block(kRowsThreads);
  hipLaunchKernelGGL(gate_rows_kernel, grid, block, 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
