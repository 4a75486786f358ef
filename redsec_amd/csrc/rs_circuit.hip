// rs_circuit.hip -- the two kernels of the compiled circuits (rs_circuit_run_dev; include/redsec_hip.h), per level:
//   circuit_rows_kernel   staged row r = +-c0 s0 +- c1 s1 +- c2 s2 + (0, bconst) of cell r / lanes in lane r % lanes, the sources
//                         being rows of the arena (wire * lanes + lane) or the trivial samples; the second combination of the
//                         level's MUX rows behind the C * lanes own rows
//   circuit_fold_kernel   after the blind rotation: extracted sample of MUX row m += its second sample + (0, 1/8)
// An object of its own, so that every other kernel keeps its instructions. The blind rotation between the two and the keyswitch
// after them are the unchanged paths (rs_api.cpp rotate_rows / keyswitch_rows).
//
// Both are memory-bound: up to three rows read and one written per staged row, two read and one written per folded one. A wave owns
// a row at a time, so the cell (op, neg, the three wires) is a wave-uniform load from the table and every load and store of
// ciphertext words is a run of consecutive dwords (W = n + 1 and k N + 1 are odd: rows are not 16-byte aligned, nothing wider is
// used). No LDS, no atomics; the per-word arithmetic is that of rs_circuit.h, which the lane emulator runs on the CPU.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_circuit.h"
#include "rs_kernels.h"

namespace rs {

namespace {

constexpr int kCircuitThreads = 256;
constexpr int kCircuitWaves = kCircuitThreads / 64;

// a wave per row at a time; eight workgroups of four waves fill a CU's 32 wave slots, the grid strides over the rows
dim3 circuit_grid(long rows, int num_cus) {
  return dim3((unsigned)std::min<long>((rows + kCircuitWaves - 1) / kCircuitWaves, 8L * num_cus));
}

}  // namespace

__global__ __launch_bounds__(kCircuitThreads) void circuit_rows_kernel(CircuitLevelArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // the row is the wave's: the cell load and branches are scalar
  const long waves = (long)gridDim.x * kCircuitWaves, rows = circuit_level_rows(a);
  for (long r = (long)blockIdx.x * kCircuitWaves + wave; r < rows; r += waves) circuit_row_lane(a, r, lane);
}

__global__ __launch_bounds__(kCircuitThreads) void circuit_fold_kernel(CircuitFoldArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long waves = (long)gridDim.x * kCircuitWaves;
  for (long m = (long)blockIdx.x * kCircuitWaves + wave; m < a.mux_rows; m += waves) circuit_fold_lane(a, m, lane);
}

hipError_t launch_circuit_rows(const CircuitLevelArgs& a, int num_cus, hipStream_t st) {
  if (a.lanes <= 0 || a.C <= 0) return hipSuccess;
  if (a.W < 1 || a.M < 0 || a.M > a.C || a.first < 0 || !a.cells || !a.arena || !a.out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(circuit_rows_kernel, circuit_grid(circuit_level_rows(a), num_cus), dim3(kCircuitThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_circuit_fold(const CircuitFoldArgs& a, int num_cus, hipStream_t st) {
  if (a.mux_rows <= 0) return hipSuccess;
  if (a.words < 1 || a.mux_rows > a.B || !a.u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(circuit_fold_kernel, circuit_grid(a.mux_rows, num_cus), dim3(kCircuitThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
