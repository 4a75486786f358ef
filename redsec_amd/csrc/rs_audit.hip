// rs_audit.hip -- device decryption and the exact noise audit of evaluation keys (rs_phase_dev, rs_audit_keys_dev,
// rs_audit_compressed_keys_dev; include/redsec_hip.h):
//   lwe_phase_kernel           phase = b - sum_k a_k key_k of LWE samples of any dimension up to kAuMaxDim
//   audit_bk_kernel<SEEDED>    the noise words of TGSW rows: e = b - a'*S - message, a' from HBM or from the mask seed
//   audit_ksk_kernel<SEEDED>   the noise word of every keyswitching sample, and the all-zero check of the v = 0 samples
//   audit_pack_kernel<SEEDED>  the noise words of packing-key rows (rs_audit_pack_key_dev): the c = 1 formula with t digits of basebit bits
// An object of its own, so that every other kernel keeps its instructions.
//
// All arithmetic is 32-bit integer (rs_audit.h): nothing here includes the split-key FP64 product that generated the key. The
// per-word functions are those of rs_audit.h, which the lane emulator (rs_emulate.cpp) runs on the CPU. The report fields are
// reduced per workgroup and leave by one integer atomic per field and workgroup: order-independent, hence deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_audit.h"
#include "rs_kernels.h"

namespace rs {

namespace {

constexpr int kAuWaves = kAuThreads / 64;
constexpr int kAuKeyWords = kAuMaxDim / 32;   // a packed key in LDS
constexpr int kAuBkHead = 16;                 // words in front of the bk kernel's dynamic LDS: the waves' tallies (keeps the mask 16-byte aligned)

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// dynamic LDS of audit_bk_kernel: [kAuBkHead] tallies, [N] mask, [N / 32] packed S, [N / 32 + 1] list offsets, [N] uint16 list
size_t audit_bk_lds_bytes(int N) {
  return sizeof(uint32_t) * ((size_t)kAuBkHead + N + N / 32 + (N / 32 + 1)) + sizeof(uint16_t) * (size_t)N;
}

}  // namespace

__global__ __launch_bounds__(kAuThreads) void lwe_phase_kernel(PhaseArgs a) {
  __shared__ uint32_t s_key[kAuKeyWords];
  const int t = threadIdx.x, lane = t & 63, dim = a.dim;
  for (int i = t; i < (dim + 31) / 32; i += kAuThreads) s_key[i] = a.key_bits[i];
  __syncthreads();
  const long waves = (long)gridDim.x * kAuWaves;
  for (long i = (long)blockIdx.x * kAuWaves + (t >> 6); i < a.B; i += waves) {
    const uint32_t* row = reinterpret_cast<const uint32_t*>(a.ct) + i * (dim + 1);
    const uint32_t dot = wave_sum(au_lane_dot(row, dim, s_key, lane));
    if (lane == 0) a.phase[i] = (int32_t)(row[dim] - dot);
  }
}

template <bool SEEDED>
__global__ __launch_bounds__(kAuThreads) void audit_ksk_kernel(AuditArgs a) {
  __shared__ uint32_t s_key[kAuKeyWords];
  __shared__ uint32_t s_max[kAuWaves];
  __shared__ unsigned long long s_over[kAuWaves], s_zero[kAuWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = a.n;
  for (int i = t; i < (n + 31) / 32; i += kAuThreads) s_key[i] = a.lwe_bits[i];
  __syncthreads();
  uint32_t key[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) key[k] = a.seed[k];
  AuTally tally{0u, 0ull};
  unsigned long long zero_bad = 0ull;
  const long samples = ((long)a.N * a.t) << a.basebit, waves = (long)gridDim.x * kAuWaves;
  const uint32_t* ksk = reinterpret_cast<const uint32_t*>(a.ksk);
  for (long s = (long)blockIdx.x * kAuWaves + wave; s < samples; s += waves) {
    int i, j, v;
    au_ksk_sample((uint64_t)s, a.t, a.basebit, i, j, v);   // wave-uniform
    uint32_t e = 0u;
    if (v == 0) {
      if (!SEEDED) zero_bad += wave_or(au_lane_or(ksk + s * (n + 1), n, lane)) != 0u ? 1u : 0u;
    } else {
      uint32_t dot, b;
      if (SEEDED) {
        uint32_t acc = 0u;
        for (int k0 = 0; k0 < n; k0 += kKgChunk) acc += au_ksk_seeded_lane_dot(key, (uint64_t)s, k0, lane, n, s_key);
        dot = wave_sum(acc);
        b = ksk[s];
      } else {
        const uint32_t* row = ksk + s * (n + 1);
        dot = wave_sum(au_lane_dot(row, n, s_key, lane));
        b = row[n];
      }
      e = au_ksk_noise(b, dot, au_ksk_message(au_key_bit(a.tlwe_bits, i), v, j, a.basebit));
      au_tally_word(tally, e, a.ksk_limit);   // the same in every lane of the wave; lane 0's copy is the wave's
    }
    if (lane == 0 && a.ksk_noise) a.ksk_noise[s] = (int32_t)e;
  }
  if (lane == 0) { s_max[wave] = tally.max_abs; s_over[wave] = tally.over; s_zero[wave] = zero_bad; }
  __syncthreads();
  if (t == 0) {
    AuTally all{0u, 0ull};
    unsigned long long zb = 0ull;
    for (int w = 0; w < kAuWaves; ++w) { au_tally_merge(all, AuTally{s_max[w], s_over[w]}); zb += s_zero[w]; }
    if (all.max_abs) atomicMax(&a.report->ksk_max_abs, all.max_abs);
    if (all.over) atomicAdd(&a.report->ksk_over, all.over);
    if (zb) atomicAdd(&a.report->ksk_zero_bad, zb);
  }
}

template <bool SEEDED>
__global__ __launch_bounds__(kAuThreads) void audit_bk_kernel(AuditArgs a) {
  extern __shared__ uint32_t s_lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, N = a.N, SW = N / 32;
  uint32_t* s_a = s_lds + kAuBkHead;
  uint32_t* s_S = s_a + N;
  int* s_off = reinterpret_cast<int*>(s_S + SW);
  uint16_t* s_list = reinterpret_cast<uint16_t*>(s_off + SW + 1);
  // the set bits of S, listed once per workgroup in ascending order
  for (int w = t; w < SW; w += kAuThreads) s_S[w] = a.tlwe_bits[w];
  __syncthreads();
  if (t == 0) {
    int at = 0;
    for (int w = 0; w < SW; ++w) { s_off[w] = at; at += __popc(s_S[w]); }
    s_off[SW] = at;
  }
  __syncthreads();
  for (int w = t; w < SW; w += kAuThreads) au_list_word(s_S[w], w, s_off[w], s_list);
  __syncthreads();
  const int cnt = s_off[SW];
  uint32_t key[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) key[k] = a.seed[k];
  AuTally tally{0u, 0ull};
  const long rows = (long)a.n * 2 * a.l;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    int i, c, j;
    au_bk_row((uint64_t)row, a.l, i, c, j);
    const uint32_t s = au_key_bit(a.lwe_bits, i), g = au_gadget(j, a.bgbit);
    const uint32_t* b_row;
    if (SEEDED) {
      for (int blk = t; blk < N / 16; blk += kAuThreads) {
        uint32_t w[16];
        kg_bk_mask_block(key, (uint64_t)row, blk, w);
#pragma unroll
        for (int q = 0; q < 16; ++q) s_a[16 * blk + q] = w[q];
      }
      b_row = reinterpret_cast<const uint32_t*>(a.bk) + row * N;
    } else {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(a.bk) + row * 2 * N;
      for (int k = t; k < N; k += kAuThreads) s_a[k] = src[k];
      b_row = src + N;
    }
    __syncthreads();
    for (int k0 = t; k0 < N; k0 += kAuThreads * kAuKpt) {
      uint32_t acc[kAuKpt];
      au_bk_products(s_a, N, s_list, cnt, k0, acc);
#pragma unroll
      for (int q = 0; q < kAuKpt; ++q) {
        const int k = k0 + kAuThreads * q;
        const uint32_t e = au_bk_noise(b_row[k], acc[q], au_bk_message(c, s, g, k, au_key_bit(s_S, k)));
        au_tally_word(tally, e, a.bk_limit);
        if (a.bk_noise) a.bk_noise[row * N + k] = (int32_t)e;
      }
    }
    __syncthreads();   // the mask is read to the end before the next row overwrites it
  }
  const uint32_t wmax = wave_max(tally.max_abs);
  const unsigned long long wover = wave_sum64(tally.over);
  if (lane == 0) { s_lds[wave] = wmax; s_lds[4 + 2 * wave] = (uint32_t)wover; s_lds[5 + 2 * wave] = (uint32_t)(wover >> 32); }
  __syncthreads();
  if (t == 0) {
    AuTally all{0u, 0ull};
    for (int w = 0; w < kAuWaves; ++w) au_tally_merge(all, AuTally{s_lds[w], ((unsigned long long)s_lds[5 + 2 * w] << 32) | s_lds[4 + 2 * w]});
    if (all.max_abs) atomicMax(&a.report->bk_max_abs, all.max_abs);
    if (all.over) atomicAdd(&a.report->bk_over, all.over);
  }
}

// The packing key: audit_bk_kernel's walk (the set bits of S listed once per workgroup, the row's mask in LDS, a signed sum of
// rotations per coefficient) on rows i t + j with the message s_i g_j X^0. A sparse sweep over the listed bits, on purpose another
// loop than the generator's dense scalar-masked sweep (rs_packkey.hip): the two share the ChaCha streams and nothing else.
template <bool SEEDED>
__global__ __launch_bounds__(kAuThreads) void audit_pack_kernel(AuditPackArgs a) {
  extern __shared__ uint32_t s_lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, N = a.N, SW = N / 32;
  uint32_t* s_a = s_lds + kAuBkHead;
  uint32_t* s_S = s_a + N;
  int* s_off = reinterpret_cast<int*>(s_S + SW);
  uint16_t* s_list = reinterpret_cast<uint16_t*>(s_off + SW + 1);
  for (int w = t; w < SW; w += kAuThreads) s_S[w] = a.tlwe_bits[w];
  __syncthreads();
  if (t == 0) {
    int at = 0;
    for (int w = 0; w < SW; ++w) { s_off[w] = at; at += __popc(s_S[w]); }
    s_off[SW] = at;
  }
  __syncthreads();
  for (int w = t; w < SW; w += kAuThreads) au_list_word(s_S[w], w, s_off[w], s_list);
  __syncthreads();
  const int cnt = s_off[SW];
  uint32_t key[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) key[k] = a.seed[k];
  AuTally tally{0u, 0ull};
  const long rows = (long)a.n * a.t;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    int i, j;
    au_pack_row((uint64_t)row, a.t, i, j);
    const uint32_t s = au_key_bit(a.lwe_bits, i), g = au_gadget(j, a.basebit);
    const uint32_t* b_row;
    if (SEEDED) {
      for (int blk = t; blk < N / 16; blk += kAuThreads) {
        uint32_t w[16];
        au_pack_mask_block(key, (uint64_t)row, blk, w);
#pragma unroll
        for (int q = 0; q < 16; ++q) s_a[16 * blk + q] = w[q];
      }
      b_row = reinterpret_cast<const uint32_t*>(a.key) + row * N;
    } else {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(a.key) + row * 2 * N;
      for (int k = t; k < N; k += kAuThreads) s_a[k] = src[k];
      b_row = src + N;
    }
    __syncthreads();
    for (int k0 = t; k0 < N; k0 += kAuThreads * kAuKpt) {
      uint32_t acc[kAuKpt];
      au_bk_products(s_a, N, s_list, cnt, k0, acc);
#pragma unroll
      for (int q = 0; q < kAuKpt; ++q) {
        const int k = k0 + kAuThreads * q;
        const uint32_t e = au_bk_noise(b_row[k], acc[q], au_bk_message(1, s, g, k, 0u));
        au_tally_word(tally, e, a.limit);
        if (a.noise) a.noise[row * N + k] = (int32_t)e;
      }
    }
    __syncthreads();   // the mask is read to the end before the next row overwrites it
  }
  const uint32_t wmax = wave_max(tally.max_abs);
  const unsigned long long wover = wave_sum64(tally.over);
  if (lane == 0) { s_lds[wave] = wmax; s_lds[4 + 2 * wave] = (uint32_t)wover; s_lds[5 + 2 * wave] = (uint32_t)(wover >> 32); }
  __syncthreads();
  if (t == 0) {
    AuTally all{0u, 0ull};
    for (int w = 0; w < kAuWaves; ++w) au_tally_merge(all, AuTally{s_lds[w], ((unsigned long long)s_lds[5 + 2 * w] << 32) | s_lds[4 + 2 * w]});
    if (all.max_abs) atomicMax(&a.report->bk_max_abs, all.max_abs);
    if (all.over) atomicAdd(&a.report->bk_over, all.over);
  }
}

hipError_t launch_lwe_phase(const PhaseArgs& a, int num_cus, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.dim < 1 || a.dim > kAuMaxDim) return hipErrorInvalidValue;
  // a wave per sample at a time; eight workgroups of four waves fill a CU's 32 wave slots
  const dim3 grid((unsigned)std::min<long>((a.B + kAuWaves - 1) / kAuWaves, 8L * num_cus)), block(kAuThreads);
  hipLaunchKernelGGL(lwe_phase_kernel, grid, block, 0, st, a);
  return hipGetLastError();
}

hipError_t launch_audit_bk(const AuditArgs& a, bool seeded, int num_cus, hipStream_t st) {
  const long rows = (long)a.n * 2 * a.l;
  if (rows <= 0) return hipSuccess;
  if (a.N < kAuThreads * kAuKpt || a.N > 65536 || (a.N & (a.N - 1)) != 0) return hipErrorInvalidValue;   // the list holds uint16 positions
  // 6.4 KB of LDS at N = 1024, 51 KB at N = 8192 (three workgroups per CU); the grid strides over the rows
  const dim3 grid((unsigned)std::min<long>(rows, 4L * num_cus)), block(kAuThreads);
  const size_t lds = audit_bk_lds_bytes(a.N);
  if (seeded) hipLaunchKernelGGL(audit_bk_kernel<true>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(audit_bk_kernel<false>, grid, block, lds, st, a);
  return hipGetLastError();
}

hipError_t launch_audit_pack(const AuditPackArgs& a, bool seeded, int num_cus, hipStream_t st) {
  const long rows = (long)a.n * a.t;
  if (rows <= 0) return hipSuccess;
  if (a.N < kAuThreads * kAuKpt || a.N > 65536 || (a.N & (a.N - 1)) != 0) return hipErrorInvalidValue;   // the list holds uint16 positions
  const dim3 grid((unsigned)std::min<long>(rows, 4L * num_cus)), block(kAuThreads);   // the placement of launch_audit_bk
  const size_t lds = audit_bk_lds_bytes(a.N);
  if (seeded) hipLaunchKernelGGL(audit_pack_kernel<true>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(audit_pack_kernel<false>, grid, block, lds, st, a);
  return hipGetLastError();
}

hipError_t launch_audit_ksk(const AuditArgs& a, bool seeded, int num_cus, hipStream_t st) {
  const long samples = ((long)a.N * a.t) << a.basebit;
  if (samples <= 0) return hipSuccess;
  if (a.n < 1 || a.n > kAuMaxDim) return hipErrorInvalidValue;
  const dim3 grid((unsigned)std::min<long>((samples + kAuWaves - 1) / kAuWaves, 8L * num_cus)), block(kAuThreads);
  if (seeded) hipLaunchKernelGGL(audit_ksk_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(audit_ksk_kernel<false>, grid, block, 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
