// rs_ring_selector_wide.hip -- the selector keyswitch of circuit bootstrapping at thousands of rows (rs_ring_selector_batch_dev,
// rs_circuit_bootstrap_batch_dev; include/redsec_hip.h):
//   ring_selector_wide_kernel      sel[k][f l + j] = - sum over ALL coordinates i and all q of d_iq(row k l + j) K[f][i][q]
// An object of its own, so that every earlier kernel keeps its instructions. Integer only, mod 2^32: no init kernel, no atomics, no
// floating point. The arithmetic, the key format and the digit rules are those of ring_selector_kernel (rs_ring_selector.h), so the
// words are the same whichever kernel a call takes.
//
// Why a second form. ring_selector_kernel cuts the n_src + 1 coordinates into chunks of 8 so that 30 l rows fill the device; its
// chunks meet by atomicAdd, ceil((n_src + 1) / 8) adds per output word. At 12,800 rows of redsec_small_v2 (n = 350, N = 1024,
// ks_t = 3) that is 12,800 x 4,096 x 44 x 4 B = 9.2 GB of atomic adds against 5.5e10 multiply-adds: about 7 ms at the 1.3 TB/s the
// chip sustains for float atomics (integer adds unmeasured) beside 1.5 ms of multiplies. With thousands of rows the parallelism is
// in the rows: here a workgroup owns the whole coordinate range of its tile and row block, keeps the sums in registers over the
// whole key stream and stores them once (210 MB at 12,800 rows).
//
// Placement (rs_ring_selector.h): kSeThreads = 128 threads on kSeTile = 512 coefficients of one polynomial of one family (thread t
// the coefficients k0 + 4t .. k0 + 4t + 3) and kSwRows consecutive rows. The key polynomials (i, q) of that tile are a run of
// (n_src + 1) ks_t 16-byte words per thread at a stride of 2 N words; a thread loads each ONCE (global_load_dwordx4), kSwPre = 4
// ahead of the multiplies, in a ring of registers that runs on across the staging pieces, and applies it to all rows of the block.
// The words x_i + off (b with its half step) are staged in LDS kSwPiece = 64 coordinates at a time, [coordinate][row], zero for the
// rows and coordinates that do not exist; they are the same in every lane, so each is made a scalar (readfirstlane) and the digit
// is cut out by scalar shift and mask, as ring_selector_kernel does. The sixteen words of a coordinate are made scalars once and
// kept over its ks_t digits, and the LDS read of the next coordinate's words is issued a coordinate ahead (reading and converting
// them per key word, as the chunked kernel does, cost 13 - 15 % at every row count: same-box A/B, profiles/r32/README.md).
//
// kSwRows = 16, from the arithmetic. A 16-byte key load feeds 4 kSwRows multiply-adds per lane, and the key passes through L2 and
// the Infinity Cache once per row block: rows / kSwRows x 17.3 MB at n = 350, N = 1024, ks_t = 3. The multiplies of 12,800 rows take
// 1.5 ms at the v_mul_lo_u32 ceiling of 3.66e13 / s, so the key must arrive at
//     kSwRows =  8:  1,600 x 17.3 MB = 27.7 GB in 1.5 ms = 18.4 TB/s    at or above what the L2s deliver chip-wide (16.8 - 18.8 TB/s)
//     kSwRows = 16:    800 x 17.3 MB = 13.8 GB in 1.5 ms =  9.2 TB/s    half of L2's rate, but above the Infinity Cache's 8.6 TB/s
//     kSwRows = 32:  4.6 TB/s, at 128 accumulators and 32 staged scalars a thread: two waves per SIMD at best to hide the loads behind
// 16 it is, at 64 accumulators: the loads then have to hit in L2. The grid order sees to that: (tile, polynomial, family) run
// fastest, and workgroups are dealt to the 8 XCDs in turn, so at N = 1024 an XCD only ever sees one of the 8 key streams (2.2 MB of
// 4 MB L2) and at N = 8192 eight of 64; its resident workgroups walk that stream at the same pace from the same start.
// kSwPiece = 64: 64 x 16 words = 4 KB of LDS, 8 words staged per thread per piece (lanes along the coordinates: coalesced reads of
// ct), two barriers per 64 ks_t key words of 64 multiply-adds each, under 2 % of the piece's instructions; n + 1 = 351 is 6 pieces.
// kSwPre = 4: the compiler forms each multiply-add as ONE v_mad_u64_u32 on a register pair (4.3 cycles, the rate of v_mul_lo_u32
// alone), so a key word is 64 of them, about 275 cycles of issue, and 4 words in flight cover about 1,100 cycles per wave. The
// pairs make the 64 accumulators 128 registers: 212 VGPRs, two waves per SIMD. kSwPre = 8 reaches 256 VGPRs and one wave per
// SIMD, and measured 1.6 x SLOWER from 3,840 rows on (same A/B), so 4 it stays; what the kernel reaches is 39 % of the multiply
// ceiling at 12,800 rows, and a lone workgroup walks its 1,053 key words in 0.51 ms, four times their issue time: the key loads'
// latency, not their bandwidth, is what is left (supposed from these two figures, not profiled). Sharing key words between the
// waves of a larger workgroup through LDS would attack the traffic, which is not the bound, and was not built.
// rs_emu_ring_selector_wide (rs_emulate.cpp) walks the same workgroup / piece / digit loop on the CPU as a second copy, not as
// shared code: a change to the loop below has to be made there too, or tests/test_ring_selector_batch_cpu.py stops pinning it.
// Resources (-Rpass-analysis=kernel-resource-usage): see INTEGRATION.md section 27. No scratch; static LDS kSwLdsBytes = 4,096.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_ring_selector.h"

namespace rs {

__global__ __launch_bounds__(kSeThreads) void ring_selector_wide_kernel(RingSelectorArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_x[kSwPiece * kSwRows];   // [ii][r]: x_i + off of row r0 + r, 0 where none
  const int N = a.N, n_src = a.n_src, ks_t = a.ks_t, t = threadIdx.x;
  const unsigned tiles = (unsigned)se_tiles(N);
  unsigned g = blockIdx.x;
  const int tile = (int)(g % tiles); g /= tiles;
  const int p = (int)(g & 1u); g >>= 1;
  const int f = (int)(g & 1u); g >>= 1;
  const long r0 = (long)g * kSwRows;
  const int rn = a.rows - r0 < (long)kSwRows ? (int)(a.rows - r0) : kSwRows;
  const uint32_t off = se_offset(a.ks_basebit, ks_t), mask = (1u << a.ks_basebit) - 1u;
  const uint32_t* ct = reinterpret_cast<const uint32_t*>(a.ct);
  const int k0 = tile * kSeTile + kSeKpt * t;
  const uint4* kp = reinterpret_cast<const uint4*>(reinterpret_cast<const uint32_t*>(a.key) + se_key_offset(N, n_src, ks_t, f, 0, 0, p) + k0);
  const size_t step = (size_t)N / 2;                          // 2 N words between K[f][i][q] and the next, in 16-byte units
  const int E = (n_src + 1) * ks_t;                           // the key polynomials of the tile, (i, q) in storage order
  uint4 pre[kSwPre];
#pragma unroll
  for (int k = 0; k < kSwPre; ++k) pre[k] = k < E ? kp[(size_t)k * step] : make_uint4(0u, 0u, 0u, 0u);
  uint32_t acc[kSwRows][kSeKpt];
#pragma unroll
  for (int r = 0; r < kSwRows; ++r)
#pragma unroll
    for (int c = 0; c < kSeKpt; ++c) acc[r][c] = 0u;
  int eb = 0;                                                 // key polynomials before this piece: a multiple of kSwPre
  for (int i0 = 0; i0 <= n_src; i0 += kSwPiece) {
    const int cn = n_src + 1 - i0 < kSwPiece ? n_src + 1 - i0 : kSwPiece;
    __syncthreads();                                          // the piece before has been read
#pragma unroll
    for (int s = t; s < kSwPiece * kSwRows; s += kSeThreads) {
      const int r = s / kSwPiece, ii = s - r * kSwPiece;      // lanes along the coordinates of one row
      uint32_t x = 0u;
      if (ii < cn && r < rn) {
        const int i = i0 + ii;
        x = ct[(size_t)(r0 + r) * ((size_t)n_src + 1) + (size_t)i] + off;
        if (i == n_src) x += se_half_step(a.basebit, (int)((r0 + r) % a.l));
      }
      s_x[ii * kSwRows + r] = x;
    }
    __syncthreads();
    const int En = cn * ks_t;
    int ii = 0, q = 0;
    const uint4* x4 = reinterpret_cast<const uint4*>(s_x);
    uint4 xn[kSwRows / 4];                                    // the staged words of the NEXT coordinate, read one coordinate ahead
#pragma unroll
    for (int v = 0; v < kSwRows / 4; ++v) xn[v] = x4[v];
    uint32_t x[kSwRows];                                      // the same sixteen words in every lane: scalars, kept over the ks_t digits
#pragma unroll
    for (int r = 0; r < kSwRows; ++r) x[r] = 0u;
    for (int e = 0; e < En; e += kSwPre) {
#pragma unroll
      for (int k = 0; k < kSwPre; ++k) {
        if (e + k < En) {                                     // the same in every lane
          const uint4 kw = pre[k];
          if (eb + e + k + kSwPre < E) pre[k] = kp[(size_t)(eb + e + k + kSwPre) * step];
          if (q == 0) {                                       // a new coordinate (the same in every lane)
#pragma unroll
            for (int v = 0; v < kSwRows / 4; ++v) {
              x[4 * v + 0] = (uint32_t)__builtin_amdgcn_readfirstlane((int)xn[v].x);
              x[4 * v + 1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)xn[v].y);
              x[4 * v + 2] = (uint32_t)__builtin_amdgcn_readfirstlane((int)xn[v].z);
              x[4 * v + 3] = (uint32_t)__builtin_amdgcn_readfirstlane((int)xn[v].w);
            }
            const int nx = ii + 1 < kSwPiece ? ii + 1 : ii;    // inside s_x; past the piece's last coordinate the words are not used
#pragma unroll
            for (int v = 0; v < kSwRows / 4; ++v) xn[v] = x4[nx * (kSwRows / 4) + v];
          }
          const int shift = 32 - (q + 1) * a.ks_basebit;
#pragma unroll
          for (int r = 0; r < kSwRows; ++r) {
            const uint32_t d = (x[r] >> shift) & mask;
            acc[r][0] += kw.x * d; acc[r][1] += kw.y * d; acc[r][2] += kw.z * d; acc[r][3] += kw.w * d;
          }
          if (++q == ks_t) { q = 0; ++ii; }
        }
      }
    }
    eb += En;
  }
#pragma unroll
  for (int r = 0; r < kSwRows; ++r) {
    if (r < rn) {
      uint32_t* out = reinterpret_cast<uint32_t*>(a.sel) + se_out_offset(N, a.l, (int)(r0 + r), f, p) + k0;
      *reinterpret_cast<uint4*>(out) = make_uint4(0u - acc[r][0], 0u - acc[r][1], 0u - acc[r][2], 0u - acc[r][3]);
    }
  }
}

hipError_t launch_ring_selector_wide(const RingSelectorArgs& a, hipStream_t st) {
  if (a.rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(ring_selector_wide_kernel, dim3((unsigned)sw_groups(a.rows, a.N)), dim3(kSeThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
