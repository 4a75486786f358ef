// rs_bootstrap.h -- what the three translation units of the N = 1024 blind rotation share (rs_bootstrap.hip,
// rs_bootstrap_split.hip, rs_bootstrap_listed.hip; redsec_amd/build.py says why they are three objects): the transform
// policies, the device helpers used by kernels of more than one unit, the launch helpers that cross units and the one
// definition of the diagnostic stamp array.
//   XfNtt<Cfg>  exact negacyclic NTT over a 51-bit prime carried in FP64 (rs_ntt.h)  -- guaranteed exact
//   XfFft<Cfg>  folded 512-point complex FP64 FFT (rs_fft.h), TFHE's own arithmetic class -- 2.5x fewer
//               FP64 ops; exact after rounding with overwhelming probability, with a run-time certificate
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "rs_fft.h"
#include "rs_cohort.h"
#include "rs_diag.h"
#include "rs_kernels.h"
#include "rs_lds_plan.h"
#include "rs_ntt.h"

namespace rs {

// Same-wave LDS hand-off: DS operations of one wavefront execute in order, so only the compiler
// needs to be told not to move LDS accesses across this point.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void stage_tables(double* s_tw, const double* tw_g, int nthreads, int count) {
  for (int i = threadIdx.x; i < count; i += nthreads) s_tw[i] = tw_g[i];
  __syncthreads();
}

// -------------------------------------------------------------------------------------------------
// Transform policies
// -------------------------------------------------------------------------------------------------
template <class C>
struct XfNtt {
  using Cfg = C;
  static constexpr int kTableDoubles = kTwTotal;   // staged in LDS
  static constexpr bool kCertificate = false;
  static constexpr bool kSplitKeyLoads = false;   // whole key row prefetched across the transform
  static constexpr bool kWorkgroupForm = false;
  static constexpr bool kPreparedDigits = false;  // digits extracted from the raw rotated difference
  struct State { const double* tw; };
  __device__ static __forceinline__ void init(State& st, int, const double* tw_lds, const double*) { st.tw = tw_lds; }
  using LatencyState = State;   // the cooperative kernel's twiddle source (XfFft keeps its per-lane twiddles in registers there)
  __device__ static __forceinline__ void init_latency(LatencyState& st, int lane, const double* tw_lds, const double* tw_g) { init(st, lane, tw_lds, tw_g); }

  __device__ static __forceinline__ void fwd_digits(int lane, double (&x)[kRegs], const int32_t (&d)[kRegs], int q, uint32_t offset,
                                                    const State& st, double* buf, const Field& f) {
    const double* tw = st.tw;
    fwd_F1_digits<C>(lane, x, d, q, offset, tw, buf, f);
    wave_lds_sync();
    fwd_F2<C>(lane, x, tw, buf, f);
    wave_lds_sync();
    fwd_F3(lane, x, buf);
    wave_lds_sync();
    fwd_F4<C>(lane, x, tw, buf, f);
    wave_lds_sync();
  }
  __device__ static __forceinline__ void fwd_generic(int lane, double (&x)[kRegs], const State& st, double* buf, const Field& f) {
    const double* tw = st.tw;
    fwd_F1<C>(lane, x, tw, buf, f);
    wave_lds_sync();
    fwd_F2<C>(lane, x, tw, buf, f);
    wave_lds_sync();
    fwd_F3(lane, x, buf);
    wave_lds_sync();
    fwd_F4<C>(lane, x, tw, buf, f);
    wave_lds_sync();
  }
  // key values: scaled by 1/N and fully reduced; stored as pairs (positions 16 lane + 2v, +1)
  __device__ static __forceinline__ void key_store(double2* dst, int lane, const double (&x)[kRegs], double scale, const Field& f) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const double a = f_reduce(f_mulmod(f_reduce(x[2 * v], f), scale, f), f);
      const double b = f_reduce(f_mulmod(f_reduce(x[2 * v + 1], f), scale, f), f);
      dst[v * 64 + lane] = make_double2(a, b);
    }
  }
  // multiply-accumulate against key entries v0 .. v0+3 of both columns
  __device__ static __forceinline__ void mac(double (&s0)[kRegs], double (&s1)[kRegs], const double (&x)[kRegs],
                                             const double2 (&w0)[4], const double2 (&w1)[4], int v0, const Field& f) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = v0 + k;
      s0[2 * v] += f_mulmod(x[2 * v], w0[k].x, f);
      s0[2 * v + 1] += f_mulmod(x[2 * v + 1], w0[k].y, f);
      s1[2 * v] += f_mulmod(x[2 * v], w1[k].x, f);
      s1[2 * v + 1] += f_mulmod(x[2 * v + 1], w1[k].y, f);
    }
  }
  __device__ static __forceinline__ void mac8(double (&s0)[kRegs], double (&s1)[kRegs], const double (&x)[kRegs],
                                              const double2 (&w0)[8], const double2 (&w1)[8], const Field& f) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      s0[2 * v] += f_mulmod(x[2 * v], w0[v].x, f);
      s0[2 * v + 1] += f_mulmod(x[2 * v + 1], w0[v].y, f);
      s1[2 * v] += f_mulmod(x[2 * v], w1[v].x, f);
      s1[2 * v + 1] += f_mulmod(x[2 * v + 1], w1[v].y, f);
    }
  }
  __device__ static __forceinline__ void mid(double (&s0)[kRegs], double (&s1)[kRegs], const Field& f) {
    if (C::MID_REDUCE) {
#pragma unroll
      for (int u = 0; u < kRegs; ++u) { s0[u] = f_reduce(s0[u], f); s1[u] = f_reduce(s1[u], f); }
    }
  }
  __device__ static __forceinline__ double partial(double v, const Field& f) { return f_reduce(v, f); }
  __device__ static __forceinline__ void inverse(int lane, double (&x)[kRegs], const State& st, double* buf, const Field& f) {
    const double* twi = st.tw + kN;
    inv_I1<C>(lane, x, twi, buf, f);
    wave_lds_sync();
    inv_I2<C>(lane, x, twi, buf, f);
    wave_lds_sync();
    inv_I3(lane, x, buf);
    wave_lds_sync();
    inv_I4<C>(lane, x, twi, buf, f);
    wave_lds_sync();
  }
  __device__ static __forceinline__ void inverse2(int lane, double (&xa)[kRegs], double (&xb)[kRegs], const State& st, double* buf, const Field& f) {
    inverse(lane, xa, st, buf, f);
    inverse(lane, xb, st, buf, f);
  }
  __device__ static __forceinline__ int32_t to_torus(double v, double&) { return f_to_torus32(v); }
};

template <class C>
struct XfFft {
  using Cfg = C;
  static constexpr int kTableDoubles = kFftTwDoubles;   // stage-transposed complex table staged in LDS (8 KB)
  static constexpr bool kCertificate = true;
  static constexpr bool kSplitKeyLoads = true;    // second half of the key row fetched after the transform
  static constexpr bool kWorkgroupForm = true;    // blind_rotate_wg_kernel available
  static constexpr bool kPreparedDigits = true;   // d[] = gadget_prepare(rotated difference): one v_bfe_i32 per digit
  // Twiddles are read from the LDS table at every use: keeping the 21 complex values of a lane in
  // registers (FftTw) spilled 250 B/lane to scratch at the 256-VGPR budget and cost 40 % (scratch
  // reloads share vmcnt with the in-flight key-row loads).
  using State = FftTwTable;
  __device__ static __forceinline__ void init(State& st, int lane, const double* tw_lds, const double*) { st.tw = tw_lds; st.lane = lane; }

  // One wave per SIMD in the cooperative kernel (512 registers): all eight per-lane twiddles stay in registers
  using LatencyState = FftTwKept<3>;
  __device__ static __forceinline__ void init_latency(LatencyState& st, int lane, const double* tw_lds, const double* tw_g) {
    State t;
    init(t, lane, tw_lds, tw_g);
    fft_kept_load(st, t);
  }
  template <class TWS>
  __device__ static __forceinline__ void fwd_generic(int lane, double (&x)[kRegs], const TWS& st, double* buf, const Field&) {
    ffwd_F1(lane, x, st, buf);
    wave_lds_sync();
    ffwd_F2(lane, x, st, buf);
    wave_lds_sync();
    ffwd_F3(lane, x, buf);
    wave_lds_sync();
    ffwd_F4(lane, x, st, buf);
    wave_lds_sync();
  }
  template <class TWS>
  __device__ static __forceinline__ void fwd_digits(int lane, double (&x)[kRegs], const int32_t (&d)[kRegs], int q, uint32_t offset,
                                                    const TWS& st, double* buf, const Field& f) {
#pragma unroll
    for (int r = 0; r < kRegs; ++r) x[r] = (double)gadget_digit_prepared<C>(d[r], q);
    fwd_generic(lane, x, st, buf, f);
  }
  // key values scaled by 1/M (exact power of two); stored as (re, im) of position 8 lane + v
  __device__ static __forceinline__ void key_store(double2* dst, int lane, const double (&x)[kRegs], double, const Field&) {
#pragma unroll
    for (int v = 0; v < 8; ++v) dst[v * 64 + lane] = make_double2(x[v] * (1.0 / kM), x[v + 8] * (1.0 / kM));
  }
  __device__ static __forceinline__ void mac(double (&s0)[kRegs], double (&s1)[kRegs], const double (&x)[kRegs],
                                             const double2 (&w0)[4], const double2 (&w1)[4], int v0, const Field&) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = v0 + k;
      fft_cmac(s0[v], s0[v + 8], x[v], x[v + 8], w0[k].x, w0[k].y);
      fft_cmac(s1[v], s1[v + 8], x[v], x[v + 8], w1[k].x, w1[k].y);
    }
  }
  __device__ static __forceinline__ void mac8(double (&s0)[kRegs], double (&s1)[kRegs], const double (&x)[kRegs],
                                              const double2 (&w0)[8], const double2 (&w1)[8], const Field&) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      fft_cmac(s0[v], s0[v + 8], x[v], x[v + 8], w0[v].x, w0[v].y);
      fft_cmac(s1[v], s1[v + 8], x[v], x[v + 8], w1[v].x, w1[v].y);
    }
  }
  __device__ static __forceinline__ void mid(double (&)[kRegs], double (&)[kRegs], const Field&) {}
  __device__ static __forceinline__ double partial(double v, const Field&) { return v; }
  template <class TWS>
  __device__ static __forceinline__ void inverse(int lane, double (&x)[kRegs], const TWS& st, double* buf, const Field&) {
    finv_I1(lane, x, st, buf);
    wave_lds_sync();
    finv_I2(lane, x, st, buf);
    wave_lds_sync();
    finv_I3(lane, x, buf);
    wave_lds_sync();
    finv_I4(lane, x, st, buf);
    wave_lds_sync();
  }
  // both accumulator columns at once: the two inverse transforms interleaved phase by phase
  __device__ static __forceinline__ void inverse2(int lane, double (&xa)[kRegs], double (&xb)[kRegs], const State& st, double* buf, const Field&) {
    finv_pair<false>(lane, xa, xb, st, buf, [] { wave_lds_sync(); });
  }
  __device__ static __forceinline__ int32_t to_torus(double v, double& dev) { return fft_round_torus32(v, dev); }

  // workgroup kernel: planar exchanges through a half-size per-wave buffer
  static constexpr int kWgBufDoubles = kPlaneDoubles;
  __device__ static __forceinline__ void inverse_wg(int lane, double (&x)[kRegs], const State& st, double* buf, const Field&) {
    finv_planar(lane, x, st, buf, [] { wave_lds_sync(); });
  }
  __device__ static __forceinline__ void digits(double (&x)[kRegs], const int32_t (&d)[kRegs], int q) {
#pragma unroll
    for (int r = 0; r < kRegs; ++r) x[r] = (double)gadget_digit_prepared<C>(d[r], q);
  }
  // the lock-step workgroup kernel's pairs: per-lane twiddles from registers (FftTwKept) or the LDS tables (State)
  template <class TWS>
  __device__ static __forceinline__ void fwd_pair_wg(int lane, double (&xa)[kRegs], double (&xb)[kRegs], const TWS& st, double* buf) {
    ffwd_pair<true>(lane, xa, xb, st, buf, [] { wave_lds_sync(); });
  }
  template <class TWS>
  __device__ static __forceinline__ void inverse_pair_wg(int lane, double (&xa)[kRegs], double (&xb)[kRegs], const TWS& st, double* buf) {
    finv_pair<true>(lane, xa, xb, st, buf, [] { wave_lds_sync(); });
  }
  static constexpr int kWgTableDoubles = kFftTwDoubles;
};

// largest rounding distance of the wave -> device flag (positive doubles order like their bit patterns)
__device__ __forceinline__ void publish_certificate(double dev, unsigned long long* flag, int lane) {
  if (!flag) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(dev, off, 64);
    dev = o > dev ? o : dev;
  }
  if (lane == 0) atomicMax(flag, (unsigned long long)__double_as_longlong(dev));
}

// Initial accumulator body: (test polynomial * X^rot)_j. Constant test vector (tfhe_bootstrap_woKS_FFT) or, in
// the programmable form, the ciphertext's own polynomial lut[ct % lut_count] (tfhe_blindRotateAndExtract_FFT).
__device__ __forceinline__ int32_t test_vector(const BlindRotateArgs& a, long ct, int j, int rot) {
  if (!a.lut) return rotated_const(a.mu, j, rot);
  const int32_t* v = a.lut + (size_t)((ct + a.lut_first) % a.lut_count) * kN;
  const int aa = rot & (kN - 1), nb = (rot >> 10) & 1;
  const uint32_t x = (uint32_t)v[(j - aa) & (kN - 1)];
  return (int32_t)((((j < aa) ? 1 : 0) ^ nb) ? 0u - x : x);
}

// Exact recomputation gate (see BlindRotateArgs::gate_flag). Uniform over the grid: every thread reads the
// same word, so whole workgroups leave before their first barrier. Returns true when the launch has nothing to do.
__device__ __forceinline__ bool recompute_not_needed(const BlindRotateArgs& a) {
  if (!a.gate_flag) return false;
  const unsigned long long bits = *(const volatile unsigned long long*)a.gate_flag;   // positive doubles order like their bit patterns
  const bool needed = bits >= a.gate_limit_bits;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (a.running_flag) atomicMax(a.running_flag, bits);
    if (needed && a.fallback_count) atomicAdd(a.fallback_count, 1ull);
  }
  return !needed;
}

// -------------------------------------------------------------------------------------------------
// Key rows through LDS (the lock-step and duo kernels) and their multiply-accumulate streams
// -------------------------------------------------------------------------------------------------
// Direct global -> LDS loads, 16 bytes per lane = 1 KB per wave-instruction, NCHUNK consecutive KB:
// global address = wave-uniform base (SGPR pair) + lane_off (one VGPR, lane * 16) + k KB; LDS address =
// M0 + k KB + lane * 16 (the instruction offset advances both sides). Written as asm because (a) hipcc
// puts a vmcnt(0) in front of the next LDS read whenever it knows of a pending LDS-DMA, which would
// serialise the prefetch -- the kernels' own `s_waitcnt vmcnt(0)` + barrier orders the data instead;
// (b) with per-lane 64-bit source pointers the compiler spilled around the issue point, and every
// scratch reload there waits on vmcnt, i.e. on the key rows that were just requested.
template <int NCHUNK>
__device__ __forceinline__ void glds_chunks(const double* gsrc_wave_base, unsigned lane_off, const double* lds_wave_base) {
  static_assert(NCHUNK >= 1 && NCHUNK <= 4, "instruction offsets are 13-bit signed");
  const unsigned lds_dst = (unsigned)__builtin_amdgcn_readfirstlane(
      (int)(unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)lds_wave_base);
  const unsigned long long base = (unsigned long long)(uintptr_t)gsrc_wave_base;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32));
  const unsigned long long sbase = ((unsigned long long)hi << 32) | lo;
  unsigned keep;
  if constexpr (NCHUNK == 1) {
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(sbase), "s"(lds_dst) : "memory");
  } else if constexpr (NCHUNK == 2) {
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:1024\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(sbase), "s"(lds_dst) : "memory");
  } else {
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:1024\n\tglobal_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:3072\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(sbase), "s"(lds_dst) : "memory");
    static_assert(NCHUNK == 4, "1, 2 or 4 chunks");
  }
}

// The same with the LDS side given as a byte address (a workgroup-uniform unsigned: no generic-pointer cast, whose null check
// costs three scalar instructions per call) and the global side as a wave-uniform pointer the caller keeps running.
template <int NCHUNK>
__device__ __forceinline__ void glds_chunks_at(const double* gsrc_wave_base, unsigned lane_off, unsigned lds_byte_addr) {
  static_assert(NCHUNK == 1 || NCHUNK == 2 || NCHUNK == 4, "1, 2 or 4 chunks of 1 KB per wave");
  unsigned keep;
  if constexpr (NCHUNK == 1) {
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(gsrc_wave_base), "s"(lds_byte_addr) : "memory");
  } else if constexpr (NCHUNK == 2) {
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:1024\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(gsrc_wave_base), "s"(lds_byte_addr) : "memory");
  } else {
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:1024\n\tglobal_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:3072\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(gsrc_wave_base), "s"(lds_byte_addr) : "memory");
  }
}

// Pointwise multiply-accumulate of a transform PAIR against its two key rows in LDS (FFT policies), as one
// stream: 8 steps of two complex positions (4 ds_read_b128: both columns), the reads of step k+1 issued
// before the FMAs of step k. Read in four blocks of 8 with the FMAs after each block (mac_row), every
// block exposed a fresh LDS latency because the FMAs of a block drain its reads (in-order return).
#define RS_MAC_FENCE() __builtin_amdgcn_sched_barrier(0)
// col0 / col1: offsets (in double2) of the column multiplied into s0 / s1 within a key row -- 0 and kN / 2 for (column 0, column 1);
// the duo kernel passes them swapped for its odd waves, so that s0 is always the column the wave itself inverts
__device__ __forceinline__ void mac_pair_stream(double (&s0)[kRegs], double (&s1)[kRegs], const double (&xa)[kRegs], const double (&xb)[kRegs],
                                                const double* keyA, const double* keyB, int lane, int col0 = 0, int col1 = kN / 2) {
  const double2* ka = reinterpret_cast<const double2*>(keyA);
  const double2* kb = reinterpret_cast<const double2*>(keyB);
  double2 u[2][4];
  auto issue = [&](int step, double2 (&w)[4]) {
    const double2* k0 = (step < 4 ? ka : kb) + col0;
    const double2* k1 = (step < 4 ? ka : kb) + col1;
    const int v = 2 * (step & 3);
    w[0] = k0[v * 64 + lane]; w[1] = k0[(v + 1) * 64 + lane];
    w[2] = k1[v * 64 + lane]; w[3] = k1[(v + 1) * 64 + lane];
  };
  auto fma = [&](int step, const double2 (&w)[4]) {
    const double (&x)[kRegs] = step < 4 ? xa : xb;
    const int v = 2 * (step & 3);
    fft_cmac(s0[v], s0[v + 8], x[v], x[v + 8], w[0].x, w[0].y);
    fft_cmac(s0[v + 1], s0[v + 9], x[v + 1], x[v + 9], w[1].x, w[1].y);
    fft_cmac(s1[v], s1[v + 8], x[v], x[v + 8], w[2].x, w[2].y);
    fft_cmac(s1[v + 1], s1[v + 9], x[v + 1], x[v + 9], w[3].x, w[3].y);
  };
  issue(0, u[0]);
#pragma unroll
  for (int step = 0; step < 8; ++step) {
    if (step + 1 < 8) issue(step + 1, u[(step + 1) & 1]);
    RS_MAC_FENCE();
    fma(step, u[step & 1]);
    RS_MAC_FENCE();
  }
}

// The same for the SPLIT key (blind_rotate_wgs_kernel, blind_rotate_duos_kernel): one transform against one 16 KB half-row.
// s0 += x * (column at k0), s1 += x * (column at k1): the two columns of one key half-row
__device__ __forceinline__ void mac_half_stream_cols(double (&s0)[kRegs], double (&s1)[kRegs], const double (&x)[kRegs], const double2* k0, const double2* k1, int lane) {
  double2 u[2][4];
  auto issue = [&](int step, double2 (&w)[4]) {
    const int v = 2 * step;
    w[0] = k0[v * 64 + lane]; w[1] = k0[(v + 1) * 64 + lane];
    w[2] = k1[v * 64 + lane]; w[3] = k1[(v + 1) * 64 + lane];
  };
  auto fma = [&](int step, const double2 (&w)[4]) {
    const int v = 2 * step;
    fft_cmac(s0[v], s0[v + 8], x[v], x[v + 8], w[0].x, w[0].y);
    fft_cmac(s0[v + 1], s0[v + 9], x[v + 1], x[v + 9], w[1].x, w[1].y);
    fft_cmac(s1[v], s1[v + 8], x[v], x[v + 8], w[2].x, w[2].y);
    fft_cmac(s1[v + 1], s1[v + 9], x[v + 1], x[v + 9], w[3].x, w[3].y);
  };
  issue(0, u[0]);
#pragma unroll
  for (int step = 0; step < 4; ++step) {
    if (step + 1 < 4) issue(step + 1, u[(step + 1) & 1]);
    RS_MAC_FENCE();
    fma(step, u[step & 1]);
    RS_MAC_FENCE();
  }
}

__device__ __forceinline__ void mac_half_stream(double (&s0)[kRegs], double (&s1)[kRegs], const double (&x)[kRegs], const double* key, int lane) {
  const double2* k0 = reinterpret_cast<const double2*>(key);
  mac_half_stream_cols(s0, s1, x, k0, k0 + kN / 2, lane);
}

// -------------------------------------------------------------------------------------------------
// Launch helpers that cross the units
// -------------------------------------------------------------------------------------------------
// Which transform policies have a blind_rotate_coop8_listed_kernel (rs_bootstrap_listed.hip, which static_asserts that it
// instantiates exactly these): the cfg id launch_coop8_listed takes, or -1 -- the plan then names blind_rotate_coop8_kernel.
template <class Xf> inline constexpr int kCoop8ListedCfg = -1;
template <> inline constexpr int kCoop8ListedCfg<XfFft<CfgDefault128>> = 0;
hipError_t launch_coop8_listed(int cfg, const BlindRotateArgs& a, hipStream_t st);                  // rs_bootstrap_listed.hip
// the split duo form's launch (mid-size batches of the split mode): rs_bootstrap.hip, called from rs_bootstrap_split.hip
hipError_t launch_split_duos(int cfg, const BlindRotateArgs& a, long grid, hipStream_t st);

// The compile-time facts of a policy that the launch plan depends on (rs_launch_plan.h never sees the policy types).
template <class Xf>
constexpr FormTraits form_traits(bool split = false) {
  return {Xf::kWorkgroupForm, Xf::Cfg::L, std::is_same_v<typename Xf::Cfg, CfgRedsecV2>, split ? -1 : kCoop8ListedCfg<Xf>, split};
}

// The caller's arguments cut down to the rows of one step of the plan. No table and no counter: cohort_setup and
// counter_setup below are the ONLY places that hand a kernel a progress table or a work counter.
inline BlindRotateArgs step_args(const BlindRotateArgs& whole, const LaunchStep& s) {
  BlindRotateArgs a = whole;
  a.B = s.rows;
  a.in0 += s.first * a.W;
  if (a.in1) a.in1 += s.first * a.W;
  a.u_out += s.first * (kN + 1);
  if (a.lut) a.lut_first = (int32_t)((a.lut_first + s.first) % a.lut_count);
  a.progress = nullptr; a.cohort_every = 0; a.cohort_lag = 0;
  a.counter = nullptr;                       // every wave has exactly one ciphertext
  return a;
}
// XCD cohorts of the lock-step kernels (cohort_step, rs_cohort.h), where the plan says so: the table filled with "absent".
inline hipError_t cohort_setup(BlindRotateArgs& w, int* table, const LaunchStep& s, hipStream_t st) {
  if (!s.cohort) return hipSuccess;
  w.progress = table; w.cohort_every = s.cohort_every; w.cohort_lag = s.cohort_lag;
  return hipMemsetAsync(table, 0x7f, 8 * kCohortSlots * sizeof(int), st);
}
// The work counter of a persistent per-wave launch, zeroed on the stream.
inline hipError_t counter_setup(BlindRotateArgs& w, unsigned int* counter, const LaunchStep& s, hipStream_t st) {
  if (!s.persistent) return hipSuccess;
  if (!counter) return hipErrorInvalidValue;   // (a context created without one plans with no_persist)
  w.counter = counter;
  return hipMemsetAsync(counter, 0, sizeof(unsigned int), st);
}

}  // namespace rs

// Diagnostic builds only (rs_diag.h): the phase sums, [workgroup < 256][wave][phase], and rs_debug_read_stamps (not part of
// include/redsec_hip.h), which copies them to the host and clears them. Written once here; the unit whose stamped kernel a
// build switches on instantiates it (the build has no relocatable device code: the array lives beside the kernel that writes it).
#define RS_DEFINE_STAMPS()                                                                                                    \
  namespace rs { __device__ unsigned long long g_rs_stamps[256 * 8 * diag::kStampPhases]; }                                   \
  extern "C" int rs_debug_read_stamps(unsigned long long* host, size_t count) {                                               \
    const size_t all = sizeof(rs::g_rs_stamps) / sizeof(unsigned long long);                                                  \
    if (count > all) count = all;                                                                                             \
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(rs::g_rs_stamps), count * sizeof(unsigned long long)) != hipSuccess) return 1;   \
    static unsigned long long zeros[256 * 8 * rs::diag::kStampPhases];                                                        \
    return hipMemcpyToSymbol(HIP_SYMBOL(rs::g_rs_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : 1;                        \
  }
