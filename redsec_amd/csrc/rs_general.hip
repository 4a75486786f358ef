// rs_general.hip -- kernels of the general ring path (rs_general.h): N in {1024, 2048, 4096, 8192}, any gadget,
// key split into two 16-bit halves so that the FP64 FFT product is exact by an a-priori bound (RS_MODE_FFT_SPLIT).
//
//   gen_bk_transform_kernel    key polynomial -> two transformed half polynomials (the bkFFT analogue)
//   gen_blind_rotate_kernel    gate pre-combination + modswitch + n CMUX steps + sample extract
//                              (tfhe_bootstrap_woKS_FFT / tfhe_blindRotateAndExtract_FFT; REDsec: lib/BinOps_enc.cpp:185,191)
//   gen_polymul_kernel         debug/parity tap through the same transform path
//   gen_keygen_bk_kernel       evaluation-key generation: TGSW rows of the bootstrapping key, b = a*S + e through the same product
//   keygen_ksk_kernel          evaluation-key generation: keyswitching-key samples (integer stream work)
//   expand_bk_kernel           compressed-key expansion: bk masks regenerated from the mask seed, bodies copied beside them
//   expand_ksk_kernel          compressed-key expansion: ksk masks regenerated from the mask seed, bodies copied beside them
//
// One workgroup of T = N/16 threads owns one ciphertext: its TRLWE accumulator (2 x N int32) and the two exchange
// planes live in LDS (17 N bytes), every thread keeps 8 complex values of the transform in flight and the
// 2 halves x 2 columns of pointwise sums in registers. Workgroups are persistent over the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "rs_diag.h"
#include "rs_general.h"
#include "rs_keygen.h"
#include "rs_kernels.h"

namespace rs {

namespace {

__device__ __forceinline__ void gen_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int T>
__device__ __forceinline__ void gen_sync() {
  if constexpr (T == 64) gen_wave_sync(); else __syncthreads();
}

// key loads as SGPR base + 32-bit lane offset (global_load ... v_off, s[base:base+1]): the row pointer is the same in every
// lane, and left as a 64-bit per-lane pointer the compiler kept a VGPR pair and two adds per (half, column, position) stream
// The thread index as an opaque value: address arithmetic that depends on it is then recomputed where it is used (a few shifts
// and adds) instead of being hoisted out of the CMUX loop and held -- or spilled -- for the whole kernel.
__device__ __forceinline__ int gen_local(int t) {
  asm volatile("" : "+v"(t));
  return t;
}
typedef double GenD2 __attribute__((ext_vector_type(2)));
typedef const GenD2 __attribute__((address_space(1)))* GenKeyPtr;   // global address space kept through the integer round trip
__device__ __forceinline__ GenKeyPtr gen_uniform_ptr(const double2* p) {
  const uint64_t b = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return (GenKeyPtr)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ GenKeyPtr gen_uniform_ptr(GenKeyPtr p) {   // of an already uniform value: folds to the scalar itself
  const uint64_t b = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return (GenKeyPtr)(((uint64_t)hi << 32) | lo);
}
// `base` already includes the (half, column, position) displacement; made opaque here so that the optimiser does not move
// that constant over to the lane offset (which turns every stream back into a 64-bit per-lane pointer)
__device__ __forceinline__ double2 gen_key_load(GenKeyPtr base, uint32_t lane_bytes) {
  typedef const char __attribute__((address_space(1)))* BytePtr;
  asm volatile("" : "+v"(lane_bytes));   // not hoisted, so that base + offset is selected as ONE load with a scalar base
  const GenD2 v = *(GenKeyPtr)((BytePtr)gen_uniform_ptr(base) + lane_bytes);
  return make_double2(v.x, v.y);
}

__device__ __forceinline__ void gen_publish(double dev, unsigned long long* flag) {
  if (!flag) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(dev, off, 64);
    dev = o > dev ? o : dev;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(flag, (unsigned long long)__double_as_longlong(dev));
}

}  // namespace

// Levels 0..8 of the twiddle table staged in LDS (8 KB; rs_general.h, gen_pass_tw, kGenStageTw). Measured at full size
// (profiles/r03/f_general_ab_twiddles_in_lds.jsonl): redsec_params_medium +8.9 % (two workgroups per CU, every pass used to wait
// for an L1/L2 round trip of its own), redsec_params_large -3.9 % (one 512-thread workgroup per CU on 139 KB of LDS already: the
// extra LDS reads queue behind its exchanges) -- so N = 8192 keeps reading the table from global memory.
template <int LOGN>
__device__ __forceinline__ const double* gen_stage_twiddles(double* s_twn, const double* tw, int t) {
  if constexpr (kGenStageTw<LOGN>) {
    for (int i = t; i < 2 * kGenTwLds; i += Gen<LOGN>::T) s_twn[i] = tw[i];
    __syncthreads();
    return s_twn;
  } else {
    return tw;
  }
}

template <int LOGN>
__global__ __launch_bounds__(Gen<LOGN>::T) void gen_bk_transform_kernel(const int32_t* __restrict__ bk, double* __restrict__ bk_x,
                                                                         const double* __restrict__ tw, long n_polys) {
  using G = Gen<LOGN>;
  constexpr int N = G::N, M = G::M, T = G::T;
  __shared__ double s_re[G::kPlane], s_im[G::kPlane];
  __shared__ double s_twn[kGenStageTw<LOGN> ? 2 * kGenTwLds : 2];
  const int t = threadIdx.x;
  auto sync = [] { gen_sync<T>(); };
  auto wsync = [] { gen_wave_sync(); };
  const double* twn = gen_stage_twiddles<LOGN>(s_twn, tw, t);
  for (long poly = blockIdx.x; poly < n_polys; poly += gridDim.x) {
    const int32_t* src = bk + poly * N;
#pragma unroll 1
    for (int piece = 0; piece < 2; ++piece) {
      double x[kRegs];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        int32_t lo, hi;
        gen_split_key(src[t + T * r], lo, hi);
        x[r] = (double)(piece ? hi : lo);
        gen_split_key(src[t + T * r + M], lo, hi);
        x[r + 8] = (double)(piece ? hi : lo);
      }
      gen_fft_fwd<LOGN>(x, t, tw, twn, s_re, s_im, sync, wsync);
      // [row pair index][piece][column][8][T] complex, scaled by 1/M (a power of two: exact)
      double2* dst = reinterpret_cast<double2*>(bk_x) + ((size_t)(poly >> 1) * 4 + (size_t)piece * 2 + (size_t)(poly & 1)) * M;
#pragma unroll
      for (int r = 0; r < 8; ++r) dst[r * T + t] = make_double2(x[r] * (1.0 / M), x[r + 8] * (1.0 / M));
    }
  }
}

// Choices of gen_blind_rotate_kernel, each from a same-box A/B (profiles/r03/f_*, h_*, profiles/r04/x_*; MEASUREMENTS.md section 4.5): two key
// positions requested ahead of the one being multiplied (three spill and lose); a row's first key position requested in front of its
// transform's last exchange (not in front of the transform, behind it, or behind the last exchange); the two inverse transforms of a
// column as a pipelined pair; no whole-row prefetch at the start of a step (1.2-1.5 % slower); no de-phasing of an XCD's workgroups
// at kernel start (no effect). Diagnostic builds (rs_diag.h, RS_DIAG bit 16) replace every key load by register values.
// A key chunk of the row at `p`; under the no-key probe a value made of registers instead (no load at all; results wrong).
__device__ __forceinline__ double2 gen_key_or_probe(GenKeyPtr p, uint32_t tb, double pa, double pb) {
  if constexpr (diag::kNoKeyProbe) { (void)p; (void)tb; return make_double2(pa, pb); }
  else { (void)pa; (void)pb; return gen_key_load(p, tb); }
}
template <int LOGN>
__global__ __launch_bounds__(Gen<LOGN>::T) __attribute__((amdgpu_waves_per_eu(2, 2))) void gen_blind_rotate_kernel(GenArgs a) {
  using G = Gen<LOGN>;
  constexpr int N = G::N, M = G::M, T = G::T;
  __shared__ double s_re[G::kPlane], s_im[G::kPlane];
  __shared__ int32_t s_acc[2][N];
  __shared__ double s_twn[kGenStageTw<LOGN> ? 2 * kGenTwLds : 2];
  const int t = threadIdx.x;
  auto sync = [] { gen_sync<T>(); };
  auto wsync = [] { gen_wave_sync(); };
  const double* twn = gen_stage_twiddles<LOGN>(s_twn, a.tw, t);
  const int l = a.l, bgbit = a.bgbit, n = a.n;
  // The LAST pass's twiddles of this thread stay in registers for the whole kernel where that pass reads the table from GLOBAL
  // memory (N >= 2048: its levels lie above the LDS-staged ones): same-box +3.7 % at N = 4096 and +3.4 % at N = 8192 -- those loads
  // were requested one exchange ahead of their use and mostly waited for (profiles/r03/h_general_ab_last_pass_twiddles_kept.txt,
  // h_general_ab_which_pass_kept.txt). Keeping an LDS-served pass costs more in spilled registers than its reads save (pass 1 or 2
  // at N = 4096: -0.7 % / -3.8 %).
  constexpr bool kLastPassGlobal = !kGenStageTw<LOGN> || (2 << (Gen<LOGN>::LOGM - 1)) > kGenTwLds;
  constexpr int kKeepPass = (Gen<LOGN>::P >= 2 && kLastPassGlobal) ? Gen<LOGN>::P - 1 : -1;
  GenPassTw tw_kept;
  if constexpr (kKeepPass == 1) gen_pass_tw<LOGN, 1>(tw_kept, t, a.tw, twn);
  if constexpr (kKeepPass == 2 && Gen<LOGN>::P > 2) gen_pass_tw<LOGN, 2>(tw_kept, t, a.tw, twn);
  if constexpr (kKeepPass == 3 && Gen<LOGN>::P > 3) gen_pass_tw<LOGN, 3>(tw_kept, t, a.tw, twn);
  const GenKeptTw kept1{kKeepPass >= 1 && kKeepPass < Gen<LOGN>::P ? &tw_kept : nullptr, kKeepPass};
  const uint32_t goff = gen_gadget_offset(l, bgbit);
  double dev = 0.0;

  // (XCD cohorts, rs_cohort.h, were tried here in round 4 -- wave 0 posting the step count and waiting for its XCD's slowest workgroup -- and
  // cost 7 % at N = 4096 and 3 % at N = 8192 whether switched on or off: the few registers of the cohort state spill 10-20 more dwords per lane in
  // kernels that were full (profiles/r04/x_ab_general_cohorts_and_xcd_rotation.txt). The fabric traffic of these kernels sits at the 8-XCD
  // floor without them.)
  for (long ct = blockIdx.x; ct < a.B; ct += gridDim.x) {
    const int32_t* row0 = a.in0 + ct * a.W;
    const int32_t* row1 = a.in1 ? a.in1 + ct * a.W : nullptr;
    // gate pre-combination (0, bconst) + c0*in0 + c1*in1, evaluated word by word as it is consumed
    auto word = [&](int i) -> int32_t {
      uint32_t v = (uint32_t)a.c0 * (uint32_t)row0[i];
      if (row1) v += (uint32_t)a.c1 * (uint32_t)row1[i];
      return (int32_t)v;
    };
    {
      const int32_t barb = gen_modswitch((int32_t)((uint32_t)word(n) + (uint32_t)a.bconst), LOGN);
      const int rot = 2 * N - barb;   // in (0, 2N]
      const int32_t* lut = a.lut ? a.lut + (size_t)((ct + a.lut_first) % a.lut_count) * N : nullptr;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = t + T * (r & 7) + (r >> 3) * M;
        s_acc[0][j] = 0;
        if (!lut) {
          s_acc[1][j] = gen_rotated_const(a.mu, j, rot, LOGN);
        } else {   // (X^rot * lut)_j: the ciphertext's own test polynomial (tfhe_blindRotateAndExtract_FFT)
          const int aa = rot & (N - 1), nb = (rot >> LOGN) & 1;
          const uint32_t x = (uint32_t)lut[(j - aa) & (N - 1)];
          s_acc[1][j] = (int32_t)((((j < aa) ? 1 : 0) ^ nb) ? 0u - x : x);
        }
      }
    }
    sync();

    int32_t bara_next = gen_modswitch(word(0), LOGN);
    for (int i = 0; i < n; ++i) {
      const int32_t bara = __builtin_amdgcn_readfirstlane(bara_next);   // the same word in every thread
      bara_next = (i + 1 < n) ? gen_modswitch(word(i + 1), LOGN) : 0;
      if (bara == 0) continue;   // tfhe_blindRotate_FFT skips the identity CMUX (uniform over the workgroup)
      double S[2][2][kRegs];     // [key half][column]
      const uint32_t tb = (uint32_t)t * (uint32_t)sizeof(double2);
      // prepared rotated difference of one component, shared by its l digit rows
      auto prep = [&](int comp, int32_t (&v)[kRegs]) {
          // all 32 accumulator words first, then the arithmetic: left to itself the compiler read them one at a time, each
          // behind a full s_waitcnt (24 exposed LDS round trips per component; the ISA timeline of profiles/r03 shows it)
          const int32_t* accc = s_acc[comp];
          const int aa = bara & (N - 1), nb = (bara >> LOGN) & 1;
          uint32_t rot[kRegs], own[kRegs];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = t + T * (r & 7) + (r >> 3) * M;
            rot[r] = (uint32_t)accc[(j - aa) & (N - 1)];
            own[r] = (uint32_t)accc[j];
          }
          gen_wave_sync();   // compiler-only: keep the reads together, ahead of their uses
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = t + T * (r & 7) + (r >> 3) * M;
            const int neg = (j < aa ? 1 : 0) ^ nb;
            v[r] = gen_gadget_prepare((int32_t)((neg ? (0u - rot[r]) : rot[r]) - own[r]), goff);   // gen_rotated_diff, same arithmetic
          }
      };
      // one digit row: transform, then both key halves x both columns multiplied into S
      auto row = [&](int comp, int q, const int32_t (&v)[kRegs]) {
          double x[kRegs];
#pragma unroll
          for (int r = 0; r < 16; ++r) x[r] = (double)gen_gadget_digit(v[r], q, bgbit);
          GenKeyPtr kp = gen_uniform_ptr(reinterpret_cast<const double2*>(a.bk_x) + ((size_t)i * 2 * l + (size_t)comp * l + q) * 4 * M);
          constexpr int LA = 2, NB = LA + 1;   // key positions requested ahead of the one being multiplied
          double2 w[NB][4];
          // both halves x both columns of position r; position 0 is requested in front of the transform's last exchange, position
          // r + LA before the FMAs of position r (the compiler's own schedule waited for each group of four in full before its 16
          // FMAs: eight exposed L2 round trips per row, most of a CMUX step on the large rings)
          constexpr int kFirstGroups = LOGN >= 13 ? 2 : 1;   // N = 8192 (with the row rotation): 458.5 -> 445.7 ms; N = 4096: +0.4 % at best
          constexpr int FG = kFirstGroups < LA ? kFirstGroups : LA;   // positions requested at the tail hook
          auto first = [&] {
#pragma unroll
            for (int g = 0; g < FG; ++g) {
#pragma unroll
              for (int hc = 0; hc < 4; ++hc) {
                w[g][hc] = gen_key_or_probe(kp + (size_t)hc * M + g * T, tb, 1.0 + hc, 2.0 + g);
              }
            }
            __builtin_amdgcn_sched_barrier(0);
          };
          gen_fft_fwd<LOGN>(x, gen_local(t), a.tw, twn, s_re, s_im, sync, wsync, first, kept1);
#pragma unroll
          for (int g = FG; g < LA; ++g) {
#pragma unroll
            for (int hc = 0; hc < 4; ++hc) {
              w[g][hc] = gen_key_or_probe(kp + (size_t)hc * M + g * T, tb, x[hc + g], x[hc + 8]);
            }
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            if (r + LA < (diag::kHalfKeyProbe ? 4 : 8)) {
#pragma unroll
              for (int hc = 0; hc < 4; ++hc) {
                w[(r + LA) % NB][hc] = gen_key_or_probe(kp + (size_t)hc * M + (r + LA) * T, tb, x[hc + 1], x[hc + 4]);
              }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int hc = 0; hc < 4; ++hc) fft_cmac(S[hc >> 1][hc & 1][r], S[hc >> 1][hc & 1][r + 8], x[r], x[r + 8], w[r % NB][hc].x, w[r % NB][hc].y);
            __builtin_amdgcn_sched_barrier(0);
          }
      };
      int32_t v[kRegs];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int u = 0; u < kRegs; ++u) S[h][c][u] = 0.0;
      // Workgroup b walks the 2 l rows of a step in its own order (the rows are independent; the sums are exact in any order): started
      // together, all workgroups otherwise pull the same key rows through the same L2 channels at the same moments. Mode 1 (digit
      // rotation + component order from b): N = 8192 516.5 -> 458.8 ms per 512 (+12.6 %); at N = 4096 digit rotation costs 8-10 %
      // (two workgroups per CU and 512 per launch lose more L2 locality than they gain), component order alone +0.4 %
      // (profiles/r03/h_general_ab_row_rotation_modes.txt). Modes: 0 none, 1 both, 2 digits, 3 components.
      {
        constexpr int kRot = LOGN >= 13 ? 1 : 3;
        // (round 4: the order taken from the XCD, blockIdx.x & 7, instead of the workgroup -- same rows at the same time inside an L2, different
        // rows in different XCDs -- measured: N = 4096 +-0, N = 8192 -3.7 % against mode 1; profiles/r04/x_ab_general_cohorts_and_xcd_rotation.txt)
        const int qrot = (kRot == 1 || kRot == 2) ? (int)(blockIdx.x % (unsigned)l) : 0;
        const int cfirst = kRot == 1 ? (int)((blockIdx.x / (unsigned)l) & 1u) : (kRot == 3 ? (int)(blockIdx.x & 1u) : 0);
#pragma unroll 1
        for (int cc = 0; cc < 2; ++cc) {
          const int comp = cc ^ cfirst;
          prep(comp, v);
#pragma unroll 1
          for (int qi = 0; qi < l; ++qi) {
            int q = qi + qrot;
            if (q >= l) q -= l;
            row(comp, q, v);
          }
        }
      }

      // every thread passed at least one barrier since its reads of the accumulator: the update cannot overtake them
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        gen_fft_inv2<LOGN>(S[0][c], S[1][c], gen_local(t), a.tw, twn, s_re, s_im, sync, wsync, kept1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = t + T * (r & 7) + (r >> 3) * M;
          const uint32_t lo = (uint32_t)fft_round_torus32(S[0][c][r], dev);
          const uint32_t hi = (uint32_t)fft_round_torus32(S[1][c][r], dev);
          s_acc[c][j] = (int32_t)((uint32_t)s_acc[c][j] + lo + (hi << 16));
        }
      }
      sync();
    }

    // tLweExtractLweSampleIndex(index 0): a'[0] = acc_a[0], a'[j] = -acc_a[N-j], b' = acc_b[0]
    int32_t* out = a.u_out + ct * (N + 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = t + T * (r & 7) + (r >> 3) * M;
      out[j] = (j == 0) ? s_acc[0][0] : (int32_t)(0u - (uint32_t)s_acc[0][N - j]);
    }
    if (t == 0) out[N] = s_acc[1][0];
    sync();   // the accumulator is re-initialised by the next ciphertext
  }
  gen_publish(dev, a.dev_flag);
}

// out = a_small * b_torus (negacyclic, mod 2^32) through key split, forward, pointwise, inverse, recombination
template <int LOGN>
__global__ __launch_bounds__(Gen<LOGN>::T) void gen_polymul_kernel(const int32_t* __restrict__ a_small, const int32_t* __restrict__ b_torus,
                                                                    int32_t* __restrict__ out, double* __restrict__ scratch,
                                                                    const double* __restrict__ tw, long count, unsigned long long* dev_flag) {
  using G = Gen<LOGN>;
  constexpr int N = G::N, M = G::M, T = G::T;
  __shared__ double s_re[G::kPlane], s_im[G::kPlane];
  __shared__ double s_twn[kGenStageTw<LOGN> ? 2 * kGenTwLds : 2];
  const int t = threadIdx.x;
  auto sync = [] { gen_sync<T>(); };
  auto wsync = [] { gen_wave_sync(); };
  const double* twn = gen_stage_twiddles<LOGN>(s_twn, tw, t);
  double dev = 0.0;
  for (long idx = blockIdx.x; idx < count; idx += gridDim.x) {
    const int32_t* pa = a_small + idx * N;
    const int32_t* pb = b_torus + idx * N;
    double2* key = reinterpret_cast<double2*>(scratch) + (size_t)idx * 2 * M;   // the two halves, in the key layout
#pragma unroll 1
    for (int piece = 0; piece < 2; ++piece) {
      double x[kRegs];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int32_t lo, hi;
        gen_split_key(pb[t + T * (r & 7) + (r >> 3) * M], lo, hi);
        x[r] = (double)(piece ? hi : lo);
      }
      gen_fft_fwd<LOGN>(x, t, tw, twn, s_re, s_im, sync, wsync);
#pragma unroll
      for (int r = 0; r < 8; ++r) key[(size_t)piece * M + r * T + t] = make_double2(x[r] * (1.0 / M), x[r + 8] * (1.0 / M));
    }
    double xa[kRegs];
#pragma unroll
    for (int r = 0; r < 16; ++r) xa[r] = (double)pa[t + T * (r & 7) + (r >> 3) * M];
    gen_fft_fwd<LOGN>(xa, t, tw, twn, s_re, s_im, sync, wsync);
    double S[2][kRegs];
#pragma unroll
    for (int piece = 0; piece < 2; ++piece) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const double2 w = key[(size_t)piece * M + r * T + t];   // this thread's own stores
        S[piece][r] = 0.0; S[piece][r + 8] = 0.0;
        fft_cmac(S[piece][r], S[piece][r + 8], xa[r], xa[r + 8], w.x, w.y);
      }
    }
    gen_fft_inv<LOGN>(S[0], t, tw, twn, s_re, s_im, sync, wsync);
    gen_fft_inv<LOGN>(S[1], t, tw, twn, s_re, s_im, sync, wsync);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = t + T * (r & 7) + (r >> 3) * M;
      const uint32_t lo = (uint32_t)fft_round_torus32(S[0][r], dev);
      const uint32_t hi = (uint32_t)fft_round_torus32(S[1][r], dev);
      out[idx * N + j] = (int32_t)(lo + (hi << 16));
    }
    sync();
  }
  gen_publish(dev, dev_flag);
}

// TGSW rows of the bootstrapping key (rs_keygen_dev): row = i 2l + p, p = c l + j, written as (a, b) with b = a*S + e and the gadget
// term s_i 2^(32 - (j+1) Bgbit) on coefficient 0 of component c. A workgroup transforms S once; per row the T threads generate the
// mask in its own stream (thread t: ChaCha block t = words 16t .. 16t+15, i.e. the whole row) and the noise (blocks 4t .. 4t+3),
// exchange both through LDS into the transform layout, and form a*S by gen_polymul_kernel's split product with the roles swapped:
// the torus operand (the mask) is split into 16-bit halves, S is the small one. |half| <= 2^15 and S binary keep every half-product
// coefficient below N 2^15 -- far inside the products gen_error_bound covers (2l rows of Bg/2-digits times 2^15-halves) -- so
// rounding is exact; the distances are still published through dev_flag like every other general-ring product.
// a.compressed (rs_keygen_compressed_dev): the noise comes from the noise seed, the c = 0 gadget term enters the body as
// -s_i 2^(32 - (j+1) Bgbit) S instead of the mask, and only the body is written, to a.bk + row N.
template <int LOGN>
__global__ __launch_bounds__(Gen<LOGN>::T) void gen_keygen_bk_kernel(KeygenArgs a, const double* __restrict__ tw) {
  using G = Gen<LOGN>;
  constexpr int N = G::N, M = G::M, T = G::T;
  __shared__ double s_re[G::kPlane], s_im[G::kPlane];
  __shared__ double s_twn[kGenStageTw<LOGN> ? 2 * kGenTwLds : 2];
  __shared__ uint32_t s_mask[N], s_noise[N];
  const int t = threadIdx.x;
  auto sync = [] { gen_sync<T>(); };
  auto wsync = [] { gen_wave_sync(); };
  const double* twn = gen_stage_twiddles<LOGN>(s_twn, tw, t);
  uint32_t key[8], nkey[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { key[k] = a.seed[k]; nkey[k] = a.compressed ? a.noise_seed[k] : a.seed[k]; }
  const bool noisy = a.bk_sigma != 0.0;
  const bool compressed = a.compressed != 0;
  // S in the transform domain, scaled by 1/M (a power of two: exact); kept in registers for all rows of this workgroup
  double sx[kRegs];
  uint32_t sbits = 0;   // bit r = S[t + T r], the coefficients this thread writes (the compressed body's -gadget S term)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int32_t sr = a.tlwe_key[t + T * r];
    sx[r] = (double)sr;
    sbits |= (uint32_t)(sr & 1) << r;
  }
  gen_fft_fwd<LOGN>(sx, t, tw, twn, s_re, s_im, sync, wsync);
#pragma unroll
  for (int r = 0; r < 16; ++r) sx[r] *= 1.0 / M;
  double dev = 0.0;
  const long rows = (long)a.n * 2 * a.l;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int i = (int)(row / (2 * a.l)), p = (int)(row % (2 * a.l)), c = p / a.l, j = p % a.l;
    const uint32_t gadget = a.lwe_key[i] ? (1u << (32 - (j + 1) * a.bgbit)) : 0u;
    int32_t* pa = a.bk + (size_t)row * 2 * N;
    int32_t* pb = compressed ? a.bk + (size_t)row * N : pa + N;
    {
      uint32_t w[16];
      kg_bk_mask_block(key, (uint64_t)row, t, w);
#pragma unroll
      for (int k = 0; k < 16; ++k) s_mask[16 * t + k] = w[k];
      if (!compressed) {
        // the stored mask of a c = 0 row carries the gadget term on coefficient 0 (added after b is formed from the plain mask)
        const uint32_t w0 = w[0] + ((t == 0 && c == 0) ? gadget : 0u);
        int4* dst = reinterpret_cast<int4*>(pa) + 4 * t;
        dst[0] = make_int4((int)w0, (int)w[1], (int)w[2], (int)w[3]);
        dst[1] = make_int4((int)w[4], (int)w[5], (int)w[6], (int)w[7]);
        dst[2] = make_int4((int)w[8], (int)w[9], (int)w[10], (int)w[11]);
        dst[3] = make_int4((int)w[12], (int)w[13], (int)w[14], (int)w[15]);
      }
      if (noisy) {
#pragma unroll 1
        for (int g4 = 0; g4 < 4; ++g4) {
          kg_chacha_block(nkey, kKgBkNoise, (uint64_t)row, (uint32_t)(4 * t + g4), w);
#pragma unroll
          for (int q = 0; q < 4; ++q) s_noise[16 * t + 4 * g4 + q] = (uint32_t)kg_noise32(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3], a.bk_sigma);
        }
      }
    }
    sync();
    double S[2][kRegs];
#pragma unroll
    for (int piece = 0; piece < 2; ++piece) {   // unrolled: S indexed by a run-time piece would live in scratch
      double x[kRegs];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int32_t lo, hi;
        gen_split_key((int32_t)s_mask[t + T * r], lo, hi);
        x[r] = (double)(piece ? hi : lo);
      }
      gen_fft_fwd<LOGN>(x, gen_local(t), tw, twn, s_re, s_im, sync, wsync);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        S[piece][r] = 0.0; S[piece][r + 8] = 0.0;
        fft_cmac(S[piece][r], S[piece][r + 8], x[r], x[r + 8], sx[r], sx[r + 8]);
      }
    }
    // the two inverse transforms one after the other, the first one's rounded words replacing its 16 doubles before the second
    // runs: the register peak stays below the 256 VGPRs of a 512-thread workgroup at N = 8192 beside S's transform
    uint32_t b[kRegs];
    gen_fft_inv<LOGN>(S[0], gen_local(t), tw, twn, s_re, s_im, sync, wsync);
#pragma unroll
    for (int r = 0; r < 16; ++r) b[r] = (uint32_t)fft_round_torus32(S[0][r], dev);
    gen_fft_inv<LOGN>(S[1], gen_local(t), tw, twn, s_re, s_im, sync, wsync);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jj = t + T * r;
      b[r] += ((uint32_t)fft_round_torus32(S[1][r], dev) << 16) + ((jj == 0 && c == 1) ? gadget : 0u);
      if (compressed && c == 0 && ((sbits >> r) & 1u)) b[r] -= gadget;
      if (noisy) b[r] += s_noise[jj];
      pb[jj] = (int32_t)b[r];
    }
    sync();   // s_mask / s_noise are rewritten for the next row
  }
  gen_publish(dev, a.dev_flag);
}

// Keyswitching-key samples (rs_keygen_dev): one wave per sample s = (i t + j) 2^basebit + v, which is also its row in domains 5 / 6.
// Lane L generates block 64 m + L of the mask; the words pass through LDS so that the stores and the reads of the LWE key are
// coalesced, and a wave reduction gives sum a_k s_k mod 2^32. Samples with v = 0 are written as zeros.
// a.compressed (rs_keygen_compressed_dev): the noise comes from the noise seed and only the body is written, to a.ksk[s].
constexpr int kKgWaves = 4;
__global__ __launch_bounds__(64 * kKgWaves) void keygen_ksk_kernel(KeygenArgs a) {
  __shared__ uint32_t s_w[kKgWaves][kKgChunk];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t* buf = s_w[wv];
  uint32_t key[8], nkey[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { key[k] = a.seed[k]; nkey[k] = a.compressed ? a.noise_seed[k] : a.seed[k]; }
  const bool compressed = a.compressed != 0;
  const int base = 1 << a.basebit, W = a.n + 1;
  const long samples = (long)a.N * a.t * base;
  for (long s = (long)blockIdx.x * kKgWaves + wv; s < samples; s += (long)gridDim.x * kKgWaves) {
    int32_t* out = a.ksk + (size_t)s * W;
    const int v = (int)(s & (base - 1));
    if (v == 0) {
      if (compressed) { if (lane == 0) a.ksk[s] = 0; }
      else for (int k = lane; k < W; k += 64) out[k] = 0;
      continue;
    }
    const long ij = s >> a.basebit;
    const int i = (int)(ij / a.t), j = (int)(ij % a.t);
    uint32_t acc = 0;
    uint32_t w[16];
    for (int k0 = 0; k0 < a.n; k0 += kKgChunk) {
      kg_ksk_mask_block(key, (uint64_t)s, k0, lane, a.n, w);
      gen_wave_sync();   // this wave's reads of the previous chunk are done
#pragma unroll
      for (int q = 0; q < 16; ++q) buf[16 * lane + q] = w[q];
      gen_wave_sync();
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int idx = kg_ksk_chunk_word(q, lane), k = k0 + idx;
        if (k < a.n) {
          const uint32_t x = buf[idx];
          if (!compressed) out[k] = (int32_t)x;
          acc += a.lwe_key[k] ? x : 0u;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += (uint32_t)__shfl_xor((int)acc, off, 64);
    if (lane == 0) {
      uint32_t e = 0;
      if (a.ks_sigma != 0.0) {
        kg_chacha_block(nkey, kKgKsNoise, (uint64_t)s, 0u, w);
        e = (uint32_t)kg_noise32(w[0], w[1], w[2], w[3], a.ks_sigma);
      }
      const int32_t b = (int32_t)(acc + e + (((uint32_t)a.tlwe_key[i] * (uint32_t)v) << (32 - (j + 1) * a.basebit)));
      if (compressed) a.ksk[s] = b;
      else out[a.n] = b;
    }
  }
}

// Expansion of a compressed bk (rs_expand_keys_dev): a workgroup of T = N/16 threads per row, the grid striding over the n 2l rows.
// Thread t regenerates mask words 16 t .. 16 t + 15 (one ChaCha block, kg_bk_mask_block, the mapping of gen_keygen_bk_kernel) and
// stores them as four 16-byte writes; the body row is copied beside it with coalesced word loads and stores.
template <int LOGN>
__global__ __launch_bounds__((1 << LOGN) / 16) void expand_bk_kernel(ExpandArgs a) {
  constexpr int N = 1 << LOGN, T = N / 16;
  const int t = threadIdx.x;
  uint32_t key[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) key[k] = a.seed[k];
  const long rows = (long)a.n * 2 * a.l;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    int32_t* pa = a.bk + (size_t)row * 2 * N;
    const int32_t* src = a.bk_body + (size_t)row * N;
    int32_t body[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) body[r] = src[t + T * r];
    uint32_t w[16];
    kg_bk_mask_block(key, (uint64_t)row, t, w);
    int4* dst = reinterpret_cast<int4*>(pa) + 4 * t;
    dst[0] = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
    dst[1] = make_int4((int)w[4], (int)w[5], (int)w[6], (int)w[7]);
    dst[2] = make_int4((int)w[8], (int)w[9], (int)w[10], (int)w[11]);
    dst[3] = make_int4((int)w[12], (int)w[13], (int)w[14], (int)w[15]);
#pragma unroll
    for (int r = 0; r < 16; ++r) pa[N + t + T * r] = body[r];
  }
}

// Expansion of a compressed ksk (rs_expand_keys_dev): one wave per sample, keygen_ksk_kernel's chunking and LDS transpose
// (kg_ksk_mask_block, kg_ksk_chunk_word), so that the stores on the odd n + 1 stride are coalesced. v = 0 samples are all zero.
__global__ __launch_bounds__(64 * kKgWaves) void expand_ksk_kernel(ExpandArgs a) {
  __shared__ uint32_t s_w[kKgWaves][kKgChunk];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t* buf = s_w[wv];
  uint32_t key[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) key[k] = a.seed[k];
  const int base = 1 << a.basebit, W = a.n + 1;
  const long samples = (long)a.N * a.t * base;
  for (long s = (long)blockIdx.x * kKgWaves + wv; s < samples; s += (long)gridDim.x * kKgWaves) {
    int32_t* out = a.ksk + (size_t)s * W;
    if ((s & (base - 1)) == 0) {
      for (int k = lane; k < W; k += 64) out[k] = 0;
      continue;
    }
    uint32_t w[16];
    for (int k0 = 0; k0 < a.n; k0 += kKgChunk) {
      kg_ksk_mask_block(key, (uint64_t)s, k0, lane, a.n, w);
      gen_wave_sync();   // this wave's reads of the previous chunk are done
#pragma unroll
      for (int q = 0; q < 16; ++q) buf[16 * lane + q] = w[q];
      gen_wave_sync();
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int idx = kg_ksk_chunk_word(q, lane), k = k0 + idx;
        if (k < a.n) out[k] = (int32_t)buf[idx];
      }
    }
    if (lane == 0) out[a.n] = a.ksk_body[s];
  }
}

// ---- launchers ----
// persistent grid: as many workgroups as the device keeps resident (asked from the runtime once per kernel)
template <class K>
static long gen_resident(K kernel, int threads, int num_cus) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  return (long)per_cu * num_cus;
}
// resident workgroups of the CURRENT device (contexts of a fleet may sit on devices or partitions with different CU counts):
// cached per (device, ring), filled at first use; a benign race writes the same value twice
static long gen_grid(int logn, long work, int num_cus) {
  static std::atomic<long> resident[16][kGenMaxLogN + 1];
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::atomic<long>& slot = resident[dev & 15][logn];
  long r = slot.load(std::memory_order_relaxed);
  if (r == 0 || dev > 15) {
    const int T = (1 << logn) / 16;
    switch (logn) {
      case 10: r = gen_resident(gen_blind_rotate_kernel<10>, T, num_cus); break;
      case 11: r = gen_resident(gen_blind_rotate_kernel<11>, T, num_cus); break;
      case 12: r = gen_resident(gen_blind_rotate_kernel<12>, T, num_cus); break;
      default: r = gen_resident(gen_blind_rotate_kernel<13>, T, num_cus); break;
    }
    if (dev <= 15) slot.store(r, std::memory_order_relaxed);
  }
  return work < r ? work : r;
}
long gen_resident_ciphertexts(int logn, int num_cus) { return gen_grid(logn, 1L << 40, num_cus); }

hipError_t launch_gen_blind_rotate(int logn, const GenArgs& a, int num_cus, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const dim3 grid((unsigned)gen_grid(logn, a.B, num_cus)), block((1u << logn) / 16);
  switch (logn) {
    case 10: hipLaunchKernelGGL((gen_blind_rotate_kernel<10>), grid, block, 0, st, a); break;
    case 11: hipLaunchKernelGGL((gen_blind_rotate_kernel<11>), grid, block, 0, st, a); break;
    case 12: hipLaunchKernelGGL((gen_blind_rotate_kernel<12>), grid, block, 0, st, a); break;
    case 13: hipLaunchKernelGGL((gen_blind_rotate_kernel<13>), grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_gen_bk_transform(int logn, const int32_t* bk, double* bk_x, const double* tw, long n_polys, int num_cus, hipStream_t st) {
  if (n_polys <= 0) return hipSuccess;
  const dim3 grid((unsigned)std::min<long>(n_polys, 8L * num_cus)), block((1u << logn) / 16);
  switch (logn) {
    case 10: hipLaunchKernelGGL((gen_bk_transform_kernel<10>), grid, block, 0, st, bk, bk_x, tw, n_polys); break;
    case 11: hipLaunchKernelGGL((gen_bk_transform_kernel<11>), grid, block, 0, st, bk, bk_x, tw, n_polys); break;
    case 12: hipLaunchKernelGGL((gen_bk_transform_kernel<12>), grid, block, 0, st, bk, bk_x, tw, n_polys); break;
    case 13: hipLaunchKernelGGL((gen_bk_transform_kernel<13>), grid, block, 0, st, bk, bk_x, tw, n_polys); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_gen_polymul(int logn, const int32_t* a_small, const int32_t* b_torus, int32_t* out, double* scratch, const double* tw,
                              long count, unsigned long long* dev_flag, int num_cus, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const dim3 grid((unsigned)gen_grid(logn, count, num_cus)), block((1u << logn) / 16);
  switch (logn) {
    case 10: hipLaunchKernelGGL((gen_polymul_kernel<10>), grid, block, 0, st, a_small, b_torus, out, scratch, tw, count, dev_flag); break;
    case 11: hipLaunchKernelGGL((gen_polymul_kernel<11>), grid, block, 0, st, a_small, b_torus, out, scratch, tw, count, dev_flag); break;
    case 12: hipLaunchKernelGGL((gen_polymul_kernel<12>), grid, block, 0, st, a_small, b_torus, out, scratch, tw, count, dev_flag); break;
    case 13: hipLaunchKernelGGL((gen_polymul_kernel<13>), grid, block, 0, st, a_small, b_torus, out, scratch, tw, count, dev_flag); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_keygen_bk(int logn, const KeygenArgs& a, const double* tw, int num_cus, hipStream_t st) {
  const long rows = (long)a.n * 2 * a.l;
  if (rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)gen_grid(logn, rows, num_cus)), block((1u << logn) / 16);
  switch (logn) {
    case 10: hipLaunchKernelGGL((gen_keygen_bk_kernel<10>), grid, block, 0, st, a, tw); break;
    case 11: hipLaunchKernelGGL((gen_keygen_bk_kernel<11>), grid, block, 0, st, a, tw); break;
    case 12: hipLaunchKernelGGL((gen_keygen_bk_kernel<12>), grid, block, 0, st, a, tw); break;
    case 13: hipLaunchKernelGGL((gen_keygen_bk_kernel<13>), grid, block, 0, st, a, tw); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_keygen_ksk(const KeygenArgs& a, int num_cus, hipStream_t st) {
  const long samples = (long)a.N * a.t * (1L << a.basebit);
  if (samples <= 0) return hipSuccess;
  const long blocks = std::min<long>((samples + kKgWaves - 1) / kKgWaves, 16L * num_cus);
  hipLaunchKernelGGL(keygen_ksk_kernel, dim3((unsigned)blocks), dim3(64 * kKgWaves), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_expand_bk(int logn, const ExpandArgs& a, int num_cus, hipStream_t st) {
  const long rows = (long)a.n * 2 * a.l;
  if (rows <= 0) return hipSuccess;
  // 16 workgroups of one to eight waves per CU: enough stores in flight to hide the write latency
  const dim3 grid((unsigned)std::min<long>(rows, 16L * num_cus)), block((1u << logn) / 16);
  switch (logn) {
    case 10: hipLaunchKernelGGL((expand_bk_kernel<10>), grid, block, 0, st, a); break;
    case 11: hipLaunchKernelGGL((expand_bk_kernel<11>), grid, block, 0, st, a); break;
    case 12: hipLaunchKernelGGL((expand_bk_kernel<12>), grid, block, 0, st, a); break;
    case 13: hipLaunchKernelGGL((expand_bk_kernel<13>), grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_expand_ksk(const ExpandArgs& a, int num_cus, hipStream_t st) {
  const long samples = (long)a.N * a.t * (1L << a.basebit);
  if (samples <= 0) return hipSuccess;
  const long blocks = std::min<long>((samples + kKgWaves - 1) / kKgWaves, 16L * num_cus);
  hipLaunchKernelGGL(expand_ksk_kernel, dim3((unsigned)blocks), dim3(64 * kKgWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
