// rs_bootstrap_split.hip -- the blind-rotation kernels on the SPLIT key (RS_MODE_FFT_SPLIT, N = 1024; key layout: rs_general.h)
// that want LLVM's post-RA scheduler on and the max-memory-clause strategy (redsec_amd/build.py, HIP_OBJECTS):
//
//   blind_rotate_wgs_kernel    lock-step workgroup form, throughput batch sizes
//   blind_rotate_coops_kernel  cooperative form, G waves per ciphertext (latency batch sizes)
//
// The split duo form (blind_rotate_duos_kernel) is built with rs_bootstrap.hip and launched through launch_split_duos.
#include "rs_bootstrap.h"

namespace rs {

// -------------------------------------------------------------------------------------------------
// Blind rotation, lock-step workgroup form on the SPLIT key (RS_MODE_FFT_SPLIT at throughput batch sizes, N = 1024).
// Same structure as blind_rotate_wg_kernel -- 8 waves walk 8 ciphertexts in lock step and share the key through LDS --
// but every key row comes as two 16 KB half-rows (the low and the high 16-bit half of the key, rs_general.h), each
// multiplied into its own pair of column sums: four inverse transforms per CMUX step instead of two, and the result
// acc += round(lo) + (round(hi) << 16) is exact by the a-priori bound of rs_general.h (no certificate).
// Four accumulators leave registers for ONE digit transform in flight (the unsplit kernel pairs them); the inverse
// transforms still run as software-pipelined pairs. LDS: 3 ring slots of 16 KB (the accumulators and exchange planes
// of 8 ciphertexts leave room for no more), so `bara` lives in a 64-step window refilled from global memory.
// Half-row h sits in slot h mod 3 and is requested two half-rows ahead: the barrier that publishes h also says every
// wave has finished h - 1, whose slot then takes h + 2.
// -------------------------------------------------------------------------------------------------
template <class C, int WPB>
__global__ __launch_bounds__(64 * WPB) void blind_rotate_wgs_kernel(BlindRotateArgs a) {
  using Xf = XfFft<C>;
  static_assert(WPB == 8 || WPB == 4, "a 16 KB half-row is fetched as 16 / WPB one-KB chunks per wave");
  constexpr int kChunks = 16 / WPB;
  constexpr int KPL = 2 * C::L;
  constexpr int kSlotDoubles = 2 * kN;   // one key half-row: 2 columns x N doubles = 16 KB
  constexpr int kWin = 64;
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ __attribute__((aligned(16))) double s_buf[WPB][Xf::kWgBufDoubles];
  __shared__ int32_t s_acc[WPB][2][kN];
  __shared__ __attribute__((aligned(16))) double s_key[3][kSlotDoubles];
  __shared__ uint16_t s_bara[WPB][kWin];
  __shared__ int s_mail[kCohortSlots];   // XCD cohorts: the progress row requested a step ago (wave 0 only; rs_cohort.h)
  stage_tables(s_tw, a.tw, 64 * WPB, Xf::kTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  double* buf = s_buf[wave];
  int32_t* acc0 = s_acc[wave][0];
  int32_t* acc1 = s_acc[wave][1];
  typename Xf::State tw;
  Xf::init(tw, lane, s_tw, a.tw);
  FftTwKept<9> tw_kept;
  fft_kept_load(tw_kept, tw);
  const int n = a.n;
  const long n_groups = (a.B + WPB - 1) / WPB;
  const int total_half = n * KPL * 2;   // half-rows of one blind rotation (n <= 1024 steps x 4 l: far inside an int; scalar compares)
  const unsigned lane_off = (unsigned)lane * 16u;
  auto sync_w = [] { wave_lds_sync(); };
  RS_WGS_STAMP_DECL;   // -DRS_DIAG=2 (tools/stamp_profile.py --split): 0 step prologue + rotated differences, 1 digits + forward transform,
                       // 2 key wait + barrier (low half), 3 multiply-accumulate low, 4 key wait + barrier (high half), 5 multiply-accumulate high,
                       // 6 two inverse pairs + update, 7 group prologue / extract
  int steps_done = 0;   // CMUX steps of the groups this workgroup has finished (XCD cohorts, rs_cohort.h)

  for (long group = blockIdx.x; group < n_groups; group += gridDim.x, steps_done += n) {
    const long ct = group * WPB + wave;
    const bool active = ct < a.B;
    const int32_t* row0 = a.in0 + (active ? ct : 0) * a.W;
    const int32_t* row1 = a.in1 ? a.in1 + (active ? ct : 0) * a.W : nullptr;
    auto word = [&](int i) -> int32_t {
      uint32_t v = (uint32_t)a.c0 * (uint32_t)row0[i];
      if (row1) v += (uint32_t)a.c1 * (uint32_t)row1[i];
      return (int32_t)v;
    };
    auto fill_window = [&](int i0) {   // bara of steps [i0, i0 + 64): only this wave reads its row
      const int i = i0 + lane;
      s_bara[wave][lane] = (active && i < n) ? (uint16_t)modswitch_2N(word(i)) : (uint16_t)0;
    };
    if (active) {
      const int32_t barb = modswitch_2N((int32_t)((uint32_t)word(n) + (uint32_t)a.bconst));
      const int rot = 2 * kN - barb;  // in (0, 2N]
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        acc0[j] = 0;
        acc1[j] = test_vector(a, ct, j, rot);
      }
    }
    fill_window(0);
    // every wave has left the previous group's last multiply-accumulate before the ring is refilled
    __syncthreads();
    int h_issue = 0;         // next half-row to request
    int slot_issue = 0;      // its slot, h_issue mod 3
    const double* src_next = a.bk_x + (size_t)(wave * kChunks) * 128;   // this wave's share of the next half-row
    const unsigned key_lds = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)&s_key[0][0]) +
                             (unsigned)(wave * kChunks) * 1024u;
    auto issue_next = [&]() {
      if (h_issue < total_half) {
        // half-rows are requested in storage order: a running pointer and the slot's byte address, seven scalar instructions
        // instead of the twenty-two of the general form (a 64-bit index compare, a shift-and-add pair, a pointer cast)
        glds_chunks_at<kChunks>(src_next, lane_off, key_lds + (unsigned)slot_issue * (unsigned)(kSlotDoubles * sizeof(double)));
        src_next += kSlotDoubles;
        if constexpr (diag::kNoKeyProbe) {   // diagnostic builds: every step reads the half-rows of step 0 (they stay in the L2s)
          if ((h_issue + 1) % (2 * KPL) == 0) src_next -= (size_t)(2 * KPL) * kSlotDoubles;
        }
        ++h_issue;
        slot_issue = slot_issue == 2 ? 0 : slot_issue + 1;
      }
    };
    issue_next();
    issue_next();
    int h = 0;               // half-row consumed next
    int slot = 0;
    // publishes half-row h (every wave first waits for its own share: at most the next half-row's two loads may still
    // be in flight) and frees the slot of h - 1 for h + 2
    // (a bare s_barrier behind explicit counts: __syncthreads() would drain every outstanding load, i.e. also the
    // half-row requested one barrier ago, and with it half of the prefetch distance)
    auto publish = [&]() {
      if (h + 1 < total_half) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(kChunks) : "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      issue_next();
    };
    auto consumed = [&]() { ++h; slot = slot == 2 ? 0 : slot + 1; };

    RS_WGS_STAMP(7);
    for (int i = 0; i < n; ++i) {
      if ((i & (kWin - 1)) == 0 && i > 0) { wave_lds_sync(); fill_window(i); }
      if (wave == 0) cohort_step<BlindRotateArgs>(steps_done + i, s_mail);
      wave_lds_sync();
      const int32_t bara = __builtin_amdgcn_readfirstlane((int)s_bara[wave][i & (kWin - 1)]);
      const bool work = bara != 0;   // tfhe_blindRotate_FFT skips the identity CMUX (the barriers still run)
      double sl0[kRegs], sl1[kRegs], sh0[kRegs], sh1[kRegs];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) { sl0[u] = 0.0; sl1[u] = 0.0; sh0[u] = 0.0; sh1[u] = 0.0; }
      int32_t d[kRegs];
      auto load_d = [&](auto comp_c) {
        const int32_t* accc = decltype(comp_c)::value ? acc1 : acc0;
#pragma unroll
        for (int r = 0; r < kRegs; ++r) d[r] = gadget_prepare<C>(rotated_diff(accc, lane + 64 * r, bara));
      };
      auto row = [&](int q) {
        double x[kRegs];
        if (work) {
          Xf::digits(x, d, q);
          ffwd_planar(lane, x, tw_kept, buf, sync_w);
        }
        RS_WGS_STAMP(1);
        publish();
        RS_WGS_STAMP(2);
        if (work) mac_half_stream(sl0, sl1, x, s_key[slot], lane);
        consumed();
        RS_WGS_STAMP(3);
        publish();
        RS_WGS_STAMP(4);
        if (work) mac_half_stream(sh0, sh1, x, s_key[slot], lane);
        consumed();
        RS_WGS_STAMP(5);
      };
      // (the forward transforms stay single: run as software-pipelined pairs -- two transforms beside the four 32-register column
      // sums -- the kernel does not fit 256 registers: 1,040 bytes of scratch per lane, compiled in round 4 and dropped)
      if (work) load_d(std::false_type{});
      RS_WGS_STAMP(0);
#pragma unroll 1
      for (int q = 0; q < C::L; ++q) row(q);
      if (work) load_d(std::true_type{});
      RS_WGS_STAMP(0);
#pragma unroll 1
      for (int q = 0; q < C::L; ++q) row(q);

      if (work) {
        Xf::inverse_pair_wg(lane, sl0, sl1, tw, buf);
        uint32_t lo0[kRegs], lo1[kRegs];
#pragma unroll
        for (int r = 0; r < kRegs; ++r) { lo0[r] = (uint32_t)f_to_torus32(sl0[r]); lo1[r] = (uint32_t)f_to_torus32(sl1[r]); }
        Xf::inverse_pair_wg(lane, sh0, sh1, tw, buf);
#pragma unroll
        for (int r = 0; r < kRegs; ++r) {
          const int j = lane + 64 * r;
          acc0[j] = (int32_t)((uint32_t)acc0[j] + lo0[r] + ((uint32_t)f_to_torus32(sh0[r]) << 16));
          acc1[j] = (int32_t)((uint32_t)acc1[j] + lo1[r] + ((uint32_t)f_to_torus32(sh1[r]) << 16));
        }
        wave_lds_sync();
      }
      RS_WGS_STAMP(6);
    }

    if (active) {
      // tLweExtractLweSampleIndex(index 0): a'[0] = acc_a[0], a'[j] = -acc_a[N-j], b' = acc_b[0]
      int32_t* out = a.u_out + ct * (kN + 1);
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        out[j] = (j == 0) ? acc0[0] : (int32_t)(0u - (uint32_t)acc0[kN - j]);
      }
      if (lane == 0) out[kN] = acc1[0];
    }
  }
  RS_WGS_STAMP(7);
  RS_WGS_STAMP_FLUSH(wave);
  if (wave == 0) cohort_leave<BlindRotateArgs>(steps_done);
}

// -------------------------------------------------------------------------------------------------
// Cooperative blind rotation on the SPLIT key (RS_MODE_FFT_SPLIT at latency batch sizes, B <= 2 x #CUs, N = 1024): G waves
// share ONE ciphertext as in blind_rotate_coop_kernel. Wave g transforms the digit rows [g R, (g+1) R) and multiplies each
// into FOUR partial sums (low / high key half x two columns; sum index = 2 half + column); every sum has one owner wave
// that keeps its own partial in registers, adds the other waves' partials from LDS and runs the inverse transform:
//   G = 4: wave s owns sum s; the rounded low and high results of a column meet in the accumulator by LDS integer
//          atomics (exact, order-independent);
//   G = 2: wave w owns both halves of column w -- its two inverse transforms run as a software-pipelined pair.
// Key half-rows stream from L2 into registers in four chunks per row (the first one requested across the transform).
// -------------------------------------------------------------------------------------------------
template <class C, int G>
__global__ __launch_bounds__(64 * G) void blind_rotate_coops_kernel(BlindRotateArgs a) {
  using Xf = XfFft<C>;
  constexpr int KPL = 2 * C::L;
  constexpr int R = KPL / G;
  static_assert((G == 2 || G == 4) && KPL % G == 0, "waves split the digit rows evenly within a component");
  constexpr int OWN = 4 / G;                  // sums per owner wave
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ __attribute__((aligned(16))) double s_buf[G][kBufDoubles];
  __shared__ double s_part[G][4 - OWN][kN];   // the sums a wave does NOT own (G = 4: 96 KB, G = 2: 32 KB)
  __shared__ int32_t s_acc[2][kN];
  stage_tables(s_tw, a.tw, 64 * G, Xf::kTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long ct = blockIdx.x;
  const Field f = a.f;
  double* buf = s_buf[wave];
  typename Xf::State tw;
  Xf::init(tw, lane, s_tw, a.tw);
  const int32_t* row0 = a.in0 + ct * a.W;
  const int32_t* row1 = a.in1 ? a.in1 + ct * a.W : nullptr;
  const int n = a.n;
  const int comp = wave / (G / 2);
  const int row_begin = wave * R;
  auto word = [&](int i) -> int32_t {
    uint32_t v = (uint32_t)a.c0 * (uint32_t)row0[i];
    if (row1) v += (uint32_t)a.c1 * (uint32_t)row1[i];
    return (int32_t)v;
  };
  auto owner = [](int sum) { return coops_owner<G>(sum); };              // placement: rs_lds_plan.h (checked on the host)
  auto slot = [](int sum, int g) { return coops_slot<G>(sum, g); };      // index among the sums wave g does not own
  if (wave < 2) {
    const int32_t barb = modswitch_2N((int32_t)((uint32_t)word(n) + (uint32_t)a.bconst));
    const int rot = 2 * kN - barb;
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
      const int j = lane + 64 * r;
      s_acc[wave][j] = wave == 0 ? 0 : test_vector(a, ct, j, rot);
    }
  }
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const int32_t bara = __builtin_amdgcn_readfirstlane(modswitch_2N(word(i)));
    if (bara == 0) continue;   // uniform over the workgroup
    double s[4][kRegs];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int u = 0; u < kRegs; ++u) s[k][u] = 0.0;
    int32_t d[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; ++r) d[r] = gadget_prepare<C>(rotated_diff(s_acc[comp], lane + 64 * r, bara));
#pragma unroll 1
    for (int rr = 0; rr < R; ++rr) {
      const int row = row_begin + (int)((rr + blockIdx.x) % R);
      const int q = row - comp * C::L;
      // half-row (row, half) = [column 0: N doubles][column 1: N doubles], pairs (re, im) of position 8 lane + v at [v][lane]
      const double2* lo0 = reinterpret_cast<const double2*>(a.bk_x + ((size_t)i * KPL + row) * 4 * kN);
      const double2* lo1 = lo0 + kN / 2;
      const double2* hi0 = lo0 + kN;
      const double2* hi1 = hi0 + kN / 2;
      auto load4 = [&](const double2* k0, const double2* k1, int v0, double2 (&w0)[4], double2 (&w1)[4]) {
#pragma unroll
        for (int v = 0; v < 4; ++v) { w0[v] = k0[(v0 + v) * 64 + lane]; w1[v] = k1[(v0 + v) * 64 + lane]; }
      };
      double x[kRegs];
      double2 wa0[4], wa1[4], wb0[4], wb1[4], wc0[4], wc1[4], wd0[4], wd1[4];
      load4(lo0, lo1, 0, wa0, wa1);
      load4(lo0, lo1, 4, wb0, wb1);
      load4(hi0, hi1, 0, wc0, wc1);
      load4(hi0, hi1, 4, wd0, wd1);
      Xf::fwd_digits(lane, x, d, q, 0u, tw, buf, f);
      Xf::mac(s[0], s[1], x, wa0, wa1, 0, f);
      Xf::mac(s[0], s[1], x, wb0, wb1, 4, f);
      Xf::mac(s[2], s[3], x, wc0, wc1, 0, f);
      Xf::mac(s[2], s[3], x, wd0, wd1, 4, f);
    }
    // partial sums a wave does not own go through LDS (position u*64 + lane is conflict-free)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (owner(k) != wave) {
        double* dst = s_part[wave][slot(k, wave)];
#pragma unroll
        for (int u = 0; u < kRegs; ++u) dst[u * 64 + lane] = s[k][u];
      }
    }
    __syncthreads();   // partials visible; every wave has finished reading the accumulator
    if constexpr (G == 4) {
      double x[kRegs];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (wave == k) {
#pragma unroll
          for (int u = 0; u < kRegs; ++u) x[u] = s[k][u];
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (g != wave) {
          const double* src = s_part[g][slot(wave, g)];
#pragma unroll
          for (int u = 0; u < kRegs; ++u) x[u] += src[u * 64 + lane];
        }
      }
      Xf::inverse(lane, x, tw, buf, f);
      const int sh = wave >= 2 ? 16 : 0;
      int32_t* acc = s_acc[wave & 1];
#pragma unroll
      for (int r = 0; r < kRegs; ++r) atomicAdd(reinterpret_cast<unsigned*>(acc) + lane + 64 * r, (uint32_t)f_to_torus32(x[r]) << sh);
    } else {
      double xa[kRegs], xb[kRegs];
      if (wave == 0) {
#pragma unroll
        for (int u = 0; u < kRegs; ++u) { xa[u] = s[0][u]; xb[u] = s[2][u]; }
      } else {
#pragma unroll
        for (int u = 0; u < kRegs; ++u) { xa[u] = s[1][u]; xb[u] = s[3][u]; }
      }
      const double* pa = s_part[1 - wave][0];
      const double* pb = s_part[1 - wave][1];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) { xa[u] += pa[u * 64 + lane]; xb[u] += pb[u * 64 + lane]; }
      Xf::inverse2(lane, xa, xb, tw, buf, f);
      int32_t* acc = s_acc[wave];
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        acc[j] = (int32_t)((uint32_t)acc[j] + (uint32_t)f_to_torus32(xa[r]) + ((uint32_t)f_to_torus32(xb[r]) << 16));
      }
    }
    __syncthreads();   // accumulator updated
  }
  int32_t* out = a.u_out + ct * (kN + 1);
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
      const int j = lane + 64 * r;
      out[j] = (j == 0) ? s_acc[0][0] : (int32_t)(0u - (uint32_t)s_acc[0][kN - j]);
    }
    if (lane == 0) out[kN] = s_acc[1][0];
  }
}

// (An eight-wave form of this kernel -- blind_rotate_coops8_kernel, round 4: rows over 8 waves as in blind_rotate_coop8_kernel, the
// four sums met by LDS f64 atomics -- was built, bit-exact, and is SLOWER: 4.90 / 6.93 ms against 4.08 ms for 196 sign bootstraps
// (profiles/r04/i_ab_coop8_atomics_and_coops8.txt). Four 32-register sums beside a transform leave a wave of a two-wave SIMD (256
// registers) no room to keep a key row in flight across the transform, which is what the four-wave form's 412 registers buy. Removed.)

// -------------------------------------------------------------------------------------------------
// Launcher
// -------------------------------------------------------------------------------------------------
// Split-key workgroup form (N = 1024; cfg 0 / 1 = the two shipped gadgets, 2 = redsec_params_small's l=3 Bgbit=10): a.bk_x = the split key of rs_general.h,
// a.tw = the FFT tables of rs_fft.h. Returns hipErrorNotSupported for an unknown gadget id (caller: general kernel).
// The plan's one step (rs_launch_plan.h: the split forms have no cut-off last round) -> its kernel instantiation.
template <class C>
static hipError_t launch_split(int cfg, const BlindRotateArgs& whole, int num_cus, const LaunchOpts& o, hipStream_t st, LaunchInfo* info) {
  const LaunchPlan plan = plan_blind_rotate(form_traits<XfFft<C>>(true), whole.n, whole.B, num_cus, o, whole.progress != nullptr);
  const LaunchStep& s = plan.step[0];
  BlindRotateArgs a = step_args(whole, s);
  if (hipError_t e = cohort_setup(a, whole.progress, s, st); e != hipSuccess) return e;
  auto run = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)s.grid), dim3((unsigned)s.block), 0, st, a); };
  switch (plan_key(s.form, s.waves)) {
    case plan_key(kFormSplitCoop, 4):
      if constexpr ((2 * C::L) % 4 == 0) { run(blind_rotate_coops_kernel<C, 4>); break; }
      return hipErrorInvalidValue;
    case plan_key(kFormSplitCoop, 2): run(blind_rotate_coops_kernel<C, 2>); break;
    case plan_key(kFormSplitDuo, 8):   // built with rs_bootstrap.hip
      if (hipError_t e = launch_split_duos(cfg, a, s.grid, st); e != hipSuccess) return e;
      break;
    // (8 before 4: the order of instantiation is worth an instruction in each of these kernels; tools/codeobj_digest.py)
    case plan_key(kFormSplitWorkgroup, 8): run(blind_rotate_wgs_kernel<C, 8>); break;
    case plan_key(kFormSplitWorkgroup, 4): run(blind_rotate_wgs_kernel<C, 4>); break;
    default: return hipErrorInvalidValue;
  }
  if (info) *info = plan.info;
  return hipGetLastError();
}

hipError_t launch_blind_rotate_split_wg(int cfg, const BlindRotateArgs& a, int num_cus, const LaunchOpts& o, hipStream_t st, LaunchInfo* info) {
  if (cfg == 0) return launch_split<CfgDefault128>(cfg, a, num_cus, o, st, info);
  if (cfg == 1) return launch_split<CfgRedsecV2>(cfg, a, num_cus, o, st, info);
  if (cfg == 2) return launch_split<CfgRedsecSmall>(cfg, a, num_cus, o, st, info);
  return hipErrorNotSupported;
}

}  // namespace rs

#if RS_STAMPS_ON(2)   // blind_rotate_wgs_kernel
RS_DEFINE_STAMPS()
#endif
