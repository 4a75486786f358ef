// rs_bootstrap.hip -- the transform-based kernels of the gate bootstrap, written once over a
// "transform policy" (rs_bootstrap.h: XfNtt<Cfg> exact NTT, XfFft<Cfg> FP64 FFT with a run-time certificate):
//
//   bk_transform_kernel       bootstrapping key -> transform domain (the bkFFT analogue; once per key)
//   blind_rotate_kernel       gate pre-combination + modswitch + n CMUX steps + sample extract
//                             (tfhe_bootstrap_woKS_FFT; REDsec: lib/BinOps_enc.cpp:185,191), throughput form
//   blind_rotate_coop_kernel  the same with G waves per ciphertext (latency form for small batches)
//   polymul_kernel            debug/parity tap through the same transform path
//
// One wavefront owns one ciphertext for the whole blind rotation: its TRLWE accumulator (2 x 1024
// int32) lives in LDS, each of the (k+1) l digit polynomials is transformed in registers with two
// LDS transposes, multiplied against the coalesced-streamed key row and accumulated in registers,
// and two inverse transforms update the accumulator. Waves never synchronise with each other after
// the twiddle tables are staged.
//
// This unit holds the FFT / exact-NTT kernels and the split duo form, which are built with LLVM's post-RA scheduler off; the
// split lock-step and cooperative kernels (rs_bootstrap_split.hip) and the listed coop8 kernel (rs_bootstrap_listed.hip) are
// objects of their own -- redsec_amd/build.py (HIP_OBJECTS) gives the measured reasons. The one compile-time switch is RS_DIAG
// (rs_diag.h: phase stamps and the no-key timing probe of diagnostic builds). Every experiment of rounds 1-4 that was measured
// and not adopted has its verdict in MEASUREMENTS.md and no code path here.
#include "rs_bootstrap.h"

namespace rs {

// -------------------------------------------------------------------------------------------------
// Key transform: one wavefront per key polynomial. Output layout per polynomial: [v 0..7][lane][2]
// doubles in the exact register order of the consuming wavefront, so the blind rotation reads each
// row with eight perfectly coalesced 16-byte-per-lane loads.
// -------------------------------------------------------------------------------------------------
template <class Xf, int WPB>
__global__ __launch_bounds__(64 * WPB) void bk_transform_kernel(const int32_t* __restrict__ bk, double* __restrict__ bk_x,
                                                                 const double* __restrict__ tw_g, Field f, double scale, long n_polys) {
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ double s_buf[WPB][kBufDoubles];
  stage_tables(s_tw, tw_g, 64 * WPB, Xf::kTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long poly = (long)blockIdx.x * WPB + wave;
  if (poly >= n_polys) return;
  typename Xf::State st;
  Xf::init(st, lane, s_tw, tw_g);
  double x[kRegs];
  const int32_t* src = bk + poly * kN;
#pragma unroll
  for (int r = 0; r < kRegs; ++r) x[r] = (double)src[lane + 64 * r];
  Xf::fwd_generic(lane, x, st, s_buf[wave], f);
  Xf::key_store(reinterpret_cast<double2*>(bk_x + poly * kN), lane, x, scale, f);
}

// -------------------------------------------------------------------------------------------------
// Blind rotation + sample extract, throughput form (persistent waves).
// -------------------------------------------------------------------------------------------------
template <class Xf, int WPB>
__global__ __launch_bounds__(64 * WPB) void blind_rotate_kernel(BlindRotateArgs a) {
  using C = typename Xf::Cfg;
  if (recompute_not_needed(a)) return;
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ double s_buf[WPB][kBufDoubles];
  __shared__ int32_t s_acc[WPB][2][kN];
  stage_tables(s_tw, a.tw, 64 * WPB, Xf::kTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  // Persistent waves: the first ciphertext is assigned statically, further ones are pulled from a
  // device counter (zeroed by the launcher on the same stream). A 150 KB-LDS workgroup cannot be
  // replaced until its LAST wave exits, and waves sharing a SIMD finish up to 20 % apart (issue
  // arbitration favours the older wave), which left 18 % of the wave slots idle with one ciphertext
  // per wave. Every wave leaves the loop as soon as the counter passes B, so the grid always drains.
  long ct = (long)blockIdx.x * WPB + wave;
  const long first_dynamic = (long)gridDim.x * WPB;
  if (ct >= a.B) return;

  const Field f = a.f;
  double* buf = s_buf[wave];
  int32_t* acc0 = s_acc[wave][0];
  int32_t* acc1 = s_acc[wave][1];
  typename Xf::State tw;
  Xf::init(tw, lane, s_tw, a.tw);
  const int n = a.n;
  constexpr uint32_t offset = gadget_offset<C>();
  constexpr int KPL = 2 * C::L;
  double dev = 0.0;

  for (;;) {
    const int32_t* row0 = a.in0 + ct * a.W;
    const int32_t* row1 = a.in1 ? a.in1 + ct * a.W : nullptr;
    // gate pre-combination (0, bconst) + c0*in0 + c1*in1, evaluated word by word as it is consumed
    auto word = [&](int i) -> int32_t {
      uint32_t v = (uint32_t)a.c0 * (uint32_t)row0[i];
      if (row1) v += (uint32_t)a.c1 * (uint32_t)row1[i];
      return (int32_t)v;
    };
    {
      const int32_t barb = modswitch_2N((int32_t)((uint32_t)word(n) + (uint32_t)a.bconst));
      const int rot = 2 * kN - barb;  // in (0, 2N]
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        acc0[j] = 0;
        acc1[j] = test_vector(a, ct, j, rot);
      }
    }
    wave_lds_sync();

    for (int i = 0; i < n; ++i) {
      const int32_t bara = __builtin_amdgcn_readfirstlane(modswitch_2N(word(i)));
      if (bara == 0) continue;  // tfhe_blindRotate_FFT skips the identity CMUX
      double s0[kRegs], s1[kRegs];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) { s0[u] = 0.0; s1[u] = 0.0; }
      const double* bk_i = a.bk_x + (size_t)i * KPL * 2 * kN;

#pragma unroll 1
      for (int comp = 0; comp < 2; ++comp) {
        const int32_t* accc = comp ? acc1 : acc0;
        int32_t d[kRegs];
#pragma unroll
        for (int r = 0; r < kRegs; ++r) {
          d[r] = rotated_diff(accc, lane + 64 * r, bara);
          if (Xf::kPreparedDigits) d[r] = gadget_prepare<C>(d[r]);
        }
#pragma unroll 1
        for (int q = 0; q < C::L; ++q) {
          const int row = comp * C::L + q;
          const double2* bp0 = reinterpret_cast<const double2*>(bk_i + (size_t)(row * 2) * kN);
          const double2* bp1 = bp0 + kN / 2;
          double x[kRegs];
          if constexpr (Xf::kSplitKeyLoads) {
            // first half of the key row prefetched across the transform, second half fetched after it
            double2 wa0[4], wa1[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) { wa0[v] = bp0[v * 64 + lane]; wa1[v] = bp1[v * 64 + lane]; }
            Xf::fwd_digits(lane, x, d, q, offset, tw, buf, f);
            double2 wb0[4], wb1[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) { wb0[v] = bp0[(v + 4) * 64 + lane]; wb1[v] = bp1[(v + 4) * 64 + lane]; }
            Xf::mac(s0, s1, x, wa0, wa1, 0, f);
            Xf::mac(s0, s1, x, wb0, wb1, 4, f);
          } else {
            double2 w0[8], w1[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) { w0[v] = bp0[v * 64 + lane]; w1[v] = bp1[v * 64 + lane]; }
            Xf::fwd_digits(lane, x, d, q, offset, tw, buf, f);
            Xf::mac8(s0, s1, x, w0, w1, f);
          }
        }
        if (comp == 0) Xf::mid(s0, s1, f);
      }

      Xf::inverse2(lane, s0, s1, tw, buf, f);
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        acc0[j] = (int32_t)((uint32_t)acc0[j] + (uint32_t)Xf::to_torus(s0[r], dev));
        acc1[j] = (int32_t)((uint32_t)acc1[j] + (uint32_t)Xf::to_torus(s1[r], dev));
      }
      wave_lds_sync();
    }

    // tLweExtractLweSampleIndex(index 0): a'[0] = acc_a[0], a'[j] = -acc_a[N-j], b' = acc_b[0]
    int32_t* out = a.u_out + ct * (kN + 1);
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
      const int j = lane + 64 * r;
      out[j] = (j == 0) ? acc0[0] : (int32_t)(0u - (uint32_t)acc0[kN - j]);
    }
    if (lane == 0) out[kN] = acc1[0];

    if (!a.counter) break;
    unsigned int nxt = 0;
    if (lane == 0) nxt = atomicAdd(a.counter, 1u);
    nxt = (unsigned int)__builtin_amdgcn_readfirstlane((int)nxt);
    ct = first_dynamic + (long)nxt;
    if (ct >= a.B) break;
    wave_lds_sync();
  }
  if (Xf::kCertificate) publish_certificate(dev, a.dev_flag, lane);
}

// -------------------------------------------------------------------------------------------------
// Blind rotation, workgroup lock-step form (large batches). The per-wave kernel above makes EVERY
// wavefront stream the whole transformed key by itself: at 150k bootstraps/s that is ~9.6 TB/s of
// L2 -> CU reads with a 64 % L2 miss rate (waves drift apart, so a key row is rarely still in L2 for
// the next wave), and both parameter sets stall at that same byte rate. Here the WPB waves of a
// workgroup walk the CMUX chain of WPB different ciphertexts in lock step and share each key row
// through LDS: every wave fetches 1/WPB of the row with direct global->LDS loads (no VGPRs), one
// workgroup barrier per row publishes it, and the multiply-accumulate reads it with 16-byte LDS
// reads. Rows go in pairs through a two-slot ring (see the loop) -- two barriers per pair.
// Every wave executes every barrier: inactive waves (ragged last group) and identity CMUX steps
// (bara == 0) only skip the arithmetic. Groups are assigned round-robin: all groups take the same
// number of steps, so there is nothing to balance dynamically.
// -------------------------------------------------------------------------------------------------
template <class Xf, int WPB>
__global__ __launch_bounds__(64 * WPB) void blind_rotate_wg_kernel(BlindRotateArgs a) {
  using C = typename Xf::Cfg;
  constexpr int KPL = 2 * C::L;
  constexpr int kRowDoubles = 2 * kN;             // one key row: 2 columns x N doubles = 16 KB
  constexpr int kChunks = kRowDoubles / 128;      // 1 KB pieces = one wave-wide 16-byte load each
  constexpr int kChunksPerWave = kChunks / WPB;
  static_assert(kChunks % WPB == 0 && (kChunksPerWave == 1 || kChunksPerWave == 2 || kChunksPerWave == 4), "waves must split a key row evenly");
  __shared__ double s_tw[Xf::kWgTableDoubles + 1];
  __shared__ __attribute__((aligned(16))) double s_buf[WPB][Xf::kWgBufDoubles];
  __shared__ int32_t s_acc[WPB][2][kN];
  __shared__ __attribute__((aligned(16))) double s_key[2][kRowDoubles];
  constexpr int kWin = 64;                       // mask words live in a 64-step window, as in the split kernel
  __shared__ uint16_t s_bara[WPB][kWin];
  __shared__ int s_mail[kCohortSlots];   // XCD cohorts: the progress row requested a step ago (wave 0 only; rs_cohort.h)
  stage_tables(s_tw, a.tw, 64 * WPB, Xf::kWgTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const Field f = a.f;
  double* buf = s_buf[wave];
  int32_t* acc0 = s_acc[wave][0];
  int32_t* acc1 = s_acc[wave][1];
  typename Xf::State tw_table;
  Xf::init(tw_table, lane, s_tw, a.tw);
  FftTwKept<3> tw;   // all eight per-lane twiddles stay in registers for the whole kernel (32 registers; +2.4 % / +1.3 %, profiles/r03/n_*)
  fft_kept_load(tw, tw_table);
  const int n = a.n;
  constexpr uint32_t offset = gadget_offset<C>();
  double dev = 0.0;
  const long n_groups = (a.B + WPB - 1) / WPB;
  const int total_rows = n * KPL;   // key rows of one blind rotation (n <= 1024 steps x 2 l: far inside an int; scalar compares)
  RS_STAMP_DECL;   // -DRS_DIAG=1 (tools/stamp_profile.py): 0 step prologue, 1 digits + forward pair, 2 wait for the key rows + barrier, 3 multiply-
                   // accumulate, 4 barrier + next rows requested, 5 accumulator pre-read + inverse pair, 6 rounding + accumulator update, 7 group prologue / extract
  const unsigned lane_off = (unsigned)lane * 16u;   // my 1/WPB share of a key row: chunks of 1 KB, 16 bytes per lane

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
    fill_window(0);
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
    // all global reads of this prologue are complete and every wave has left the previous group's
    // last multiply-accumulate before the ring is refilled
    __syncthreads();
    // the pairs are requested in storage order, row R into slot 0 and R + 1 into slot 1: a running pointer and two fixed LDS
    // byte addresses instead of a 64-bit row index, its compare, a multiply-add and a generic-pointer cast per row (the same
    // change took the split lock-step kernel from 137 k to 145 k/s, profiles/r04/az_*)
    const double* src_next = a.bk_x + (size_t)(wave * kChunksPerWave) * 128;
    const unsigned key_lds = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)&s_key[0][0]) +
                             (unsigned)(wave * kChunksPerWave) * 1024u;
    auto issue_pair = [&] {
      glds_chunks_at<kChunksPerWave>(src_next, lane_off, key_lds);
      glds_chunks_at<kChunksPerWave>(src_next + kRowDoubles, lane_off, key_lds + (unsigned)(kRowDoubles * sizeof(double)));
      src_next += 2 * kRowDoubles;
    };
    issue_pair();
    RS_STAMP(7);

    // Rows are processed in PAIRS (R, R+1), the two digit transforms interleaved phase by phase.
    // Barrier 1 of a pair publishes both rows (each wave first waits for its own shares); barrier 2
    // says every wave has finished reading them, after which the next pair's loads are issued and
    // have the whole next transform pair to land.
    int R = 0;
    unsigned bara_next = s_bara[wave][0];   // read one step ahead: its LDS latency is not exposed
    for (int i = 0; i < n; ++i) {
      // XCD cohorts (cohort_step above): with l = 10 a step reads 320 KB of key per CU and an XCD's L2 keeps 12 steps; launches of the REDsec
      // set were seen at twice the 8-XCD floor of fabric traffic (60.8 GB, profiles/r04/pmc) when workgroups drifted further apart
      if (wave == 0) cohort_step<BlindRotateArgs>(steps_done + i, s_mail);
      const int32_t bara = __builtin_amdgcn_readfirstlane((int)bara_next);
      if (((i + 1) & (kWin - 1)) == 0 && i + 1 < n) { wave_lds_sync(); fill_window(i + 1); wave_lds_sync(); }
      bara_next = (i + 1 < n) ? s_bara[wave][(i + 1) & (kWin - 1)] : 0;
      const bool work = bara != 0;   // tfhe_blindRotate_FFT skips the identity CMUX
      double s0[kRegs], s1[kRegs];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) { s0[u] = 0.0; s1[u] = 0.0; }
      int32_t d[kRegs];
      RS_STAMP(0);

      // d holds the PREPARED rotated difference of one component (gadget offset added and field sign bits
      // flipped once per component, not per digit row). Written as straight-line code with a
      // compile-time component: inside the rolled pair loop (run-time component) the compiler issued
      // its 32 LDS reads one at a time, each followed by a full wait.
      auto load_d = [&](auto comp_c) {
        const int32_t* accc = decltype(comp_c)::value ? acc1 : acc0;
#pragma unroll
        for (int r = 0; r < kRegs; ++r) d[r] = gadget_prepare<C>(rotated_diff(accc, lane + 64 * r, bara));
      };
      auto pair = [&](int compA, int qA, int compB, int qB) {
        double xa[kRegs], xb[kRegs];
        if (work) {
          if constexpr (C::L % 2 != 0) {
            if (qA == 0) { if (compA) load_d(std::true_type{}); else load_d(std::false_type{}); }
          }
          Xf::digits(xa, d, qA);
          if constexpr (C::L % 2 != 0) {
            if (qB == 0) { if (compB) load_d(std::true_type{}); else load_d(std::false_type{}); }
          }
          Xf::digits(xb, d, qB);
          Xf::fwd_pair_wg(lane, xa, xb, tw, buf);
        }
        RS_STAMP(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        RS_STAMP(2);
        if (work) {
          mac_pair_stream(s0, s1, xa, xb, s_key[0], s_key[1], lane);
        }
        RS_STAMP(3);
        __syncthreads();
        R += 2;
        if (R < total_rows) issue_pair();
        RS_STAMP(4);
      };
      if constexpr (C::L % 2 == 0) {
        if (work) load_d(std::false_type{});
#pragma unroll 1
        for (int q = 0; q < C::L; q += 2) pair(0, q, 0, q + 1);
        if (work) { Xf::mid(s0, s1, f); load_d(std::true_type{}); }
#pragma unroll 1
        for (int q = 0; q < C::L; q += 2) pair(1, q, 1, q + 1);
      } else {
        // odd l: the middle pair straddles the two accumulator components (no place for Xf::mid:
        // the workgroup form is only instantiated for policies whose mid() is empty)
#pragma unroll
        for (int p = 0; p < C::L; ++p) {
          const int rA = 2 * p, rB = 2 * p + 1;
          pair(rA / C::L, rA % C::L, rB / C::L, rB % C::L);
        }
      }

      if (work) {
        // the accumulator words are read BEFORE the inverse pair (the digit transforms are dead, there
        // are registers to spare): read after it, every read-modify-write of the update exposed an LDS
        // round trip behind the store in front of it
        uint32_t a0[kRegs], a1[kRegs];
#pragma unroll
        for (int r = 0; r < kRegs; ++r) { a0[r] = (uint32_t)acc0[lane + 64 * r]; a1[r] = (uint32_t)acc1[lane + 64 * r]; }
        wave_lds_sync();
        Xf::inverse_pair_wg(lane, s0, s1, tw, buf);
        RS_STAMP(5);
#pragma unroll
        for (int r = 0; r < kRegs; ++r) {
          const int j = lane + 64 * r;
          acc0[j] = (int32_t)(a0[r] + (uint32_t)Xf::to_torus(s0[r], dev));
          acc1[j] = (int32_t)(a1[r] + (uint32_t)Xf::to_torus(s1[r], dev));
        }
        wave_lds_sync();
        RS_STAMP(6);
      }
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
    RS_STAMP(7);
  }
  RS_STAMP_FLUSH(wave);
  if (wave == 0) cohort_leave<BlindRotateArgs>(steps_done);
  if (Xf::kCertificate) publish_certificate(dev, a.dev_flag, lane);
}

// -------------------------------------------------------------------------------------------------
// Blind rotation, "duo" form on the SPLIT key (RS_MODE_FFT_SPLIT, 2 x #CUs < B <= 4 x #CUs, N = 1024, any l): a workgroup
// is 4 ciphertexts x 2 waves, as in blind_rotate_duo_kernel -- wave (c, h) owns accumulator component h of ciphertext c. It
// transforms the l digit rows of that component (one transform in flight: the four partial sums low / high half x two columns
// fill 128 registers, as in blind_rotate_wgs_kernel) and multiplies each into all four sums; then it hands the two partials of
// column 1 - h to its partner, adds the partner's partials of column h to its own, runs the two inverse transforms of column h
// (low and high half) as one software-pipelined pair and updates component h: acc += round(lo) + (round(hi) << 16).
// Against the 4-wave lock-step groups that served this batch range (one wave per ciphertext, one wave per SIMD) a wave does
// half the transforms of a CMUX step and the second wave slot of every SIMD is in use.
// Key: the 8 waves run in lock step; per (digit row q, key half) a PAIR of 16 KB half-rows -- the one of component 0 and the
// one of component 1 -- is fetched by direct global->LDS loads, 4 one-KB chunks per wave, into pair slot p & 1 (p numbers the
// pairs in the order they are consumed). The barrier that publishes pair p also says every wave has finished pair p - 1, whose
// slot then takes pair p + 1 (an L2-resident half-row lands within one multiply-accumulate phase: measured on the wgs
// kernel). The partials change hands through the same 64 KB once the last pair of a step has been consumed, low halves first,
// then high halves (8 waves x 8 KB each time), so the first pair of the next step is requested behind that exchange; it has
// the inverse transforms, the rotated difference and a forward transform to arrive. Barriers per CMUX step: 2 l + 4.
// -------------------------------------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(512) void blind_rotate_duos_kernel(BlindRotateArgs a) {
  using Xf = XfFft<C>;
  constexpr int KPL = 2 * C::L;
  constexpr int kSlotDoubles = 2 * kN;   // one key half-row: 2 columns x N doubles = 16 KB
  constexpr int kCts = 4;
  constexpr int kWin = 64;
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ __attribute__((aligned(16))) double s_buf[8][Xf::kWgBufDoubles];
  __shared__ int32_t s_acc[kCts][2][kN];
  __shared__ __attribute__((aligned(16))) double s_key[4][kSlotDoubles];   // slot 2 (p & 1) + component
  __shared__ uint16_t s_bara[8][kWin];                                      // one window per wave (the two waves of a ciphertext fill the same values)
  stage_tables(s_tw, a.tw, 512, Xf::kTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int c = wave >> 1, h = wave & 1;
  double* buf = s_buf[wave];
  int32_t* acc = s_acc[c][h];
  typename Xf::State tw;
  Xf::init(tw, lane, s_tw, a.tw);
  const int n = a.n;
  const long n_groups = (a.B + kCts - 1) / kCts;
  const int total_pairs = n * C::L * 2;   // 32-bit counters: scalar compares (see blind_rotate_wgs_kernel)
  const unsigned lane_off = (unsigned)lane * 16u;
  auto sync_w = [] { wave_lds_sync(); };
  // own += x * column h, given += x * column 1 - h of the half-row in `slot`
  auto mac_cols = [&](double (&own)[kRegs], double (&given)[kRegs], const double (&x)[kRegs], const double* slot) {
    const double2* k = reinterpret_cast<const double2*>(slot);
    mac_half_stream_cols(own, given, x, k + h * (kN / 2), k + (1 - h) * (kN / 2), lane);
  };
  // pair p = (i L + k) 2 + half holds the half-rows ((i KPL + comp L + q_k) 2 + half) of comp = 0, 1, where q_k = (k + rot) mod L:
  // workgroup b walks the l digits of a step in the order rotated by b (the rows of a step are independent), so that the 256
  // workgroups of a launch do not pull the same half-rows through the same L2 channels at the same moments (600 sign
  // bootstraps 12.06 -> 11.25 ms, profiles/r03/v_ab_*). This wave fetches chunks [4 (wave & 3), +4) of component wave >> 2.
  const int rot = (int)(blockIdx.x % C::L);
  const int kcomp = duos_fetch_comp(wave);                                 // placement: rs_lds_plan.h (checked on the host)
  const size_t chunk_off = (size_t)duos_first_chunk(wave) * 128;
  const unsigned key_lds = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)&s_key[0][0]) + (unsigned)chunk_off * 8u;
  int issued;
  int iss_i, iss_k;   // step and position (digit slot, half) of the next pair to request
  auto issue_reset = [&] { issued = 0; iss_i = 0; iss_k = 0; };
  auto issue_next = [&] {
    if (issued >= total_pairs) return;
    int q = (iss_k >> 1) + rot;
    if (q >= C::L) q -= C::L;
    // the half-row's byte offset fits 32 bits (at most n * 4 l half-rows of 16 KB: 229 MB for the REDsec set); the slot as an LDS byte address
    const unsigned hrow = (unsigned)(((iss_i * KPL + kcomp * C::L + q) << 1) + (iss_k & 1));
    glds_chunks_at<4>(reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.bk_x) + (size_t)(hrow * (unsigned)(kSlotDoubles * sizeof(double)))) + chunk_off, lane_off,
                      key_lds + (unsigned)duos_pair_slot(issued, kcomp) * (unsigned)(kSlotDoubles * sizeof(double)));
    ++issued;
    if (++iss_k == 2 * C::L) { iss_k = 0; ++iss_i; }
  };

  for (long group = blockIdx.x; group < n_groups; group += gridDim.x) {
    const long ct = group * kCts + c;
    const bool active = ct < a.B;
    const int32_t* row0 = a.in0 + (active ? ct : 0) * a.W;
    const int32_t* row1 = a.in1 ? a.in1 + (active ? ct : 0) * a.W : nullptr;
    auto word = [&](int i) -> int32_t {
      uint32_t v = (uint32_t)a.c0 * (uint32_t)row0[i];
      if (row1) v += (uint32_t)a.c1 * (uint32_t)row1[i];
      return (int32_t)v;
    };
    auto fill_window = [&](int i0) {   // bara of steps [i0, i0 + 64): read back by this wave only
      const int i = i0 + lane;
      s_bara[wave][lane] = (active && i < n) ? (uint16_t)modswitch_2N(word(i)) : (uint16_t)0;
    };
    if (active) {
      const int32_t barb = modswitch_2N((int32_t)((uint32_t)word(n) + (uint32_t)a.bconst));
      const int rot = 2 * kN - barb;  // in (0, 2N]
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        acc[j] = h ? test_vector(a, ct, j, rot) : 0;
      }
    }
    fill_window(0);
    __syncthreads();   // every wave has left the previous group's last exchange and extract before the key buffer is refilled
    int p = 0;         // pair consumed next; it has been requested, pair p + 1 has not
    issue_reset();
    issue_next();
    // publishes pair p (every wave first waits for its own share; nothing else of this wave is in flight) and requests pair
    // p + 1 into the other slot unless the step's exchange needs the buffer first (`hold`)
    auto publish = [&](bool hold) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (!hold) issue_next();
    };

    for (int i = 0; i < n; ++i) {
      if ((i & (kWin - 1)) == 0 && i > 0) { wave_lds_sync(); fill_window(i); }
      wave_lds_sync();
      const int32_t bara = __builtin_amdgcn_readfirstlane((int)s_bara[wave][i & (kWin - 1)]);
      const bool work = bara != 0;   // tfhe_blindRotate_FFT skips the identity CMUX (the barriers still run)
      // partial sums of the column this wave inverts (own = column h) and of the one its partner inverts, low / high key half
      double lo[kRegs], hi[kRegs], glo[kRegs], ghi[kRegs];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) { lo[u] = 0.0; hi[u] = 0.0; glo[u] = 0.0; ghi[u] = 0.0; }
      int32_t d[kRegs];
      if (work) {
#pragma unroll
        for (int r = 0; r < kRegs; ++r) d[r] = gadget_prepare<C>(rotated_diff(acc, lane + 64 * r, bara));
      }
#pragma unroll 1
      for (int q = 0; q < C::L; ++q) {
        double x[kRegs];
        if (work) {
          int qd = q + rot;
          if (qd >= C::L) qd -= C::L;
          Xf::digits(x, d, qd);
          ffwd_planar(lane, x, tw, buf, sync_w);
        }
        publish(false);
        if (work) mac_cols(lo, glo, x, s_key[duos_pair_slot(p, h)]);
        ++p;
        publish(q + 1 == C::L);
        if (work) mac_cols(hi, ghi, x, s_key[duos_pair_slot(p, h)]);
        ++p;
      }
      // partial exchange through the key buffer (64 KB = 8 waves x 8 KB), low halves, then high halves: wave (c, h) hands over
      // its partials of column 1 - h and adds its partner's partials of column h to its own
      double* mine_xchg = &s_key[0][0] + duo_xchg_doubles(wave);
      const double* theirs = &s_key[0][0] + duo_xchg_doubles(duo_partner(wave));
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every wave has consumed the last pair
      if (work) {
#pragma unroll
        for (int u = 0; u < kRegs; ++u) mine_xchg[u * 64 + lane] = glo[u];
      }
      __syncthreads();
      if (work) {
#pragma unroll
        for (int u = 0; u < kRegs; ++u) lo[u] += theirs[u * 64 + lane];
      }
      __syncthreads();
      if (work) {
#pragma unroll
        for (int u = 0; u < kRegs; ++u) mine_xchg[u * 64 + lane] = ghi[u];
      }
      __syncthreads();
      if (work) {
#pragma unroll
        for (int u = 0; u < kRegs; ++u) hi[u] += theirs[u * 64 + lane];
      }
      __syncthreads();                             // partials consumed: the key buffer may be refilled
      issue_next();
      if (work) {
        uint32_t a0[kRegs];   // accumulator words read ahead of the inverse transforms (see the workgroup kernel)
#pragma unroll
        for (int r = 0; r < kRegs; ++r) a0[r] = (uint32_t)acc[lane + 64 * r];
        wave_lds_sync();
        Xf::inverse_pair_wg(lane, lo, hi, tw, buf);
#pragma unroll
        for (int r = 0; r < kRegs; ++r)
          acc[lane + 64 * r] = (int32_t)(a0[r] + (uint32_t)f_to_torus32(lo[r]) + ((uint32_t)f_to_torus32(hi[r]) << 16));
        wave_lds_sync();
      }
    }

    if (active) {
      // tLweExtractLweSampleIndex(index 0): a'[0] = acc_a[0], a'[j] = -acc_a[N-j], b' = acc_b[0]
      int32_t* out = a.u_out + ct * (kN + 1);
      if (h == 0) {
#pragma unroll
        for (int r = 0; r < kRegs; ++r) {
          const int j = lane + 64 * r;
          out[j] = (j == 0) ? acc[0] : (int32_t)(0u - (uint32_t)acc[kN - j]);
        }
      } else if (lane == 0) {
        out[kN] = acc[0];
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------
// Blind rotation, "duo" workgroup form (mid-size batches: 2 x #CUs < B < 8 x #CUs, even l).
// One wave per ciphertext leaves half the wave slots empty there and every wave streams the whole key
// by itself (the 1,024-neuron MNIST layer was bound by ~10 TB/s of key reads). Here a workgroup is
// 4 ciphertexts x 2 waves: wave (c, h) owns accumulator component h of ciphertext c -- it transforms
// the l digit rows of that component (in software-pipelined pairs), accumulates partial sums for both
// output columns, receives column h's other partial from its partner, runs that column's inverse
// transform and updates component h. The 8 waves run in lock step and share the key rows through LDS:
// per pair of rows a "quad" (2 rows of each component, 64 KB) is fetched by direct global->LDS loads,
// 1/8 per wave. Barriers per CMUX step: 2 per row pair + 2 around the partial exchange, which goes
// through the (then idle) quad buffer.
// -------------------------------------------------------------------------------------------------
template <class Xf>
__global__ __launch_bounds__(512) void blind_rotate_duo_kernel(BlindRotateArgs a) {
  using C = typename Xf::Cfg;
  static_assert(C::L % 2 == 0, "rows are processed in pairs within one component");
  constexpr int KPL = 2 * C::L;
  constexpr int kRowDoubles = 2 * kN;
  constexpr int kCts = 4;
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ __attribute__((aligned(16))) double s_buf[8][Xf::kWgBufDoubles];
  __shared__ int32_t s_acc[kCts][2][kN];
  __shared__ __attribute__((aligned(16))) double s_key[4][kRowDoubles];   // slot 2 h + k: row k of the pair, component h
  __shared__ uint16_t s_bara[kCts][kSmall];
  stage_tables(s_tw, a.tw, 512, Xf::kTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int c = wave >> 1, h = wave & 1;
  const int own_col = h ? kN / 2 : 0, given_col = h ? 0 : kN / 2;   // offsets (double2) of the two columns within a key row
  const Field f = a.f;
  double* buf = s_buf[wave];
  int32_t* acc = s_acc[c][h];
  typename Xf::State tw;
  Xf::init(tw, lane, s_tw, a.tw);
  FftTwKept<6> tw_kept;
  fft_kept_load(tw_kept, tw);
  const int n = a.n;
  constexpr uint32_t offset = gadget_offset<C>();
  double dev = 0.0;
  const long n_groups = (a.B + kCts - 1) / kCts;
  RS_DUO_STAMP_DECL;   // -DRS_DIAG=4 (tools/stamp_coop8.py duo): 0 step prologue + rotated difference, 1 digits + forward pair,
                       // 2 key wait + barrier 1, 3 multiply-accumulate, 4 barrier 2 + next quad, 5 partial exchange (2 barriers), 6 inverse + update, 7 group prologue / extract

  const unsigned lane_off = (unsigned)lane * 16u;
  // (Row pairs walked in per-workgroup rotated orders, as in the split forms: no effect on the 1,024-neuron MNIST layer,
  // profiles/r03/v_ab_duo_row_rotation.txt -- every workgroup walks them in storage order.)
  // quad (i, p): rows i KPL + hh L + 2 p + k; this wave fetches half of slot (wave >> 1)
  auto issue_quad = [&](int i, int p) {
    const int slot = duo_quad_slot(wave), chunk0 = duo_quad_first_chunk(wave);   // placement: rs_lds_plan.h (checked on the host)
    const long R = (long)i * KPL + (slot >> 1) * C::L + 2 * p + (slot & 1);
    const double* src = a.bk_x + (size_t)R * kRowDoubles + (size_t)chunk0 * 128;
    double* dst = s_key[slot] + chunk0 * 128;
    glds_chunks<4>(src, lane_off, dst);
    glds_chunks<4>(src + 4 * 128, lane_off, dst + 4 * 128);
  };
  // (The eight 1 KB requests of a wave's share of the next quad spread over the six segments of the next forward pair instead of one burst
  // behind the barrier: 7.96 -> 9.97 ms at 1,024 ciphertexts, profiles/r04/aq_*: the rows arrive late and the asm statements cut the pair's schedule.)
  for (long group = blockIdx.x; group < n_groups; group += gridDim.x) {
    const long ct = group * kCts + c;
    const bool active = ct < a.B;
    if (active) {
      const int32_t* row0 = a.in0 + ct * a.W;
      const int32_t* row1 = a.in1 ? a.in1 + ct * a.W : nullptr;
      auto word = [&](int i) -> int32_t {
        uint32_t v = (uint32_t)a.c0 * (uint32_t)row0[i];
        if (row1) v += (uint32_t)a.c1 * (uint32_t)row1[i];
        return (int32_t)v;
      };
      for (int i = lane + 64 * h; i < n; i += 128) s_bara[c][i] = (uint16_t)modswitch_2N(word(i));
      const int32_t barb = modswitch_2N((int32_t)((uint32_t)word(n) + (uint32_t)a.bconst));
      const int rot = 2 * kN - barb;  // in (0, 2N]
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        acc[j] = h ? test_vector(a, ct, j, rot) : 0;
      }
    }
    __syncthreads();   // bara complete; previous group's last reads of the quad buffer are over
    issue_quad(0, 0);
    RS_DUO_STAMP(7);

    unsigned bara_next = active ? s_bara[c][0] : 0;   // read one step ahead
    for (int i = 0; i < n; ++i) {
      const int32_t bara = __builtin_amdgcn_readfirstlane((int)bara_next);
      bara_next = (active && i + 1 < n) ? s_bara[c][i + 1] : 0;
      const bool work = bara != 0;   // tfhe_blindRotate_FFT skips the identity CMUX
      // own: partial sum of the column this wave inverts (column h); given: of the column its partner inverts. Addressed through the
      // key-row offsets (own_col, given_col) instead of (column 0, column 1) selected by h afterwards: those selects were 310
      // v_cndmask per CMUX step (the compiler cannot know h at compile time)
      double own[kRegs], given[kRegs];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) { own[u] = 0.0; given[u] = 0.0; }
      int32_t d[kRegs];
      if (work) {
#pragma unroll
        for (int r = 0; r < kRegs; ++r) d[r] = gadget_prepare<C>(rotated_diff(acc, lane + 64 * r, bara));
      }
      RS_DUO_STAMP(0);
#pragma unroll 1
      for (int p = 0; p < C::L / 2; ++p) {
        double xa[kRegs], xb[kRegs];
        if (work) {
          Xf::digits(xa, d, 2 * p);
          Xf::digits(xb, d, 2 * p + 1);
          Xf::fwd_pair_wg(lane, xa, xb, tw_kept, buf);
        }
        RS_DUO_STAMP(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                         // quad (i, p) published
        RS_DUO_STAMP(2);
        if (work) {
          mac_pair_stream(own, given, xa, xb, s_key[2 * h], s_key[2 * h + 1], lane, own_col, given_col);
        }
        RS_DUO_STAMP(3);
        __syncthreads();                         // every wave has finished reading it
        if (p + 1 < C::L / 2) issue_quad(i, p + 1);
        RS_DUO_STAMP(4);
      }
      // partial exchange through the idle quad buffer: wave (c, h) hands over its partial of column 1 - h
      double* xchg = &s_key[0][0] + duo_xchg_doubles(wave);
      if (work) {
#pragma unroll
        for (int u = 0; u < kRegs; ++u) xchg[u * 64 + lane] = given[u];
      }
      __syncthreads();
      double (&mine)[kRegs] = own;
      if (work) {
        const double* theirs = &s_key[0][0] + duo_xchg_doubles(duo_partner(wave));
#pragma unroll
        for (int u = 0; u < kRegs; ++u) mine[u] += theirs[u * 64 + lane];
      }
      __syncthreads();                           // partials consumed: the quad buffer may be refilled
      if (i + 1 < n) issue_quad(i + 1, 0);
      RS_DUO_STAMP(5);
      if (work) {
        uint32_t a0[kRegs];   // accumulator words read ahead of the inverse transform (see the workgroup kernel)
#pragma unroll
        for (int r = 0; r < kRegs; ++r) a0[r] = (uint32_t)acc[lane + 64 * r];
        wave_lds_sync();
        Xf::inverse_wg(lane, mine, tw, buf, f);
#pragma unroll
        for (int r = 0; r < kRegs; ++r) acc[lane + 64 * r] = (int32_t)(a0[r] + (uint32_t)Xf::to_torus(mine[r], dev));
        wave_lds_sync();
      }
      RS_DUO_STAMP(6);
    }

    if (active) {
      // tLweExtractLweSampleIndex(index 0): a'[0] = acc_a[0], a'[j] = -acc_a[N-j], b' = acc_b[0]
      int32_t* out = a.u_out + ct * (kN + 1);
      if (h == 0) {
#pragma unroll
        for (int r = 0; r < kRegs; ++r) {
          const int j = lane + 64 * r;
          out[j] = (j == 0) ? acc[0] : (int32_t)(0u - (uint32_t)acc[kN - j]);
        }
      } else if (lane == 0) {
        out[kN] = acc[0];
      }
    }
  }
  RS_DUO_STAMP(7);
  RS_DUO_STAMP_FLUSH(wave);
  if (Xf::kCertificate) publish_certificate(dev, a.dev_flag, lane);
}

// -------------------------------------------------------------------------------------------------
// Cooperative blind rotation (latency form, B <= 2 x #CUs): G waves share ONE ciphertext.
// Wave g transforms the digit polynomials [g R, (g+1) R) (R = 2l / G, so each wave stays within one
// accumulator component) and accumulates its partial column sums; the partials meet in LDS, waves 0
// and 1 sum one column each, run the inverse transform and update the shared accumulator. Two
// workgroup barriers per CMUX step.
// -------------------------------------------------------------------------------------------------
template <class Xf, int G>
__global__ __launch_bounds__(64 * G) void blind_rotate_coop_kernel(BlindRotateArgs a) {
  using C = typename Xf::Cfg;
  if (recompute_not_needed(a)) return;
  constexpr int KPL = 2 * C::L;
  constexpr int R = KPL / G;
  static_assert(KPL % G == 0 && G % 2 == 0, "waves must split the digit rows evenly within a component");
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ double s_buf[G][kBufDoubles];
  __shared__ double s_part[G][2][kN];
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
  const int grp = wave;
  const int comp = grp / (G / 2);
  const int row_begin = grp * R;
  double dev = 0.0;
  auto word = [&](int i) -> int32_t {
    uint32_t v = (uint32_t)a.c0 * (uint32_t)row0[i];
    if (row1) v += (uint32_t)a.c1 * (uint32_t)row1[i];
    return (int32_t)v;
  };
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
  constexpr uint32_t offset = gadget_offset<C>();
  for (int i = 0; i < n; ++i) {
    const int32_t bara = __builtin_amdgcn_readfirstlane(modswitch_2N(word(i)));
    if (bara == 0) continue;   // uniform over the workgroup: every wave works on the same ciphertext
    double s0[kRegs], s1[kRegs];
#pragma unroll
    for (int u = 0; u < kRegs; ++u) { s0[u] = 0.0; s1[u] = 0.0; }
    const double* bk_i = a.bk_x + (size_t)diag::key_step(i) * KPL * 2 * kN;
    int32_t d[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
      d[r] = rotated_diff(s_acc[comp], lane + 64 * r, bara);
      if (Xf::kPreparedDigits) d[r] = gadget_prepare<C>(d[r]);
    }
#pragma unroll 1
    for (int rr = 0; rr < R; ++rr) {
      // workgroups walk their rows of a step in different orders (the rows of a step are independent), so that the whole chip
      // does not pull the same key rows through the same L2 channels at the same moments: the 196-neuron MNIST layer
      // 3.33 -> 3.15 ms (profiles/r03/v_ab_coop_row_rotation.txt)
      const int row = row_begin + (int)((rr + blockIdx.x) % R);
      const int q = row - comp * C::L;
      const double2* bp0 = reinterpret_cast<const double2*>(bk_i + (size_t)(row * 2) * kN);
      const double2* bp1 = bp0 + kN / 2;
      double x[kRegs];
      // the whole key row is requested across the transform (3.21 -> 3.01 ms once the rows were rotated, v_ab_coop_whole_row.txt)
      double2 w0[8], w1[8];
#pragma unroll
      for (int v = 0; v < 8; ++v) { w0[v] = bp0[v * 64 + lane]; w1[v] = bp1[v * 64 + lane]; }
      Xf::fwd_digits(lane, x, d, q, offset, tw, buf, f);
      Xf::mac8(s0, s1, x, w0, w1, f);
    }
    // partial sums exchanged through LDS: position u*64 + lane is conflict-free
#pragma unroll
    for (int u = 0; u < kRegs; ++u) {
      s_part[wave][0][u * 64 + lane] = Xf::partial(s0[u], f);
      s_part[wave][1][u * 64 + lane] = Xf::partial(s1[u], f);
    }
    __syncthreads();   // partials visible; every wave has finished reading the accumulator
    if (wave < 2) {
      double x[kRegs];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) {
        double t = s_part[0][wave][u * 64 + lane];
#pragma unroll
        for (int g = 1; g < G; ++g) t += s_part[g][wave][u * 64 + lane];
        x[u] = t;
      }
      Xf::inverse(lane, x, tw, buf, f);
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        s_acc[wave][j] = (int32_t)((uint32_t)s_acc[wave][j] + (uint32_t)Xf::to_torus(x[r], dev));
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
  if (Xf::kCertificate && wave < 2) publish_certificate(dev, a.dev_flag, lane);
}

// -------------------------------------------------------------------------------------------------
// Cooperative blind rotation, EIGHT waves per ciphertext (latency form for B <= #CUs, FFT mode; round 4).
// The four-wave form above runs one wave per SIMD: a lone wave issues its FP64 and LDS instructions one behind
// the other (78 % of a two-wave SIMD's rate per wave-slot), and its critical path per CMUX step is
// R = 2l/4 forward transforms plus one inverse. Here the 2l digit rows of a step go to 8 waves -- the components
// alternate (wave & 1), and of the four waves of a component the OLDER ones (waves 0-3, which win the issue
// arbitration against their SIMD partners 4-7) take the extra rows, so that every SIMD (waves s and s + 4) carries
// the same number of rows and finishes them together (l = 10: 3+2 on every SIMD; rs_lds_plan.h; round-4 phase stamps:
// with the extra rows on younger waves two SIMDs finished 1,100 cycles late, 196 ciphertexts 2.53 -> 2.43 ms) -- and the
// two inverse transforms to two waves with the fewest rows, on different SIMDs (waves 6 and 7). For l < 4 (six rows for
// eight waves) the first form's deal stays -- waves 0-3 component 0, waves 4-7 component 1, inverse transforms on the
// two waves without rows (3 and 4): measured faster there (2.66 against 2.73 ms).
// Partial column sums meet by LDS floating-point atomics (ds_add_f64, no return value) in s_sum[2][N]; after the barrier each
// inverse wave reads its 16 values, clears them for the next step, transforms and updates the accumulator (a first form parked
// the 14 partials in idle transform buffers and s_part slots: 2.92 ms where the atomics take 2.64, MEASUREMENTS.md R4). Integer
// results are independent of the summation order (the sums are rounded to the exact integers, certificate-tracked as
// everywhere); two workgroup barriers per step. LDS: 8 KB tables + 8 x 9 KB buffers + 16 KB sums + 8 KB accumulator = 104 KB.
// -------------------------------------------------------------------------------------------------
template <class Xf>
__global__ __launch_bounds__(512) void blind_rotate_coop8_kernel(BlindRotateArgs a) {
  using C = typename Xf::Cfg;
  static_assert(Xf::kCertificate, "FFT policy only: the exact-NTT reduction schedule is validated for four partials");
  if (recompute_not_needed(a)) return;
  constexpr int G = kCoop8Waves, L = C::L, KPL = 2 * L;
  constexpr int kInvA = coop8_inv_a(L), kInvB = coop8_inv_b(L);   // placement: rs_lds_plan.h (checked on the host)
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ double s_buf[G][kBufDoubles];
  __shared__ double s_sum[2][kN];   // the two column sums, added up by LDS floating-point atomics (zero between steps)
  __shared__ int32_t s_acc[2][kN];
  stage_tables(s_tw, a.tw, 64 * G, Xf::kTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long ct = blockIdx.x;
  const Field f = a.f;
  double* buf = s_buf[wave];
  for (int e = threadIdx.x; e < 2 * kN; e += 64 * G) (&s_sum[0][0])[e] = 0.0;
  typename Xf::State tw;
  Xf::init(tw, lane, s_tw, a.tw);
  const int32_t* row0 = a.in0 + ct * a.W;
  const int32_t* row1 = a.in1 ? a.in1 + ct * a.W : nullptr;
  const int n = a.n;
  // rows [first, first + cnt) of this wave's component (digit index q = first + rr, TGSW row comp * L + q)
  const int comp = coop8_comp(L, wave), cnt = coop8_row_count(L, wave), first = coop8_row_first(L, wave);
  [[maybe_unused]] const int r_first = cnt > 0 ? (int)(blockIdx.x % (unsigned)cnt) : 0;
  double dev = 0.0;
  RS_C8_STAMP_DECL;   // -DRS_DIAG=8 (tools/stamp_coop8.py): 0 mask word, 1 rotated difference, 2 rows (forward +
                      // multiply-accumulate), 3 atomics issued, 4 barrier 1, 5 inverse + accumulator update, 6 barrier 2, 7 prologue / extract
  auto word = [&](int i) -> int32_t {
    uint32_t v = (uint32_t)a.c0 * (uint32_t)row0[i];
    if (row1) v += (uint32_t)a.c1 * (uint32_t)row1[i];
    return (int32_t)v;
  };
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
  constexpr uint32_t offset = gadget_offset<C>();
  RS_C8_STAMP(7);
  for (int i = 0; i < n; ++i) {
    // (requesting the mask word of step i + 1 here, a step ahead, was measured: 2.43 -> 2.47 ms for 196 ciphertexts; the load hits the L1)
    const int32_t bara = __builtin_amdgcn_readfirstlane(modswitch_2N(word(i)));
    RS_C8_STAMP(0);
    if (bara == 0) continue;   // uniform over the workgroup
    double s0[kRegs], s1[kRegs];
#pragma unroll
    for (int u = 0; u < kRegs; ++u) { s0[u] = 0.0; s1[u] = 0.0; }
    if (cnt > 0) {
      const double* bk_i = a.bk_x + (size_t)diag::key_step(i) * KPL * 2 * kN;
      int32_t d[kRegs];
#pragma unroll
      for (int r = 0; r < kRegs; ++r) d[r] = gadget_prepare<C>(rotated_diff(s_acc[comp], lane + 64 * r, bara));
      RS_C8_STAMP(1);
      [[maybe_unused]] int r_run = r_first;   // rr = 0 starts at blockIdx.x mod cnt in every step
#pragma unroll 1
      for (int rr = 0; rr < cnt; ++rr) {
        const int q = first + r_run;                                       // per-workgroup row order, as in the four-wave form
        r_run = r_run + 1 == cnt ? 0 : r_run + 1;
        const double2* bp0 = reinterpret_cast<const double2*>(bk_i + (size_t)((comp * L + q) * 2) * kN);
        const double2* bp1 = bp0 + kN / 2;
        double x[kRegs];
        double2 w0[8], w1[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) { w0[v] = bp0[v * 64 + lane]; w1[v] = bp1[v * 64 + lane]; }
        Xf::fwd_digits(lane, x, d, q, offset, tw, buf, f);
        Xf::mac8(s0, s1, x, w0, w1, f);
      }
      RS_C8_STAMP(2);
    }
    // every wave adds its two partial sums into the column sums with ds_add_f64 (no return value: 32 instructions that overlap
    // the other waves' transforms); the order of the floating-point additions is free -- the sums are rounded to the exact
    // integers afterwards, with the certificate watching the distance as everywhere
    if (cnt > 0) {
#pragma unroll
      for (int u = 0; u < kRegs; ++u) { unsafeAtomicAdd(&s_sum[0][u * 64 + lane], s0[u]); unsafeAtomicAdd(&s_sum[1][u * 64 + lane], s1[u]); }
    }
    RS_C8_STAMP(3);
    __syncthreads();   // sums complete; every wave has finished reading the accumulator
    RS_C8_STAMP(4);
    if (wave == kInvA || wave == kInvB) {
      double* sum = s_sum[wave == kInvA ? 0 : 1];
      double x[kRegs];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) x[u] = sum[u * 64 + lane];
#pragma unroll
      for (int u = 0; u < kRegs; ++u) sum[u * 64 + lane] = 0.0;   // for the next step (same lane, same address: in order)
      Xf::inverse(lane, x, tw, buf, f);
      int32_t* acc = s_acc[wave == kInvA ? 0 : 1];
#pragma unroll
      for (int r = 0; r < kRegs; ++r) {
        const int j = lane + 64 * r;
        acc[j] = (int32_t)((uint32_t)acc[j] + (uint32_t)Xf::to_torus(x[r], dev));
      }
    }
    RS_C8_STAMP(5);
    __syncthreads();   // accumulator updated, sums zero
    RS_C8_STAMP(6);
    continue;
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
  RS_C8_STAMP(7);
  RS_C8_STAMP_FLUSH(wave);
  if (wave == kInvA || wave == kInvB) publish_certificate(dev, a.dev_flag, lane);
}

// -------------------------------------------------------------------------------------------------
// Debug tap: out = a_small * b_torus (negacyclic, mod 2^32) through forward/pointwise/inverse.
// -------------------------------------------------------------------------------------------------
template <class Xf, int WPB>
__global__ __launch_bounds__(64 * WPB) void polymul_kernel(const int32_t* __restrict__ a_small, const int32_t* __restrict__ b_torus,
                                                            int32_t* __restrict__ out, double* __restrict__ scratch,
                                                            const double* __restrict__ tw_g, Field f, double scale, long count,
                                                            unsigned long long* dev_flag) {
  __shared__ double s_tw[Xf::kTableDoubles + 1];
  __shared__ double s_buf[WPB][kBufDoubles];
  stage_tables(s_tw, tw_g, 64 * WPB, Xf::kTableDoubles);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long idx = (long)blockIdx.x * WPB + wave;
  if (idx >= count) return;
  double* buf = s_buf[wave];
  typename Xf::State st;
  Xf::init(st, lane, s_tw, tw_g);
  double xa[kRegs], xb[kRegs];
#pragma unroll
  for (int r = 0; r < kRegs; ++r) {
    xa[r] = (double)a_small[idx * kN + lane + 64 * r];
    xb[r] = (double)b_torus[idx * kN + lane + 64 * r];
  }
  // key side exactly as bk_transform_kernel: through global memory in the key layout
  Xf::fwd_generic(lane, xb, st, buf, f);
  double2* key = reinterpret_cast<double2*>(scratch + idx * kN);
  Xf::key_store(key, lane, xb, scale, f);
  double2 wa[4], wb[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) { wa[v] = key[v * 64 + lane]; wb[v] = key[(v + 4) * 64 + lane]; }
  Xf::fwd_generic(lane, xa, st, buf, f);
  double s0[kRegs], s1[kRegs];
#pragma unroll
  for (int u = 0; u < kRegs; ++u) { s0[u] = 0.0; s1[u] = 0.0; }
  Xf::mac(s0, s1, xa, wa, wa, 0, f);
  Xf::mac(s0, s1, xa, wb, wb, 4, f);
  Xf::inverse(lane, s0, st, buf, f);
  double dev = 0.0;
#pragma unroll
  for (int r = 0; r < kRegs; ++r) out[idx * kN + lane + 64 * r] = Xf::to_torus(s0[r], dev);
  if (Xf::kCertificate) publish_certificate(dev, dev_flag, lane);
}

// -------------------------------------------------------------------------------------------------
// Launchers. cfg: 0 = default-128-shaped gadget, 1 = REDsec-shaped; mode: 0 = exact NTT, 1 = FFT.
// -------------------------------------------------------------------------------------------------
// One step of a plan -> its kernel instantiation. `if constexpr` only keeps a kernel from being instantiated for a policy the plan
// never names it for; such a step (the plan and form_traits disagree) is an error.
template <class Xf>
static hipError_t dispatch_br(const LaunchStep& s, const BlindRotateArgs& a, hipStream_t st) {
  constexpr FormTraits t = form_traits<Xf>();
  constexpr bool kWg = Xf::kWorkgroupForm, kOdd = Xf::Cfg::L % 2 != 0;
  auto run = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)s.grid), dim3((unsigned)s.block), 0, st, a);
    return hipGetLastError();
  };
  switch (plan_key(s.form, s.waves)) {
    case plan_key(kFormCoop8Listed, 8): if constexpr (t.listed_cfg >= 0) return launch_coop8_listed(t.listed_cfg, a, st); break;   // rs_bootstrap_listed.hip
    case plan_key(kFormCoop8, 8): if constexpr (kWg) return run(blind_rotate_coop8_kernel<Xf>); break;
    case plan_key(kFormCoop4, 4): if constexpr ((2 * t.L) % 4 == 0) return run(blind_rotate_coop_kernel<Xf, 4>); break;
    case plan_key(kFormCoop2, 2): return run(blind_rotate_coop_kernel<Xf, 2>);
    case plan_key(kFormWorkgroup, 8): if constexpr (kWg) return run(blind_rotate_wg_kernel<Xf, 8>); break;
    case plan_key(kFormWorkgroup, 4): if constexpr (kWg && kOdd) return run(blind_rotate_wg_kernel<Xf, 4>); break;
    case plan_key(kFormDuo, 8): if constexpr (kWg && !kOdd) return run(blind_rotate_duo_kernel<Xf>); break;
    case plan_key(kFormPerWave, 1): return run(blind_rotate_kernel<Xf, 1>);
    case plan_key(kFormPerWave, 2): return run(blind_rotate_kernel<Xf, 2>);
    case plan_key(kFormPerWave, 4): return run(blind_rotate_kernel<Xf, 4>);
    case plan_key(kFormPerWave, 8): return run(blind_rotate_kernel<Xf, 8>);
  }
  return hipErrorInvalidValue;
}

// Plan (rs_launch_plan.h: every threshold lives there), then per step: slice the arguments, zero what the step needs, dispatch.
template <class Xf>
static hipError_t launch_br_xf(const BlindRotateArgs& whole, int num_cus, const LaunchOpts& o, hipStream_t st, LaunchInfo* info) {
  const LaunchPlan plan = plan_blind_rotate(form_traits<Xf>(), whole.n, whole.B, num_cus, o, whole.progress != nullptr);
  for (int k = 0; k < plan.steps; ++k) {
    BlindRotateArgs a = step_args(whole, plan.step[k]);
    if (hipError_t e = cohort_setup(a, whole.progress, plan.step[k], st); e != hipSuccess) return e;
    if (hipError_t e = counter_setup(a, whole.counter, plan.step[k], st); e != hipSuccess) return e;
    if (hipError_t e = dispatch_br<Xf>(plan.step[k], a, st); e != hipSuccess) return e;
  }
  if (info) *info = plan.info;
  return hipSuccess;
}

hipError_t launch_blind_rotate(int cfg, int mode, const BlindRotateArgs& a, int num_cus, const LaunchOpts& opts, hipStream_t st, LaunchInfo* info) {
  if (a.B <= 0) return hipSuccess;
  if (mode == 0) {
    return cfg == 0 ? launch_br_xf<XfNtt<CfgDefault128>>(a, num_cus, opts, st, info) : launch_br_xf<XfNtt<CfgRedsecV2>>(a, num_cus, opts, st, info);
  }
  return cfg == 0 ? launch_br_xf<XfFft<CfgDefault128>>(a, num_cus, opts, st, info) : launch_br_xf<XfFft<CfgRedsecV2>>(a, num_cus, opts, st, info);
}

// The split duo form's launch (mid-size batches of the split mode): called from rs_bootstrap_split.hip.
hipError_t launch_split_duos(int cfg, const BlindRotateArgs& a, long grid, hipStream_t st) {
  if (cfg == 0) hipLaunchKernelGGL((blind_rotate_duos_kernel<CfgDefault128>), dim3((unsigned)grid), dim3(512), 0, st, a);
  else if (cfg == 1) hipLaunchKernelGGL((blind_rotate_duos_kernel<CfgRedsecV2>), dim3((unsigned)grid), dim3(512), 0, st, a);
  else if (cfg == 2) hipLaunchKernelGGL((blind_rotate_duos_kernel<CfgRedsecSmall>), dim3((unsigned)grid), dim3(512), 0, st, a);
  else return hipErrorNotSupported;
  return hipGetLastError();
}

hipError_t launch_bk_transform(int cfg, int mode, const int32_t* bk, double* bk_x, const double* tw, Field f, double scale,
                               long n_polys, hipStream_t st) {
  constexpr int WPB = 4;
  const dim3 grid((unsigned)((n_polys + WPB - 1) / WPB)), block(64 * WPB);
  if (mode == 1) {
    hipLaunchKernelGGL((bk_transform_kernel<XfFft<CfgDefault128>, WPB>), grid, block, 0, st, bk, bk_x, tw, f, scale, n_polys);
  } else if (cfg == 0) {
    hipLaunchKernelGGL((bk_transform_kernel<XfNtt<CfgDefault128>, WPB>), grid, block, 0, st, bk, bk_x, tw, f, scale, n_polys);
  } else {
    hipLaunchKernelGGL((bk_transform_kernel<XfNtt<CfgRedsecV2>, WPB>), grid, block, 0, st, bk, bk_x, tw, f, scale, n_polys);
  }
  return hipGetLastError();
}

hipError_t launch_polymul(int cfg, int mode, const int32_t* a_small, const int32_t* b_torus, int32_t* out, double* scratch,
                          const double* tw, Field f, double scale, long count, unsigned long long* dev_flag, hipStream_t st) {
  constexpr int WPB = 4;
  const dim3 grid((unsigned)((count + WPB - 1) / WPB)), block(64 * WPB);
  if (mode == 1) {
    hipLaunchKernelGGL((polymul_kernel<XfFft<CfgDefault128>, WPB>), grid, block, 0, st, a_small, b_torus, out, scratch, tw, f, scale, count, dev_flag);
  } else if (cfg == 0) {
    hipLaunchKernelGGL((polymul_kernel<XfNtt<CfgDefault128>, WPB>), grid, block, 0, st, a_small, b_torus, out, scratch, tw, f, scale, count, dev_flag);
  } else {
    hipLaunchKernelGGL((polymul_kernel<XfNtt<CfgRedsecV2>, WPB>), grid, block, 0, st, a_small, b_torus, out, scratch, tw, f, scale, count, dev_flag);
  }
  return hipGetLastError();
}

}  // namespace rs

#if RS_STAMPS_ON(1 | 4 | 8)   // blind_rotate_wg_kernel, blind_rotate_duo_kernel, blind_rotate_coop8_kernel
RS_DEFINE_STAMPS()
#endif
