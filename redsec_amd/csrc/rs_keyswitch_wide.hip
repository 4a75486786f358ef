// rs_keyswitch_wide.hip -- the WIDE throughput form of the tiled keyswitch (round 16), in an object of its own so that the
// kernels of rs_kernels.hip keep their instructions.
//
// keyswitch_tiled_comb_kernel (rs_kernels.hip) gives a workgroup 256 ciphertexts x 32 output words: the table of combined-digit
// sums is built once per 256 ciphertexts, and the build and the staging of the next base rows sit between two barriers per
// group of coefficients, with 8 waves per CU to cover them. Here ONE workgroup of 16 waves owns a CU: 1,024 ciphertexts x 32
// words (lane = ciphertext, as there), so a table serves four times as many lookups, and both LDS tables are double-buffered
// so that a group of KS_IG coefficients needs ONE barrier. In iteration g
//   * every wave does its lookups of group g from s_tab[g & 1];
//   * between them every thread builds its share of the sums of group g + 1 into s_tab[(g + 1) & 1] from s_base[(g + 1) & 1];
//   * the base rows of group g + 2 travel global -> registers before the lookups and registers -> s_base[g & 1] after them.
// What is read in iteration g was written in iteration g - 1 or earlier, and what is written in iteration g was last read in
// iteration g - 1: the barrier at the end of an iteration orders both.
// D = 1 (no combined digits: the (9, 3) REDsec shape) has no build and no s_base: the rows of group g + 1 are staged straight
// into s_tab[(g + 1) & 1].
// The sums are the same wrapping 32-bit sums in another grouping: bit for bit the result of the other forms.
#include <hip/hip_runtime.h>

#include "rs_diag.h"
#include "rs_host.h"
#include "rs_kernels.h"

namespace rs {

constexpr int KSW_CH = 32;             // output words per workgroup
constexpr int KSW_CHP = KSW_CH + 4;    // padded row (words): the 16 rows of a digit group sit in distinct bank quads
constexpr int KSW_THREADS = kKsWideTile;

template <int T, int BASEBIT, int KS_IG, int D, bool TWO>   // TWO: u = u0 + u1 (bootsMUX)
__global__ __launch_bounds__(KSW_THREADS) void keyswitch_wide_kernel(KeyswitchArgs a) {
  constexpr int BASE = 1 << BASEBIT;
  constexpr int NG = (T + D - 1) / D;              // lookups per coefficient
  constexpr int RG = 1 << (BASEBIT * D);           // rows of a full group
  constexpr int DL = T - (NG - 1) * D;             // digits of the last group (1 ... D)
  constexpr bool kBuild = D > 1;
  constexpr int BROWS = KS_IG * T * BASE, TROWS = KS_IG * NG * RG;
  constexpr int LEAD = kBuild ? 2 : 1;             // groups the staging runs ahead of the lookups
  __shared__ __attribute__((aligned(16))) int32_t s_tab[2][TROWS * KSW_CHP];
  __shared__ __attribute__((aligned(16))) int32_t s_base[2][kBuild ? BROWS * KSW_CHP : 4];
  __shared__ __attribute__((aligned(16))) int32_t s_idle[4];   // where the threads without a staging piece put theirs
  static_assert(sizeof(int32_t) * (2 * (TROWS + (kBuild ? BROWS : 0)) * KSW_CHP + 8) <= 111 * 1024, "one workgroup per CU, <= 111 KB");
  const int tid = threadIdx.x;
  const long ct = (long)blockIdx.x * KSW_THREADS + tid;
  const bool live = ct < a.B;
  const int w0 = (int)blockIdx.y * KSW_CH;
  const int W = a.W, N = a.N;
  const int32_t* u0 = a.u0 + (live ? ct : 0) * (size_t)(N + 1);
  const int32_t* u1 = TWO ? a.u1 + (live ? ct : 0) * (size_t)(N + 1) : nullptr;
  // where the key rows are staged: s_base, or (no build) the lookup table itself. The v = 0 rows stay zero.
  constexpr int STAGE_WORDS = BROWS * KSW_CHP;     // D = 1: TROWS == BROWS
  int32_t* const s_stage = kBuild ? &s_base[0][0] : &s_tab[0][0];
  for (int e = tid; e < 2 * STAGE_WORDS; e += KSW_THREADS) s_stage[e] = 0;

  uint32_t acc[KSW_CH];
#pragma unroll
  for (int k = 0; k < KSW_CH; ++k) acc[k] = 0;
  constexpr uint32_t prec_offset = 1u << (32 - (1 + BASEBIT * T));
  // staging: KS_IG * T * (BASE - 1) row segments of KSW_CH words, 8 threads x 16 B per segment: less than one per thread
  constexpr int SEGS = KS_IG * T * (BASE - 1);
  static_assert(SEGS * 8 <= KSW_THREADS, "one 16-byte piece per thread at most");
  int32_t st[4];
  const int s_seg = tid >> 3, s_part = tid & 7;
  const int s_v = s_seg % (BASE - 1) + 1, s_ij = s_seg / (BASE - 1);   // ij = ii * T + j
  const bool s_on = tid < SEGS * 8;
  // Every thread loads, from an address inside the key, and every thread stores: the threads past the last piece re-read a
  // piece of row (0, 1) into s_idle, and the words past W repeat word W - 1 (their sums are never stored). No branch and no
  // select hangs on the loaded words, so the requests stay in flight behind the lookups until the store needs them.
  const int s_row = ((s_on ? s_ij : 0) * BASE + s_v) * W;
  int s_off[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) s_off[e] = s_row + (w0 + s_part * 4 + e < W ? w0 + s_part * 4 + e : W - 1);
  auto stage_load = [&](int i0) {
    // rows are only 4-byte aligned in general (W odd): assemble from scalar loads
    const int32_t* src = a.ksk + (size_t)i0 * T * BASE * (size_t)W;
#pragma unroll
    for (int e = 0; e < 4; ++e) st[e] = src[s_off[e]];
  };
  int32_t* const s_dst = s_on ? &s_stage[(s_ij * BASE + s_v) * KSW_CHP + s_part * 4] : &s_idle[0];
  auto stage_store = [&](int buf) {
    *reinterpret_cast<int4*>(s_dst + (s_on ? buf * STAGE_WORDS : 0)) = make_int4(st[0], st[1], st[2], st[3]);
  };
  // row `comb` of group gq of coefficient ii = the sum over the group's digits k of base row (ii, gq D + k, digit k of comb),
  // digit 0 the most significant (as it sits in the coefficient); 8 threads x 16 B per row
  constexpr int NB = (TROWS * 8 + KSW_THREADS - 1) / KSW_THREADS;   // build items per thread
  constexpr int NL = KS_IG * NG;                                    // lookups per lane and group
  static_assert(!kBuild || (TROWS * 8 % KSW_THREADS == 0 && NL % NB == 0), "the build is dealt out evenly between the lookups");
  auto build_item = [&](int buf, int item) {
    const int part = item & 7, r = item >> 3;
    const int comb = r % RG, igq = r / RG, gq = igq % NG, ii = igq / NG;
    const int dl = gq == NG - 1 ? DL : D;
    if (comb >> (BASEBIT * dl)) return;       // rows a short last group never selects
    int4 sum = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if (k < dl) {
        const int dgt = ks_comb_digit(comb, k, dl, BASEBIT);   // rs_host.h (host-tested)
        const int4 v = *reinterpret_cast<const int4*>(&s_base[buf][((ii * T + gq * D + k) * BASE + dgt) * KSW_CHP + part * 4]);
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
      }
    }
    *reinterpret_cast<int4*>(&s_tab[buf][r * KSW_CHP + part * 4]) = sum;
  };

  // A lane's KS_IG words of group g (a-bar: the rounding offset added). Lanes past the batch read row 0 and select digit 0.
  // (Sample-load probe of diagnostic builds: a lane-dependent word that costs no memory access -- a constant would make every
  // lane select the same row, which the LDS serves as one broadcast.)
  auto load_words = [&](int g, uint32_t (&dst)[KS_IG]) {
#pragma unroll
    for (int ii = 0; ii < KS_IG; ++ii) {
      const int i = g * KS_IG + ii;
      uint32_t v = (uint32_t)u0[i];
      if (TWO) v += (uint32_t)u1[i];
      if (diag::kKsSampleProbe) v = ((uint32_t)ct * 2654435761u + (uint32_t)i * 40503u) * 2246822519u;
      dst[ii] = live ? v + prec_offset : 0u;
    }
  };

  const int G = N / KS_IG;
  uint32_t ai[KS_IG], un[KS_IG];
  load_words(0, un);
  __syncthreads();
  stage_load(0);
  stage_store(0);
  if (kBuild) {
    if (G > 1) { stage_load(KS_IG); stage_store(1); }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NB; ++h) build_item(0, tid + h * KSW_THREADS);
  }
  __syncthreads();
  for (int g = 0; g < G; ++g) {
    const int buf = g & 1;
#pragma unroll
    for (int ii = 0; ii < KS_IG; ++ii) ai[ii] = un[ii];
    // this lane's words of the NEXT group (the last iteration re-reads its own): requested here, used after the barrier
    load_words(g + 1 < G ? g + 1 : g, un);
    if (g + LEAD < G) stage_load((g + LEAD) * KS_IG);
    // The NL lookups of the group, software-pipelined by hand one deep in steps of half a row (16 words): the four 16-byte reads
    // of step s + 1 are issued before the 16 adds of step s, and the scheduler is held to that order (left alone it hoists the
    // reads of many lookups and spills: 128 registers are all a wave has at 16 waves per CU). This thread's share of the NEXT
    // group's sums is dealt out between the lookups. In the last iteration it rebuilds from a stale s_base into the table
    // nobody reads any more: cheaper than a branch around it in every iteration.
    constexpr int HQ = KSW_CH / 8;                  // 16-byte reads of a step
    constexpr int NS = 2 * NL;                      // steps of a group
    int4 r[2][HQ];
    auto fetch = [&](int s, int4 (&dst)[HQ]) {
      const int l = s / 2, ii = l / NG, gq = l % NG;
      const int dl = gq == NG - 1 ? DL : D;
      const uint32_t comb = ks_comb_index(ai[ii], gq, D, dl, BASEBIT);
      const int4* row = reinterpret_cast<const int4*>(&s_tab[buf][((ii * NG + gq) * RG + (int)comb) * KSW_CHP]) + (s % 2) * HQ;
#pragma unroll
      for (int q = 0; q < HQ; ++q) dst[q] = row[q];
    };
    fetch(0, r[0]);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (kBuild && s % (NS / NB) == 0) build_item(buf ^ 1, tid + (s / (NS / NB)) * KSW_THREADS);
      if (s + 1 < NS) fetch(s + 1, r[(s + 1) & 1]);
      const int k0 = (s % 2) * (KSW_CH / 2);
#pragma unroll
      for (int q = 0; q < HQ; ++q) {
        acc[k0 + 4 * q + 0] += (uint32_t)r[s & 1][q].x;
        acc[k0 + 4 * q + 1] += (uint32_t)r[s & 1][q].y;
        acc[k0 + 4 * q + 2] += (uint32_t)r[s & 1][q].z;
        acc[k0 + 4 * q + 3] += (uint32_t)r[s & 1][q].w;
      }
      // (an empty statement that pins the sums: without it the adds of several lookups are re-associated into three-operand
      // adds whose operands -- the rows of several lookups -- stay live together, 1.8 KB of spills per lane)
#pragma unroll
      for (int k = 0; k < KSW_CH / 2; ++k) asm volatile("" : "+v"(acc[k0 + k]));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (g + LEAD < G) stage_store(kBuild ? buf : buf ^ 1);   // free: last read one iteration ago (its sums are built / its lookups done)
    __syncthreads();
  }
  if (!live) return;
  uint32_t bw = (uint32_t)u0[N];
  if (TWO) bw += (uint32_t)u1[N];
  bw += (uint32_t)a.bconst;
  int32_t* out = a.out + ct * W + w0;
#pragma unroll
  for (int k = 0; k < KSW_CH; ++k) {
    const int w = w0 + k;
    if (w < W) out[k] = (int32_t)((w == W - 1 ? bw : 0u) - acc[k]);
  }
}

hipError_t launch_keyswitch_wide(const KeyswitchArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (!ks_wide_shape(a.t, a.basebit) || a.N % 4 != 0) return hipErrorNotSupported;
  const dim3 grid((unsigned)((a.B + KSW_THREADS - 1) / KSW_THREADS), (unsigned)((a.W + KSW_CH - 1) / KSW_CH), 1);
  if (a.t == 8 && !a.u1) hipLaunchKernelGGL((keyswitch_wide_kernel<8, 2, 4, 2, false>), grid, dim3(KSW_THREADS), 0, st, a);
  else if (a.t == 8) hipLaunchKernelGGL((keyswitch_wide_kernel<8, 2, 4, 2, true>), grid, dim3(KSW_THREADS), 0, st, a);
  else if (!a.u1) hipLaunchKernelGGL((keyswitch_wide_kernel<9, 3, 2, 1, false>), grid, dim3(KSW_THREADS), 0, st, a);
  else hipLaunchKernelGGL((keyswitch_wide_kernel<9, 3, 2, 1, true>), grid, dim3(KSW_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace rs
