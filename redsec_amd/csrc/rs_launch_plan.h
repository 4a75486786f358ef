// rs_launch_plan.h -- WHICH kernel form a blind-rotation batch of the N = 1024 ring runs in: kernel, waves per workgroup, grid,
// the cut-off last round and the XCD cohorts. No HIP: a pure function of the batch and the device's CU count, called by the
// launchers (rs_bootstrap.hip, rs_bootstrap_split.hip), which only slice the arguments and dispatch to the kernel instantiation,
// and -- on the host -- by rs_emulate.cpp (rs_emu_launch_plan), so that every threshold is pinned by CPU tests
// (tests/test_directed_cpu.py). The general-ring form is not planned here: its grid comes from an occupancy query (rs_api.cpp).
#pragma once

#include <algorithm>

#include "rs_lds_plan.h"

namespace rs {

// Launch policy switches, read from the environment ONCE at rs_create (A/B experiments only).
struct LaunchOpts {
  bool no_coop = false, no_wg = false, no_duo = false, no_persist = false, no_conv_tiled = false, no_wg4 = false, no_tail = false, no_coop8 = false, no_coop8_listed = false, ks_atomics = false, force_host_staged = false, no_cohort = false;
};
// What a blind-rotate launch actually ran: kernel form and how many ciphertexts share one sweep of the key
// from L2/HBM (R of SURVEY.md section 8d).
enum { kFormPerWave = 0, kFormWorkgroup = 1, kFormDuo = 2, kFormCoop2 = 3, kFormCoop4 = 4, kFormGeneral = 5, kFormSplitWorkgroup = 6, kFormSplitCoop = 7, kFormSplitDuo = 8, kFormCoop8 = 9, kFormCoop8Listed = 10 };
struct LaunchInfo { int form = -1; int waves_per_block = 0; long resident = 0; };
constexpr int kCohortSlots = 64;   // workgroups per XCD the cohort table has room for (256 CUs / 8 XCDs = 32)

// The compile-time facts of a transform policy / gadget the decision depends on (form_traits, rs_bootstrap.h): the policy has the
// eight-wave, lock-step and duo kernels (FFT); gadget length; the REDsec gadget (four waves per ciphertext up to one ciphertext
// per CU); kCoop8ListedCfg of the policy, or -1; the call is the split-key launcher's.
struct FormTraits { bool workgroup_form; int L; bool coop4; int listed_cfg; bool split; };
// One kernel launch on rows [first, first + rows): kForm*, waves per workgroup, grid, threads (64 x waves). persistent: the
// per-wave kernel with the work counter; cohort: the lock-step workgroups get the progress table (rs_cohort.h).
struct LaunchStep {
  int form = -1, waves = 0; long grid = 0; int block = 0; long first = 0, rows = 0;
  bool persistent = false, cohort = false; int cohort_every = 0, cohort_lag = 0;
};
struct LaunchPlan { int steps = 0; LaunchStep step[2]; LaunchInfo info; };   // main launch, cut-off last round
constexpr int plan_key(int form, int waves) { return form * 16 + waves; }   // what the launchers switch over
constexpr int plan_group(const LaunchStep& s) {   // ciphertexts of one workgroup of a lock-step form (0: another kind of form)
  return (s.form == kFormWorkgroup || s.form == kFormSplitWorkgroup) ? s.waves : (s.form == kFormDuo || s.form == kFormSplitDuo) ? 4 : 0;
}

// The form B rows take as ONE launch. `wpb`: waves per workgroup of the per-wave kernel, chosen from the WHOLE batch.
inline LaunchStep plan_single(const FormTraits& t, int n, long B, int wpb, long cus, const LaunchOpts& o) {
  LaunchStep s;
  s.rows = s.grid = B;   // cooperative forms: one ciphertext per workgroup
  auto coop = [&](int form, int waves) { s.form = form; s.waves = waves; s.block = 64 * waves; return s; };
  // lock-step forms: the grid walks the batch in rounds of group x #CUs ciphertexts
  auto lock_step = [&](int form, int waves, int group) { s.grid = std::min((B + group - 1) / group, cus); return coop(form, waves); };
  const bool four = t.coop4 && (2 * t.L) % 4 == 0 && B <= cus;
  if (t.split) {
    // any batch size: even one group walks its CMUX chain faster than a lone wave of the general kernel
    if (!o.no_coop && B <= 2 * cus) return coop(kFormSplitCoop, four ? 4 : 2);
    if (!o.no_duo && B <= 4 * cus) return lock_step(kFormSplitDuo, 8, 4);   // (no_duo: the 4-wave lock-step groups)
    const int w = (B <= 4 * cus && !o.no_wg4) ? 4 : 8;
    return lock_step(kFormSplitWorkgroup, w, w);
  }
  // latency forms: several waves per ciphertext while the batch cannot fill the chip by itself
  if (!o.no_coop) {
    if (t.workgroup_form && !o.no_coop8 && B <= cus)   // eight waves share a ciphertext, two per SIMD
      return coop(t.listed_cfg >= 0 && !o.no_coop8_listed && n <= kCoop8MaxSteps ? kFormCoop8Listed : kFormCoop8, 8);
    if (four) return coop(kFormCoop4, 4);
    if (B <= 2 * cus) return coop(kFormCoop2, 2);
  }
  if (t.workgroup_form && !o.no_wg) {
    // throughput form: lock-step workgroups of 8 ciphertexts, key rows shared in LDS. Taken as soon as the batch exceeds FOUR
    // ciphertexts per CU: a partly filled single round of it (10.2 ms for up to 2,048 default-128 ciphertexts) beats two rounds
    // of the half-size forms (12.8-13.1 ms at 1,536; tools/midsize_rate.py).
    if (B > 4 * cus) return lock_step(kFormWorkgroup, 8, 8);
    // 2 x #CUs < B <= 4 x #CUs. Odd l (no duo form): half-size lock-step groups, 4 ciphertexts x 1 wave = one wave per SIMD, 78 %
    // of the full form's rate per CU and the key rows shared (2-3 % faster than the per-wave kernel). Even l: the duo form, 4
    // ciphertexts x 2 waves; it keeps the mod-switched mask words in LDS, s_bara[4][kSmall], so a longer key runs per wave.
    if (t.L % 2 != 0 && !o.no_wg4 && B > 2 * cus) return lock_step(kFormWorkgroup, 4, 4);
    if (t.L % 2 == 0 && !o.no_duo && n <= kSmall && B > 2 * cus) return lock_step(kFormDuo, 8, 4);
  }
  // one wave per ciphertext. Eight waves are ~150 KB of LDS, exactly one workgroup per CU: beyond that the waves pull rows
  s.grid = (B + wpb - 1) / wpb;
  s.persistent = wpb == 8 && !o.no_persist && s.grid > cus;
  if (s.persistent) s.grid = cus;
  return coop(kFormPerWave, wpb);
}

// The launches of a batch of B > 0 rows with n CMUX steps each. XCD cohorts (the caller offers a progress table) go to the
// lock-step launches whose workgroups sweep the key more than once (groups > grid) on a device whose workgroups are dealt
// round-robin over EIGHT XCDs -- the protocol's xcd = blockIdx & 7: the whole MI355X as one partition (SPX, 256 CUs = 8 x 32);
// under CPX / DPX / QPX a table row would mix workgroups served by different L2s, so there they run free. The lag keeps a cohort
// inside a third of its XCD's 4 MB L2: a CMUX step reads 2l key rows of 16 KB, on the split key 2 x 2l half-rows of 16 KB.
inline LaunchPlan plan_blind_rotate(const FormTraits& t, int n, long B, int num_cus, const LaunchOpts& o, bool cohort_table_offered) {
  const long cus = num_cus;
  const int wpb = B >= 8 * cus ? 8 : B >= 4 * cus ? 4 : B >= 2 * cus ? 2 : 1;
  LaunchPlan p;
  p.steps = 1;
  LaunchStep& m = p.step[0] = plan_single(t, n, B, wpb, cus, o);
  // The unsplit lock-step grid walks the batch in rounds of 8 x #CUs ciphertexts. A last round of at most 4 x #CUs of them is cut
  // off and runs in the form that batch size would take by itself (cooperative / duo / half-size groups: 3.1-8.2 ms against
  // 14.8 ms for a whole round of the REDsec set, tools/midsize_rate.py); every ciphertext is independent of the split. The
  // cut-off launch never has cohorts, is not reported in `info`, and a per-wave one keeps the whole batch's eight waves.
  const long cap = 8 * cus, tail = B % cap;
  if (m.form == kFormWorkgroup && m.waves == 8 && !o.no_tail && B > cap && tail > 0 && tail <= 4 * cus) {
    m.rows = B - tail;
    p.step[1] = plan_single(t, n, tail, wpb, cus, o);
    p.step[1].first = m.rows;
    p.steps = 2;
  }
  const int group = plan_group(m);
  const bool sweeps_together = m.form == kFormWorkgroup || m.form == kFormSplitWorkgroup;
  if (sweeps_together && cohort_table_offered && !o.no_cohort && cus == 256 && m.grid <= 8L * kCohortSlots && (m.rows + group - 1) / group > m.grid) {
    m.cohort = true;
    m.cohort_lag = (int)std::max(1L, (4L << 20) / 3 / ((t.split ? 4L : 2L) * t.L * 16384) - 1);
    m.cohort_every = m.cohort_lag >= 4 ? 2 : 1;
  }
  // ciphertexts of one key sweep: a lock-step grid's; 1 in a cooperative form; per wave those resident at once (an upper bound)
  p.info = {m.form, m.waves, group ? group * m.grid : m.form == kFormPerWave ? std::min(B, m.waves * cus) : 1};
  return p;
}

}  // namespace rs
