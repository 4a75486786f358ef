// rs_emulate.cpp -- TEST-ONLY host emulation of one wavefront of the HIP kernels.
//
// Runs the very same phase functions (rs_ntt.h) lane by lane, with a plain array standing in for
// the LDS exchange buffer, so that the transform's index mapping, the reduction schedule and the
// CMUX bookkeeping can be checked bit-for-bit against the oracle on a machine without a GPU
// (pytest -m "not gpu"). It is NOT part of libredsec_hip.so and is never a fallback: the product
// library has no CPU compute path. Built by redsec_amd/build.py as librs_emulate.so.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "rs_audit.h"
#include "rs_general.h"
#include "rs_host.h"
#include "rs_keygen.h"
#include "rs_pack.h"
#include "rs_packkey.h"
#include "rs_rekey.h"
#include "rs_ring_cmux.h"
#include "rs_ring_lookup.h"
#include "rs_ring_rotate.h"
#include "rs_ring_rekey.h"
#include "rs_ring_selector.h"
#include "rs_rlwe.h"
#include "rs_launch_plan.h"
#include "rs_lds_plan.h"
#include "rs_ntt.h"
#include "rs_circuit.h"
#include "rs_rows.h"
#include "rs_sparse.h"

namespace {

using rs::Field;
using rs::kLanes;
using rs::kN;
using rs::kRegs;

struct Wave {
  double x[kLanes][kRegs];
};

template <class C>
void emu_forward(Wave& w, const double* tw, double* buf, const Field& f) {
  for (int l = 0; l < kLanes; ++l) rs::fwd_F1<C>(l, w.x[l], tw, buf, f);
  for (int l = 0; l < kLanes; ++l) rs::fwd_F2<C>(l, w.x[l], tw, buf, f);
  for (int l = 0; l < kLanes; ++l) rs::fwd_F3(l, w.x[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::fwd_F4<C>(l, w.x[l], tw, buf, f);
}
template <class C>
void emu_forward_digits(Wave& w, const int32_t (*d)[kRegs], int q, uint32_t offset, const double* tw, double* buf, const Field& f) {
  for (int l = 0; l < kLanes; ++l) rs::fwd_F1_digits<C>(l, w.x[l], d[l], q, offset, tw, buf, f);
  for (int l = 0; l < kLanes; ++l) rs::fwd_F2<C>(l, w.x[l], tw, buf, f);
  for (int l = 0; l < kLanes; ++l) rs::fwd_F3(l, w.x[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::fwd_F4<C>(l, w.x[l], tw, buf, f);
}
template <class C>
void emu_inverse(Wave& w, const double* twi, double* buf, const Field& f) {
  for (int l = 0; l < kLanes; ++l) rs::inv_I1<C>(l, w.x[l], twi, buf, f);
  for (int l = 0; l < kLanes; ++l) rs::inv_I2<C>(l, w.x[l], twi, buf, f);
  for (int l = 0; l < kLanes; ++l) rs::inv_I3(l, w.x[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::inv_I4<C>(l, w.x[l], twi, buf, f);
}

// key polynomial -> device layout [v][lane][2], scaled by 1/N, reduced (bk_transform_kernel)
template <class C>
void emu_key_transform(const int32_t* poly, double* dst, const rs::Tables& t, double* buf) {
  Wave w;
  for (int l = 0; l < kLanes; ++l)
    for (int r = 0; r < kRegs; ++r) w.x[l][r] = (double)poly[l + 64 * r];
  emu_forward<C>(w, t.tw.data(), buf, t.f);
  for (int l = 0; l < kLanes; ++l)
    for (int v = 0; v < 8; ++v)
      for (int e = 0; e < 2; ++e) {
        double a = rs::f_reduce(rs::f_mulmod(rs::f_reduce(w.x[l][2 * v + e], t.f), t.ninv, t.f), t.f);
        dst[(v * 64 + l) * 2 + e] = a;
      }
}

template <class C>
int emu_polymul(const int32_t* a_small, const int32_t* b_torus, int32_t* out) {
  rs::PrimeSpec ps;
  if (!rs::prime_for(C::L, C::BGBIT, &ps)) return -1;
  rs::Tables t = rs::make_tables(ps, C::FUSE);
  std::vector<double> buf(rs::kBufDoubles), bkd(kN);
  emu_key_transform<C>(b_torus, bkd.data(), t, buf.data());
  Wave w;
  for (int l = 0; l < kLanes; ++l)
    for (int r = 0; r < kRegs; ++r) w.x[l][r] = (double)a_small[l + 64 * r];
  emu_forward<C>(w, t.tw.data(), buf.data(), t.f);
  for (int l = 0; l < kLanes; ++l)
    for (int u = 0; u < kRegs; ++u) w.x[l][u] = rs::f_mulmod(w.x[l][u], bkd[((u >> 1) * 64 + l) * 2 + (u & 1)], t.f);
  emu_inverse<C>(w, t.tw.data() + kN, buf.data(), t.f);
  for (int l = 0; l < kLanes; ++l)
    for (int r = 0; r < kRegs; ++r) out[l + 64 * r] = rs::f_to_torus32(w.x[l][r]);
  return 0;
}

// blind_rotate_kernel for one ciphertext: in0/in1 rows [n+1], bk torus [n][2l][2][N] -> u [N+1]
template <class C>
int emu_blind_rotate(int n, const int32_t* in0, const int32_t* in1, int32_t c0, int32_t c1, int32_t bconst, int32_t mu,
                     const int32_t* bk, int32_t* u_out, int32_t* acc_out, int steps) {
  rs::PrimeSpec ps;
  if (!rs::prime_for(C::L, C::BGBIT, &ps)) return -1;
  rs::Tables t = rs::make_tables(ps, C::FUSE);
  const Field f = t.f;
  const double* tw = t.tw.data();
  const double* twi = tw + kN;
  std::vector<double> buf(rs::kBufDoubles);
  constexpr int KPL = 2 * C::L;
  std::vector<double> bk_ntt((size_t)n * KPL * 2 * kN);
  for (size_t poly = 0; poly < (size_t)n * KPL * 2; ++poly)
    emu_key_transform<C>(bk + poly * kN, bk_ntt.data() + poly * kN, t, buf.data());

  auto word = [&](int i) -> int32_t {
    uint32_t v = (uint32_t)c0 * (uint32_t)in0[i];
    if (in1) v += (uint32_t)c1 * (uint32_t)in1[i];
    return (int32_t)v;
  };
  std::vector<int32_t> acc0(kN), acc1(kN);
  const int32_t barb = rs::modswitch_2N((int32_t)((uint32_t)word(n) + (uint32_t)bconst));
  const int rot = 2 * kN - barb;
  for (int j = 0; j < kN; ++j) { acc0[j] = 0; acc1[j] = rs::rotated_const(mu, j, rot); }
  constexpr uint32_t offset = rs::gadget_offset<C>();
  if (steps < 0 || steps > n) steps = n;
  Wave s0, s1, x;
  static int32_t d[kLanes][kRegs];
  for (int i = 0; i < steps; ++i) {
    const int32_t bara = rs::modswitch_2N(word(i));
    if (bara == 0) continue;
    std::memset(&s0, 0, sizeof s0);
    std::memset(&s1, 0, sizeof s1);
    const double* bk_i = bk_ntt.data() + (size_t)i * KPL * 2 * kN;
    for (int comp = 0; comp < 2; ++comp) {
      const int32_t* accc = comp ? acc1.data() : acc0.data();
      for (int l = 0; l < kLanes; ++l)
        for (int r = 0; r < kRegs; ++r) d[l][r] = rs::rotated_diff(accc, l + 64 * r, bara);
      for (int q = 0; q < C::L; ++q) {
        const int row = comp * C::L + q;
        const double* bp0 = bk_i + (size_t)(row * 2) * kN;
        const double* bp1 = bp0 + kN;
        emu_forward_digits<C>(x, d, q, offset, tw, buf.data(), f);
        for (int l = 0; l < kLanes; ++l)
          for (int u = 0; u < kRegs; ++u) {
            const size_t k = ((size_t)(u >> 1) * 64 + l) * 2 + (u & 1);
            s0.x[l][u] += rs::f_mulmod(x.x[l][u], bp0[k], f);
            s1.x[l][u] += rs::f_mulmod(x.x[l][u], bp1[k], f);
          }
      }
      if (C::MID_REDUCE && comp == 0)
        for (int l = 0; l < kLanes; ++l)
          for (int u = 0; u < kRegs; ++u) { s0.x[l][u] = rs::f_reduce(s0.x[l][u], f); s1.x[l][u] = rs::f_reduce(s1.x[l][u], f); }
    }
    emu_inverse<C>(s0, twi, buf.data(), f);
    for (int l = 0; l < kLanes; ++l)
      for (int r = 0; r < kRegs; ++r) {
        const int j = l + 64 * r;
        acc0[j] = (int32_t)((uint32_t)acc0[j] + (uint32_t)rs::f_to_torus32(s0.x[l][r]));
      }
    emu_inverse<C>(s1, twi, buf.data(), f);
    for (int l = 0; l < kLanes; ++l)
      for (int r = 0; r < kRegs; ++r) {
        const int j = l + 64 * r;
        acc1[j] = (int32_t)((uint32_t)acc1[j] + (uint32_t)rs::f_to_torus32(s1.x[l][r]));
      }
  }
  if (acc_out) {
    std::memcpy(acc_out, acc0.data(), sizeof(int32_t) * kN);
    std::memcpy(acc_out + kN, acc1.data(), sizeof(int32_t) * kN);
  }
  if (u_out) {
    for (int j = 0; j < kN; ++j) u_out[j] = (j == 0) ? acc0[0] : (int32_t)(0u - (uint32_t)acc0[kN - j]);
    u_out[kN] = acc1[0];
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// FFT mode (rs_fft.h)
// ---------------------------------------------------------------------------------------------
static int g_planar = 0;   // 1: exercise the planar (one plane at a time) exchange of the workgroup kernel

template <int L0, int L1, int T>
void emu_exchange(Wave& w, double* buf) {
  for (int l = 0; l < kLanes; ++l) rs::fpl_store<L0, T, 0>(l, w.x[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::fpl_load<L1, T, 0>(l, w.x[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::fpl_store<L0, T, 1>(l, w.x[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::fpl_load<L1, T, 1>(l, w.x[l], buf);
}

void emu_fft_forward(Wave& w, const double* tw, double* buf) {
  static rs::FftTw t[kLanes];
  for (int l = 0; l < kLanes; ++l) rs::fft_tw_load(t[l], l, tw);
  if (g_planar) {
    for (int l = 0; l < kLanes; ++l) { rs::fft_stage_fwd<0>(w.x[l], t[l]); rs::fft_stage_fwd<1>(w.x[l], t[l]); rs::fft_stage_fwd<2>(w.x[l], t[l]); }
    emu_exchange<rs::kLayA, rs::kLayB, 1>(w, buf);
    for (int l = 0; l < kLanes; ++l) { rs::fft_stage_fwd<3>(w.x[l], t[l]); rs::fft_stage_fwd<4>(w.x[l], t[l]); rs::fft_stage_fwd<5>(w.x[l], t[l]); }
    emu_exchange<rs::kLayB, rs::kLayC, 2>(w, buf);
    for (int l = 0; l < kLanes; ++l) { rs::fft_stage_fwd<6>(w.x[l], t[l]); rs::fft_stage_fwd<7>(w.x[l], t[l]); rs::fft_stage_fwd<8>(w.x[l], t[l]); }
    return;
  }
  for (int l = 0; l < kLanes; ++l) rs::ffwd_F1(l, w.x[l], t[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::ffwd_F2(l, w.x[l], t[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::ffwd_F3(l, w.x[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::ffwd_F4(l, w.x[l], t[l], buf);
}
void emu_fft_inverse(Wave& w, const double* tw, double* buf) {
  static rs::FftTw t[kLanes];
  for (int l = 0; l < kLanes; ++l) rs::fft_tw_load(t[l], l, tw);
  if (g_planar) {
    for (int l = 0; l < kLanes; ++l) { rs::fft_stage_inv<8>(w.x[l], t[l]); rs::fft_stage_inv<7>(w.x[l], t[l]); rs::fft_stage_inv<6>(w.x[l], t[l]); }
    emu_exchange<rs::kLayC, rs::kLayB, 2>(w, buf);
    for (int l = 0; l < kLanes; ++l) { rs::fft_stage_inv<5>(w.x[l], t[l]); rs::fft_stage_inv<4>(w.x[l], t[l]); rs::fft_stage_inv<3>(w.x[l], t[l]); }
    emu_exchange<rs::kLayB, rs::kLayA, 1>(w, buf);
    for (int l = 0; l < kLanes; ++l) { rs::fft_stage_inv<2>(w.x[l], t[l]); rs::fft_stage_inv<1>(w.x[l], t[l]); rs::fft_stage_inv<0>(w.x[l], t[l]); }
    return;
  }
  for (int l = 0; l < kLanes; ++l) rs::finv_I1(l, w.x[l], t[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::finv_I2(l, w.x[l], t[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::finv_I3(l, w.x[l], buf);
  for (int l = 0; l < kLanes; ++l) rs::finv_I4(l, w.x[l], t[l], buf);
}
// key polynomial -> [v][lane][2] = (re, im) of transform position 8*lane + v, scaled by 1/M
void emu_fft_key_transform(const int32_t* poly, double* dst, const double* tw, double* buf) {
  Wave w;
  for (int l = 0; l < kLanes; ++l)
    for (int r = 0; r < kRegs; ++r) w.x[l][r] = (double)poly[l + 64 * r];
  emu_fft_forward(w, tw, buf);
  for (int l = 0; l < kLanes; ++l)
    for (int v = 0; v < 8; ++v) {
      dst[(v * 64 + l) * 2] = w.x[l][v] * (1.0 / rs::kM);
      dst[(v * 64 + l) * 2 + 1] = w.x[l][v + 8] * (1.0 / rs::kM);
    }
}

template <class C>
int emu_blind_rotate_fft(int n, const int32_t* in0, const int32_t* in1, int32_t c0, int32_t c1, int32_t bconst, int32_t mu,
                         const int32_t* bk, int32_t* u_out, int32_t* acc_out, int steps, double* max_dev_out) {
  std::vector<double> tw = rs::make_fft_tables();
  std::vector<double> buf(rs::kBufDoubles);
  constexpr int KPL = 2 * C::L;
  std::vector<double> bk_fft((size_t)n * KPL * 2 * kN);
  for (size_t poly = 0; poly < (size_t)n * KPL * 2; ++poly)
    emu_fft_key_transform(bk + poly * kN, bk_fft.data() + poly * kN, tw.data(), buf.data());
  auto word = [&](int i) -> int32_t {
    uint32_t v = (uint32_t)c0 * (uint32_t)in0[i];
    if (in1) v += (uint32_t)c1 * (uint32_t)in1[i];
    return (int32_t)v;
  };
  std::vector<int32_t> acc0(kN), acc1(kN);
  const int32_t barb = rs::modswitch_2N((int32_t)((uint32_t)word(n) + (uint32_t)bconst));
  const int rot = 2 * kN - barb;
  for (int j = 0; j < kN; ++j) { acc0[j] = 0; acc1[j] = rs::rotated_const(mu, j, rot); }
  constexpr uint32_t offset = rs::gadget_offset<C>();
  if (steps < 0 || steps > n) steps = n;
  Wave s0, s1, x;
  double max_dev = 0.0;
  for (int i = 0; i < steps; ++i) {
    const int32_t bara = rs::modswitch_2N(word(i));
    if (bara == 0) continue;
    std::memset(&s0, 0, sizeof s0);
    std::memset(&s1, 0, sizeof s1);
    const double* bk_i = bk_fft.data() + (size_t)i * KPL * 2 * kN;
    for (int comp = 0; comp < 2; ++comp) {
      const int32_t* accc = comp ? acc1.data() : acc0.data();
      for (int q = 0; q < C::L; ++q) {
        const int row = comp * C::L + q;
        const double* bp0 = bk_i + (size_t)(row * 2) * kN;
        const double* bp1 = bp0 + kN;
        for (int l = 0; l < kLanes; ++l)
          for (int r = 0; r < kRegs; ++r) x.x[l][r] = (double)rs::gadget_digit_prepared<C>(rs::gadget_prepare<C>(rs::rotated_diff(accc, l + 64 * r, bara)), q);
        emu_fft_forward(x, tw.data(), buf.data());
        for (int l = 0; l < kLanes; ++l)
          for (int v = 0; v < 8; ++v) {
            const size_t k = ((size_t)v * 64 + l) * 2;
            rs::fft_cmac(s0.x[l][v], s0.x[l][v + 8], x.x[l][v], x.x[l][v + 8], bp0[k], bp0[k + 1]);
            rs::fft_cmac(s1.x[l][v], s1.x[l][v + 8], x.x[l][v], x.x[l][v + 8], bp1[k], bp1[k + 1]);
          }
      }
    }
    emu_fft_inverse(s0, tw.data(), buf.data());
    emu_fft_inverse(s1, tw.data(), buf.data());
    for (int l = 0; l < kLanes; ++l)
      for (int r = 0; r < kRegs; ++r) {
        const int j = l + 64 * r;
        acc0[j] = (int32_t)((uint32_t)acc0[j] + (uint32_t)rs::fft_round_torus32(s0.x[l][r], max_dev));
        acc1[j] = (int32_t)((uint32_t)acc1[j] + (uint32_t)rs::fft_round_torus32(s1.x[l][r], max_dev));
      }
  }
  if (max_dev_out) *max_dev_out = max_dev;
  if (acc_out) {
    std::memcpy(acc_out, acc0.data(), sizeof(int32_t) * kN);
    std::memcpy(acc_out + kN, acc1.data(), sizeof(int32_t) * kN);
  }
  if (u_out) {
    for (int j = 0; j < kN; ++j) u_out[j] = (j == 0) ? acc0[0] : (int32_t)(0u - (uint32_t)acc0[kN - j]);
    u_out[kN] = acc1[0];
  }
  return 0;
}


// ---- general ring path (rs_general.h): the workgroup's threads run phase by phase, two arrays stand in for the LDS planes ----
template <int LOGN>
struct GenEmu {
  using G = rs::Gen<LOGN>;
  std::vector<double> tw, re, im;
  std::vector<double> x;   // [T][16]
  GenEmu() : tw((size_t)G::N), re(G::kPlane), im(G::kPlane), x((size_t)G::T * 16) { rs::gen_make_twiddles(LOGN, tw.data()); }
  double (&regs(int t))[kRegs] { return *reinterpret_cast<double (*)[kRegs]>(&x[(size_t)t * 16]); }

  template <int P>
  void pass_fwd() {
    if constexpr (P > 0) {
      for (int t = 0; t < G::T; ++t) rs::gen_store<LOGN, P - 1, P - 1>(regs(t), t, re.data(), im.data());
      for (int t = 0; t < G::T; ++t) rs::gen_load<LOGN, P, P - 1>(regs(t), t, re.data(), im.data());
    }
    for (int t = 0; t < G::T; ++t) {
      rs::GenPassTw w;
      rs::gen_pass_tw<LOGN, P>(w, t, tw.data());
      rs::gen_pass_fwd<LOGN, P>(regs(t), w);
    }
    if constexpr (P + 1 < G::P) pass_fwd<P + 1>();
  }
  template <int P>
  void pass_inv() {
    for (int t = 0; t < G::T; ++t) {
      rs::GenPassTw w;
      rs::gen_pass_tw<LOGN, P>(w, t, tw.data());
      rs::gen_pass_inv<LOGN, P>(regs(t), w);
    }
    if constexpr (P > 0) {
      for (int t = 0; t < G::T; ++t) rs::gen_store<LOGN, P, P - 1>(regs(t), t, re.data(), im.data());
      for (int t = 0; t < G::T; ++t) rs::gen_load<LOGN, P - 1, P - 1>(regs(t), t, re.data(), im.data());
      pass_inv<P - 1>();
    }
  }
  void load_poly(const int32_t* poly, int piece /* -1: as is, 0 lo, 1 hi */) {
    for (int t = 0; t < G::T; ++t)
      for (int r = 0; r < 16; ++r) {
        const int32_t c = poly[t + G::T * (r & 7) + (r >> 3) * G::M];
        int32_t lo = c, hi = c;
        if (piece >= 0) rs::gen_split_key(c, lo, hi);
        regs(t)[r] = (double)(piece == 1 ? hi : lo);
      }
  }
  int polymul(const int32_t* a_small, const int32_t* b_torus, int32_t* out, double* max_dev) {
    std::vector<double> key[2];
    for (int piece = 0; piece < 2; ++piece) {
      load_poly(b_torus, piece);
      pass_fwd<0>();
      key[piece].assign(x.begin(), x.end());
    }
    load_poly(a_small, -1);
    pass_fwd<0>();
    const std::vector<double> xa = x;
    std::vector<uint32_t> acc((size_t)G::N, 0u);
    double dev = 0.0;
    for (int piece = 0; piece < 2; ++piece) {
      for (int t = 0; t < G::T; ++t)
        for (int r = 0; r < 8; ++r) {
          double sr = 0.0, si = 0.0;
          const size_t o = (size_t)t * 16 + r;
          rs::fft_cmac(sr, si, xa[o], xa[o + 8], key[piece][o] * (1.0 / G::M), key[piece][o + 8] * (1.0 / G::M));
          x[o] = sr; x[o + 8] = si;
        }
      pass_inv<G::P - 1>();
      for (int t = 0; t < G::T; ++t)
        for (int r = 0; r < 16; ++r) {
          const int j = t + G::T * (r & 7) + (r >> 3) * G::M;
          acc[j] += (uint32_t)rs::fft_round_torus32(regs(t)[r], dev) << (16 * piece);
        }
    }
    for (int j = 0; j < G::N; ++j) out[j] = (int32_t)acc[j];
    if (max_dev) *max_dev = dev;
    return 0;
  }
  // Measured 2-norm error of one forward and one inverse transform against an 80-bit reference (direct evaluation at the
  // tree's roots), relative to sqrt(M) ||input||_2: ratios[0] forward, ratios[1] inverse. The a-priori analysis of
  // rs_general.h bounds them by g_f - 1 and g_i - 1; a sanity check of its per-stage constants, not a proof.
  void transform_error_ratios(uint64_t seed, int amplitude, double* ratios) {
    const long double pi = 3.141592653589793238462643383279502884L;
    std::vector<long double> cr((size_t)2 * G::N), ci((size_t)2 * G::N);
    for (int e = 0; e < 2 * G::N; ++e) { cr[e] = cosl(pi * e / G::N); ci[e] = sinl(pi * e / G::N); }
    auto bitrev = [](int p) { int r = 0; for (int b = 0; b < G::LOGM; ++b) r |= ((p >> b) & 1) << (G::LOGM - 1 - b); return r; };
    uint64_t st = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    // forward: folded value j = t + T r  (registers r, r + 8 = re, im), signs random, magnitudes up to `amplitude`
    std::vector<long double> zr(G::M), zi(G::M);
    long double nin = 0;
    for (int t = 0; t < G::T; ++t)
      for (int r = 0; r < 8; ++r) {
        const int j = t + G::T * r;
        const int a = (int)(rnd() % (2u * (unsigned)amplitude + 1u)) - amplitude, b = (rnd() & 1) ? amplitude : -amplitude;
        regs(t)[r] = (double)a; regs(t)[r + 8] = (double)b;
        zr[j] = a; zi[j] = b;
        nin += (long double)a * a + (long double)b * b;
      }
    pass_fwd<0>();
    std::vector<long double> Xr(G::M), Xi(G::M);
    long double err = 0;
    for (int p = 0; p < G::M; ++p) {
      const long e1 = 1 + 4L * bitrev(p);
      long double sr = 0, si = 0;
      for (int j = 0; j < G::M; ++j) {
        const int e = (int)((e1 * j) % (2L * G::N));
        sr += zr[j] * cr[e] - zi[j] * ci[e];
        si += zr[j] * ci[e] + zi[j] * cr[e];
      }
      Xr[p] = sr; Xi[p] = si;
      const long double dr = (long double)regs(p >> 3)[p & 7] - sr, di = (long double)regs(p >> 3)[(p & 7) + 8] - si;
      err += dr * dr + di * di;
    }
    ratios[0] = (double)(sqrtl(err) / (sqrtl((long double)G::M) * sqrtl(nin)));
    // inverse of the (rounded) forward values: z'_j = sum_p X_p conj(root_p)^j = M z_j
    long double nX = 0;
    for (int p = 0; p < G::M; ++p) {
      Xr[p] = (long double)regs(p >> 3)[p & 7]; Xi[p] = (long double)regs(p >> 3)[(p & 7) + 8];
      nX += Xr[p] * Xr[p] + Xi[p] * Xi[p];
    }
    pass_inv<G::P - 1>();
    err = 0;
    for (int j = 0; j < G::M; ++j) {
      long double sr = 0, si = 0;
      for (int p = 0; p < G::M; ++p) {
        const int e = (int)(((1 + 4L * bitrev(p)) * j) % (2L * G::N));
        sr += Xr[p] * cr[e] + Xi[p] * ci[e];
        si += Xi[p] * cr[e] - Xr[p] * ci[e];
      }
      const int t = j % G::T, r = j / G::T;
      const long double dr = (long double)regs(t)[r] - sr, di = (long double)regs(t)[r + 8] - si;
      err += dr * dr + di * di;
    }
    ratios[1] = (double)(sqrtl(err) / (sqrtl((long double)G::M) * sqrtl(nX)));
  }
  // (a) register r sits at register 0's position plus the compile-time offset the device code uses; (b) the 8-byte accesses
  // of every 32-lane group hit 32 different bank pairs on both sides of every exchange. Returns the number of violations.
  template <int XP>
  static long layout_violations() {
    long bad = 0;
    if constexpr (XP + 1 < G::P) {
      auto side = [&](auto lay_c) {
        constexpr int LAY = decltype(lay_c)::value;
        for (int r = 0; r < 8; ++r) {
          for (int t = 0; t < G::T; ++t)
            bad += rs::gen_phys(rs::gen_idx(t, G::H(LAY), r), G::H(XP + 1)) !=
                   rs::gen_phys(rs::gen_idx(t, G::H(LAY), 0), G::H(XP + 1)) + rs::gen_reg_offset<LOGN, LAY, XP>(r);
          for (int g = 0; g < G::T; g += 32) {
            unsigned seen = 0;
            for (int t = g; t < g + 32; ++t) {
              const int pos = rs::gen_phys(rs::gen_idx(t, G::H(LAY), r), G::H(XP + 1));
              if (pos < 0 || pos >= G::kPlane) ++bad;
              const unsigned bit = 1u << (pos & 31);
              if (seen & bit) ++bad;
              seen |= bit;
            }
          }
        }
      };
      side(std::integral_constant<int, XP>{});
      side(std::integral_constant<int, XP + 1>{});
      bad += layout_violations<XP + 1>();
    }
    return bad;
  }
};

}  // namespace

// Planar exchange of rs_fft.h (8-byte stores, 16-byte loads), all four directions: every value has its own position inside the
// plane, the reader's registers (2m, 2m+1) are adjacent and 16-byte aligned, every ds_write_b64 (lane groups of 16 consecutive
// lanes, 32 banks of 4 bytes) and every ds_read_b128 (the four lane groups of MI355X_MICROARCH.md, 64 banks) is conflict-free.
template <int FROM, int TO, int T>
static long plane_violations() {
  long bad = 0;
  static const int kGroups128[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                        {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  double buf[rs::kPlaneDoubles];
  for (int i = 0; i < rs::kPlaneDoubles; ++i) buf[i] = -1.0;
  // the functions the device runs: store value id (lane, k), load it back in the other layout
  for (int lane = 0; lane < 64; ++lane) {
    double x[rs::kRegs];
    for (int k = 0; k < 8; ++k) x[k] = (double)rs::flay_index<FROM>(lane, k);
    rs::fpl_store<FROM, T, 0>(lane, x, buf);
  }
  for (int lane = 0; lane < 64; ++lane) {
    double x[rs::kRegs];
    rs::fpl_load<TO, T, 0>(lane, x, buf);
    for (int k = 0; k < 8; ++k) bad += x[k] != (double)rs::flay_index<TO>(lane, k);
  }
  for (int k = 0; k < 8; ++k) {        // stores: register k of 16 consecutive lanes
    for (int g = 0; g < 4; ++g) {
      int hits[32] = {0};
      for (int l = 16 * g; l < 16 * g + 16; ++l) {
        int a, b, c;
        rs::flay_abc<FROM>(l, k, a, b, c);
        const int pos = rs::xpos<FROM, TO>(a, b, c);
        bad += pos < 0 || pos >= rs::kPlaneDoubles;
        ++hits[(2 * pos) % 32]; ++hits[(2 * pos + 1) % 32];
      }
      for (int h : hits) bad += h != 1;
    }
  }
  for (int m = 0; m < 4; ++m) {        // loads: registers (2m, 2m + 1) of each ds_read_b128 lane group
    for (int g = 0; g < 4; ++g) {
      int hits[64] = {0};
      for (int i = 0; i < 16; ++i) {
        const int l = kGroups128[g][i];
        int a, b, c, a1, b1, c1;
        rs::flay_abc<TO>(l, 2 * m, a, b, c);
        rs::flay_abc<TO>(l, 2 * m + 1, a1, b1, c1);
        const int pos = rs::xpos<FROM, TO>(a, b, c);
        bad += (pos & 1) != 0 || rs::xpos<FROM, TO>(a1, b1, c1) != pos + 1;
        for (int d = 0; d < 4; ++d) ++hits[(2 * pos + d) % 64];
      }
      for (int h : hits) bad += h != 1;
    }
  }
  return bad;
}

// Wave-local exchanges (rs_general.h, gen_exchange_is_wave_local) rely on every exchange mapping the 512 values of wavefront w to
// the SAME slots [576 w, 576 (w + 1)): what a wavefront reads in one exchange must be where it alone writes in the next, or
// its barrier-free stores overwrite data another wavefront is still reading. Counts, over all exchanges of ring 2^LOGN in both
// directions, the slots a wavefront READS outside its region (always forbidden) and the slots it WRITES outside it in an
// exchange that runs without workgroup barriers.
template <int LOGN, int XP>
long gen_wave_region_violations_xp() {
  using G = rs::Gen<LOGN>;
  long bad = 0;
  if constexpr (XP + 1 < G::P) {
    const bool local = rs::gen_exchange_is_wave_local<LOGN, XP>();
    for (int t = 0; t < G::T; ++t) {
      const int w = t >> 6, lo = 576 * w, hi = 576 * (w + 1);
      for (int r = 0; r < 8; ++r) {
        // forward: stores in the layout of pass XP, loads in the layout of pass XP + 1; the inverse swaps the two roles
        const int p_lay0 = rs::gen_phys(rs::gen_idx(t, G::H(XP), r), G::H(XP + 1));
        const int p_lay1 = rs::gen_phys(rs::gen_idx(t, G::H(XP + 1), r), G::H(XP + 1));
        const bool in0 = p_lay0 >= lo && p_lay0 < hi, in1 = p_lay1 >= lo && p_lay1 < hi;
        bad += !in1;                       // forward reader / inverse writer: its own block region in every exchange
        if (local) bad += !in0;            // forward writer / inverse reader of a barrier-free exchange
        bad += p_lay0 < 0 || p_lay0 >= G::kPlane || p_lay1 < 0 || p_lay1 >= G::kPlane;
      }
    }
    bad += gen_wave_region_violations_xp<LOGN, XP + 1>();
  }
  return bad;
}

// ---- LDS protocol model of the N = 1024 blind-rotation forms (rs_lds_plan.h) --------------------------------------------
// The waves of a workgroup advance from barrier to barrier; an EPOCH is what lies between two consecutive workgroup barriers.
// Inside an epoch nothing orders the waves, so two accesses by DIFFERENT waves to overlapping bytes, at least one a write,
// are a race (an LDS atomic against an LDS atomic is not). A direct global->LDS load is a write that may land at any moment
// from its issue to the barrier behind the issuing wave's s_waitcnt: it is entered into every epoch of that span. Each form
// below replays two CMUX steps of its kernel with the placement functions of rs_lds_plan.h -- the same functions the kernels
// call -- and the checker counts conflicting pairs. `broken` != 0 perturbs ONE decision of the protocol (a placement, a slot
// count, a hold) the way a plausible edit would: the count must then be positive, which shows the check can see such an edit.
namespace {
struct LdsAcc { int wave, epoch, kind; long lo, hi; };   // kind 0 read, 1 write, 2 atomic
struct LdsModel {
  std::vector<LdsAcc> v;
  int epoch = 0;
  enum : long { BUF = 1L << 24, PART = 2L << 24, ACC = 3L << 24, KEY = 4L << 24 };   // array bases (bytes); windows never cross
  void acc(int w, int kind, long lo, long bytes, int e = -1) { v.push_back({w, e < 0 ? epoch : e, kind, lo, lo + bytes}); }
  void rd(int w, long lo, long bytes) { acc(w, 0, lo, bytes); }
  void wr(int w, long lo, long bytes) { acc(w, 1, lo, bytes); }
  void rw(int w, long lo, long bytes) { rd(w, lo, bytes); wr(w, lo, bytes); }
  void atomic(int w, long lo, long bytes) { acc(w, 2, lo, bytes); }
  void dma(int w, long lo, long bytes, int first_epoch, int last_epoch) { for (int e = first_epoch; e <= last_epoch; ++e) acc(w, 1, lo, bytes, e); }
  void barrier() { ++epoch; }
  long conflicts() const {
    long bad = 0;
    for (size_t i = 0; i < v.size(); ++i)
      for (size_t j = i + 1; j < v.size(); ++j) {
        const LdsAcc &a = v[i], &b = v[j];
        if (a.wave == b.wave || a.epoch != b.epoch || a.hi <= b.lo || b.hi <= a.lo) continue;
        if (a.kind == 0 && b.kind == 0) continue;
        if (a.kind == 2 && b.kind == 2) continue;
        ++bad;
      }
    return bad;
  }
};
constexpr long kBufBytes = (long)rs::kBufDoubles * 8, kPolyBytes = (long)rs::kN * 8, kAccBytes = (long)rs::kN * 4, kChunkBytes = 1024;
long buf_of(int w) { return LdsModel::BUF + w * 0x10000L; }

// blind_rotate_coop_kernel<G> (G = 2, 4): s_part[wave][col], waves 0 / 1 invert column 0 / 1
long model_coop(int G, int broken) {
  LdsModel m;
  auto part = [&](int w, int col) { return LdsModel::PART + (w * 2 + col) * kPolyBytes; };
  for (int step = 0; step < 2; ++step) {
    for (int w = 0; w < G; ++w) {
      const int comp = w / (G / 2);
      m.rd(w, LdsModel::ACC + comp * kAccBytes, kAccBytes);
      m.rw(w, buf_of(w), kBufBytes);
      for (int col = 0; col < 2; ++col) m.wr(w, part(broken == 1 ? w / 2 : w, col), kPolyBytes);
    }
    m.barrier();
    for (int w = 0; w < 2; ++w) {
      for (int g = 0; g < G; ++g) m.rd(w, part(g, w), kPolyBytes);
      m.rw(w, buf_of(w), kBufBytes);
      m.rw(w, LdsModel::ACC + w * kAccBytes, kAccBytes);
    }
    if (broken != 2) m.barrier();
  }
  return m.conflicts();
}
// blind_rotate_coop8_kernel. Round-5 step (l >= 4), two epochs: (1) the row waves read their component of the accumulator,
// transform, and add their partials into s_sum[2][N] by LDS f64 atomics; (2) the two inverse waves read their column's sum,
// clear it for the next step, transform, update the accumulator. LISTED step (coop8_listed: l < 4), three epochs: all 512
// threads first build the prepared rotated difference s_d[2][N] from the accumulator (thread t: coefficients (t & 255) + 256 m
// of component coop8_diff_comp(wave)), and the row waves read s_d instead of the accumulator; the step list s_steps is written
// once in the prologue (its own epoch) and only read afterwards.
long model_coop8_atomics(int L, int broken) {
  LdsModel m;
  const bool listed = rs::coop8_listed(L);
  auto sum = [&](int col) { return LdsModel::PART + col * kPolyBytes; };
  auto diff = [&](int c) { return LdsModel::KEY + c * kAccBytes; };     // s_d (the form has no key buffer: the window is free)
  const long steps_lo = LdsModel::KEY + 0x100000L, steps_bytes = 4L * (rs::kCoop8MaxSteps + 1);
  if (listed) m.wr(2, steps_lo, steps_bytes);                            // prologue: wave 2 lists the steps
  for (int w = 0; w < 2; ++w) m.wr(w, LdsModel::ACC + w * kAccBytes, kAccBytes);
  m.barrier();
  for (int step = 0; step < 2; ++step) {
    if (listed) {
      for (int w = 0; w < rs::kCoop8Waves; ++w) {
        const int c = rs::coop8_diff_comp(w);
        m.rd(w, steps_lo, steps_bytes);
        m.rd(w, LdsModel::ACC + c * kAccBytes, kAccBytes);               // rotated reads reach the whole component
        for (int q = 0; q < 4; ++q) m.wr(w, diff(c) + 4L * (256 * q + 64 * (w & 3)), 4L * 64);   // its 4 x 64 coefficients
      }
      if (broken != 3) m.barrier();
    }
    // perturbation 1, listed step: the inverse waves clear their sums only here, beside the next step's atomics (anywhere up to
    // the barrier above would be in time: nobody touches the sums while the rotated difference is built)
    if (listed && broken == 1 && step > 0) for (int col = 0; col < 2; ++col) m.wr(col == 0 ? rs::coop8_inv_a(L) : rs::coop8_inv_b(L), sum(col), kPolyBytes);
    for (int w = 0; w < rs::kCoop8Waves; ++w) {
      if (rs::coop8_row_count(L, w) == 0) continue;
      if (listed) m.rd(w, diff(rs::coop8_comp(L, w)), kAccBytes);
      else m.rd(w, LdsModel::ACC + rs::coop8_comp(L, w) * kAccBytes, kAccBytes);
      m.rw(w, buf_of(w), kBufBytes);
      for (int col = 0; col < 2; ++col) m.atomic(w, sum(col), kPolyBytes);
    }
    m.barrier();
    for (int col = 0; col < 2; ++col) {
      const int w = col == 0 ? rs::coop8_inv_a(L) : rs::coop8_inv_b(L);
      m.rd(w, sum(col), kPolyBytes);
      if (broken != 1) m.wr(w, sum(col), kPolyBytes);     // cleared here, in the inverse waves' own epoch ...
      m.rw(w, buf_of(w), kBufBytes);
      m.rw(w, LdsModel::ACC + col * kAccBytes, kAccBytes);
    }
    if (broken != 2) m.barrier();
    // ... perturbation 1, round-5 step: not behind the barrier, where the next step's atomics already run
    if (!listed && broken == 1) for (int col = 0; col < 2; ++col) m.wr(col == 0 ? rs::coop8_inv_a(L) : rs::coop8_inv_b(L), sum(col), kPolyBytes);
  }
  return m.conflicts();
}
// blind_rotate_coops_kernel<G>: s_part[wave][slot of a sum the wave does not own]
template <int G>
long model_coops(int broken) {
  LdsModel m;
  constexpr int OWN = 4 / G;
  auto part = [&](int w, int slot) { return LdsModel::PART + (w * (4 - OWN) + slot) * kPolyBytes; };
  auto slot = [&](int sum, int g) { return broken == 1 ? sum % (4 - OWN) : rs::coops_slot<G>(sum, g); };
  long same_wave_overwrites = 0;
  for (int step = 0; step < 2; ++step) {
    for (int w = 0; w < G; ++w) {
      m.rd(w, LdsModel::ACC + (w / (G / 2)) * kAccBytes, kAccBytes);
      m.rw(w, buf_of(w), kBufBytes);
      bool used[4] = {false, false, false, false};
      for (int k = 0; k < 4; ++k)
        if (rs::coops_owner<G>(k) != w) {
          const int sl = slot(k, w);
          if (sl < 0 || sl >= 4 - OWN || used[sl]) ++same_wave_overwrites; else used[sl] = true;   // two sums of one wave in one slot
          m.wr(w, part(w, sl < 0 ? 0 : sl % (4 - OWN)), kPolyBytes);
        }
    }
    m.barrier();
    for (int k = 0; k < 4; ++k) {
      const int w = rs::coops_owner<G>(k);
      for (int g = 0; g < G; ++g)
        if (g != w) m.rd(w, part(g, rs::coops_slot<G>(k, g)), kPolyBytes);
      m.rw(w, buf_of(w), kBufBytes);
      if (G == 4) m.atomic(w, LdsModel::ACC + (k & 1) * kAccBytes, kAccBytes);
      else m.rw(w, LdsModel::ACC + w * kAccBytes, kAccBytes);
    }
    if (broken != 2) m.barrier();
  }
  return m.conflicts() + same_wave_overwrites;
}
// blind_rotate_duo_kernel: quads of four 16 KB rows in the 64 KB key buffer, partials swapped through it
long model_duo(int L, int broken) {
  LdsModel m;
  const long slot_bytes = 16 * kChunkBytes;
  auto issue = [&](int first, int last) {
    for (int w = 0; w < 8; ++w) m.dma(w, LdsModel::KEY + rs::duo_quad_slot(w) * slot_bytes + rs::duo_quad_first_chunk(w) * kChunkBytes, 8 * kChunkBytes, first, last);
  };
  auto xchg = [&](int w) { return LdsModel::KEY + (broken == 1 ? rs::duo_xchg_doubles(w) / 2 : rs::duo_xchg_doubles(w)) * 8L; };
  issue(m.epoch, m.epoch);                                   // the first quad of the group, behind the group barrier
  for (int step = 0; step < 2; ++step) {
    for (int p = 0; p < L / 2; ++p) {
      for (int w = 0; w < 8; ++w) { m.rw(w, buf_of(w), kBufBytes); if (p == 0) m.rw(w, LdsModel::ACC + w * kAccBytes, kAccBytes); }   // (inverse +) forward pair
      m.barrier();                                           // s_waitcnt vmcnt(0); barrier: the quad is published
      for (int w = 0; w < 8; ++w) { const int h = w & 1; m.rd(w, LdsModel::KEY + (2 * h) * slot_bytes, 2 * slot_bytes); }
      if (!(broken == 2 && p + 1 < L / 2)) m.barrier();      // every wave has finished reading it
      if (p + 1 < L / 2) issue(m.epoch, m.epoch);
    }
    if (broken == 3) issue(m.epoch, m.epoch + 1);            // the next step's first quad requested BEFORE the swap
    for (int w = 0; w < 8; ++w) m.wr(w, xchg(w), kPolyBytes);
    m.barrier();
    for (int w = 0; w < 8; ++w) m.rd(w, xchg(rs::duo_partner(w)), kPolyBytes);
    m.barrier();
    if (broken != 3) issue(m.epoch, m.epoch);
  }
  return m.conflicts();
}
// blind_rotate_duos_kernel: pairs of half-rows (one per component) in slots 2 (p & 1) + comp; publish(hold)
long model_duos(int L, int broken) {
  LdsModel m;
  const long slot_bytes = 16 * kChunkBytes;
  long issued = 0;
  // a request lands before the barrier of the next publish (s_waitcnt vmcnt(0) in front of it): in flight for the current
  // epoch -- and for one more (`extra`) when the next barrier is the swap's "lgkmcnt(0); s_barrier", which waits for no load
  auto issue_next = [&](int extra = 0) {
    for (int w = 0; w < 8; ++w)
      m.dma(w, LdsModel::KEY + rs::duos_pair_slot(issued, rs::duos_fetch_comp(w)) * slot_bytes + rs::duos_first_chunk(w) * kChunkBytes, 4 * kChunkBytes, m.epoch, m.epoch + extra);
    ++issued;
  };
  long p = 0;
  issue_next();
  for (int step = 0; step < 2; ++step) {
    for (int q = 0; q < L; ++q)
      for (int half = 0; half < 2; ++half) {
        const bool last = q + 1 == L && half == 1;
        if (half == 0) for (int w = 0; w < 8; ++w) { m.rw(w, buf_of(w), kBufBytes); if (q == 0) m.rw(w, LdsModel::ACC + w * kAccBytes, kAccBytes); }
        m.barrier();                                         // publish: waitcnt vmcnt(0) + barrier
        if (!(last && broken != 1)) issue_next(last ? 1 : 0);   // hold at the last pair of a step: the swap needs the buffer first
        for (int w = 0; w < 8; ++w) m.rd(w, LdsModel::KEY + rs::duos_pair_slot(p, w & 1) * slot_bytes, slot_bytes);
        ++p;
      }
    m.barrier();                                             // every wave has consumed the last pair
    for (int round = 0; round < 2; ++round) {                // low halves, then high halves
      for (int w = 0; w < 8; ++w) m.wr(w, LdsModel::KEY + rs::duo_xchg_doubles(w) * 8L, kPolyBytes);
      m.barrier();
      for (int w = 0; w < 8; ++w) m.rd(w, LdsModel::KEY + rs::duo_xchg_doubles(rs::duo_partner(w)) * 8L, kPolyBytes);
      if (!(broken == 2 && round == 0)) m.barrier();
    }
    if (broken != 1) issue_next();
  }
  return m.conflicts();
}
// blind_rotate_wgs_kernel<WPB>: three 16 KB slots, half-row h in slot h mod 3, requested two half-rows ahead
long model_wgs(int WPB, int L, int broken) {
  LdsModel m;
  const long slot_bytes = 16 * kChunkBytes;
  const int chunks = 16 / WPB, slots = broken == 1 ? 2 : 3;
  const long total = 2L * 2 * L * 2;                        // two steps
  long h_issue = 0;
  auto issue_next = [&] {   // request of half-row x: in flight until the barrier that publishes x, i.e. this epoch and the next
    if (h_issue >= total) return;
    const int sl = slots == 3 ? rs::wgs_ring_slot(h_issue) : (int)(h_issue % 2);
    for (int w = 0; w < WPB; ++w) m.dma(w, LdsModel::KEY + sl * slot_bytes + w * chunks * kChunkBytes, chunks * kChunkBytes, m.epoch, m.epoch + (h_issue < 2 ? (int)h_issue : 1));
    ++h_issue;
  };
  issue_next();
  issue_next();
  for (long h = 0; h < total; ++h) {
    for (int w = 0; w < WPB; ++w) m.rw(w, buf_of(w), 576 * 8L);
    m.barrier();                                             // publish(h): own share landed, h + 1 may still be in flight
    issue_next();                                            // h + 2 into the slot of h - 1
    const int sl = slots == 3 ? rs::wgs_ring_slot(h) : (int)(h % 2);
    for (int w = 0; w < WPB; ++w) m.rd(w, LdsModel::KEY + sl * slot_bytes, slot_bytes);
  }
  return m.conflicts();
}
// blind_rotate_wg_kernel<8>: rows in pairs through two slots; barrier 1 publishes the pair, barrier 2 frees it
long model_wg(int L, int broken) {
  LdsModel m;
  const long slot_bytes = 16 * kChunkBytes;
  long row = 0;
  auto issue_pair = [&] {
    for (int k = 0; k < 2; ++k, ++row)
      for (int w = 0; w < 8; ++w) m.dma(w, LdsModel::KEY + rs::wg_ring_slot(row) * slot_bytes + w * 2 * kChunkBytes, 2 * kChunkBytes, m.epoch, m.epoch);
  };
  issue_pair();
  for (int pair = 0; pair < 2 * L; ++pair) {                 // two steps of 2l rows
    for (int w = 0; w < 8; ++w) m.rw(w, buf_of(w), 576 * 8L);
    m.barrier();
    for (int w = 0; w < 8; ++w) m.rd(w, LdsModel::KEY, 2 * slot_bytes);
    if (broken != 2) m.barrier();
    issue_pair();
  }
  return m.conflicts();
}
}  // namespace

extern "C" {

long rs_emu_gen_wave_region_violations(int logn) {
  switch (logn) {
    case 10: return gen_wave_region_violations_xp<10, 0>();
    case 11: return gen_wave_region_violations_xp<11, 0>();
    case 12: return gen_wave_region_violations_xp<12, 0>();
    case 13: return gen_wave_region_violations_xp<13, 0>();
  }
  return -1;
}

// number of mismatches between (a) the literal twiddles of stages 0-2 and the generated table,
// (b) odd-indexed table entries and i times their even sibling -- both must be 0
int rs_emu_fft_twiddle_check() {
  std::vector<double> tw = rs::make_fft_tables();
  int bad = 0;
  const int lit_idx[4] = {1, 2, 4, 6};
  for (int e = 0; e < 4; ++e) {
    const int pos = rs::ftw_pos(lit_idx[e]);
    bad += tw[2 * pos] != rs::kFftTwU[2 * e];
    bad += tw[2 * pos + 1] != rs::kFftTwU[2 * e + 1];
  }
  for (int idx = 2; idx < rs::kM; idx += 2) {
    const int pe = rs::ftw_pos(idx), po = rs::ftw_pos(idx + 1);
    bad += tw[2 * po] != -tw[2 * pe + 1];
    bad += tw[2 * po + 1] != tw[2 * pe];
  }
  return bad;
}

// table entries 1, 2, 4, 6 of every general ring against the literals pass 0 uses instead (rs_general.h, gen_pass_tw): mismatches
int rs_emu_gen_literal_twiddle_check() {
  int bad = 0;
  const int idx[4] = {1, 2, 4, 6};
  for (int logn = rs::kGenMinLogN; logn <= rs::kGenMaxLogN; ++logn) {
    std::vector<double> tw((size_t)1 << logn);
    rs::gen_make_twiddles(logn, tw.data());
    for (int e = 0; e < 4; ++e) bad += tw[2 * idx[e]] != rs::kFftTwU[2 * e] || tw[2 * idx[e] + 1] != rs::kFftTwU[2 * e + 1];
  }
  return bad;
}

// selects the exchange form emulated by the FFT entry points (0 interleaved, 1 planar)
void rs_emu_set_planar(int on) { g_planar = on; }

// FFT-mode product of a small polynomial with a torus polynomial; returns the largest distance to
// the nearest integer seen before rounding in *max_dev.
int rs_emu_polymul_fft(const int32_t* a_small, const int32_t* b_torus, int32_t* out, double* max_dev) {
  std::vector<double> tw = rs::make_fft_tables();
  std::vector<double> buf(rs::kBufDoubles), bkd(kN);
  emu_fft_key_transform(b_torus, bkd.data(), tw.data(), buf.data());
  Wave w, s;
  std::memset(&s, 0, sizeof s);
  for (int l = 0; l < kLanes; ++l)
    for (int r = 0; r < kRegs; ++r) w.x[l][r] = (double)a_small[l + 64 * r];
  emu_fft_forward(w, tw.data(), buf.data());
  for (int l = 0; l < kLanes; ++l)
    for (int v = 0; v < 8; ++v) {
      const size_t k = ((size_t)v * 64 + l) * 2;
      rs::fft_cmac(s.x[l][v], s.x[l][v + 8], w.x[l][v], w.x[l][v + 8], bkd[k], bkd[k + 1]);
    }
  emu_fft_inverse(s, tw.data(), buf.data());
  double dev = 0.0;
  for (int l = 0; l < kLanes; ++l)
    for (int r = 0; r < kRegs; ++r) out[l + 64 * r] = rs::fft_round_torus32(s.x[l][r], dev);
  if (max_dev) *max_dev = dev;
  return 0;
}

int rs_emu_blind_rotate_fft(int cfg, int n, const int32_t* in0, const int32_t* in1, int32_t c0, int32_t c1, int32_t bconst, int32_t mu,
                            const int32_t* bk, int32_t* u_out, int32_t* acc_out, int steps, double* max_dev) {
  return cfg == 0 ? emu_blind_rotate_fft<rs::CfgDefault128>(n, in0, in1, c0, c1, bconst, mu, bk, u_out, acc_out, steps, max_dev)
                  : emu_blind_rotate_fft<rs::CfgRedsecV2>(n, in0, in1, c0, c1, bconst, mu, bk, u_out, acc_out, steps, max_dev);
}


// cfg: 0 = l=3/Bgbit=7, 1 = l=10/Bgbit=3
int rs_emu_polymul(int cfg, const int32_t* a_small, const int32_t* b_torus, int32_t* out) {
  return cfg == 0 ? emu_polymul<rs::CfgDefault128>(a_small, b_torus, out) : emu_polymul<rs::CfgRedsecV2>(a_small, b_torus, out);
}

int rs_emu_blind_rotate(int cfg, int n, const int32_t* in0, const int32_t* in1, int32_t c0, int32_t c1, int32_t bconst, int32_t mu,
                        const int32_t* bk, int32_t* u_out, int32_t* acc_out, int steps) {
  return cfg == 0 ? emu_blind_rotate<rs::CfgDefault128>(n, in0, in1, c0, c1, bconst, mu, bk, u_out, acc_out, steps)
                  : emu_blind_rotate<rs::CfgRedsecV2>(n, in0, in1, c0, c1, bconst, mu, bk, u_out, acc_out, steps);
}

// Returns 0 if the reduction schedule of cfg is provably exact for its prime, else -1 (msg filled).
int rs_emu_validate(int cfg, char* msg, int msg_len) {
  rs::PrimeSpec ps;
  const int l = cfg == 0 ? 3 : 10, bg = cfg == 0 ? 7 : 3;
  if (!rs::prime_for(l, bg, &ps)) return -1;
  const unsigned fm = cfg == 0 ? rs::CfgDefault128::FWD_MASK : rs::CfgRedsecV2::FWD_MASK;
  const unsigned im = cfg == 0 ? rs::CfgDefault128::INV_MASK : rs::CfgRedsecV2::INV_MASK;
  const int fuse = cfg == 0 ? rs::CfgDefault128::FUSE : rs::CfgRedsecV2::FUSE;
  const bool mid = cfg == 0 ? rs::CfgDefault128::MID_REDUCE : rs::CfgRedsecV2::MID_REDUCE;
  std::string why = rs::validate_schedule((double)ps.p, l, bg, fm, im, fuse, mid);
  if (msg && msg_len > 0) { std::strncpy(msg, why.c_str(), (size_t)msg_len - 1); msg[msg_len - 1] = 0; }
  return why.empty() ? 0 : -1;
}

// Largest |intermediate| / 2^53 seen while transforming worst-case inputs is not observable from
// outside; instead expose the raw forward transform for property tests:
// out[16*lane+u] layout C values (doubles) of the forward transform of `poly`.
int rs_emu_forward(int cfg, const int32_t* poly, double* out) {
  rs::PrimeSpec ps;
  const int l = cfg == 0 ? 3 : 10, bg = cfg == 0 ? 7 : 3;
  if (!rs::prime_for(l, bg, &ps)) return -1;
  rs::Tables t = rs::make_tables(ps, cfg == 0 ? rs::CfgDefault128::FUSE : rs::CfgRedsecV2::FUSE);
  std::vector<double> buf(rs::kBufDoubles);
  Wave w;
  for (int lane = 0; lane < kLanes; ++lane)
    for (int r = 0; r < kRegs; ++r) w.x[lane][r] = (double)poly[lane + 64 * r];
  if (cfg == 0) emu_forward<rs::CfgDefault128>(w, t.tw.data(), buf.data(), t.f);
  else emu_forward<rs::CfgRedsecV2>(w, t.tw.data(), buf.data(), t.f);
  for (int lane = 0; lane < kLanes; ++lane)
    for (int u = 0; u < kRegs; ++u) out[16 * lane + u] = w.x[lane][u];
  return 0;
}

// Fused-digit forward transform (fwd_F1_digits path) of gadget digit q of the coefficients `coef`;
// out as rs_emu_forward. Must agree mod p with the generic transform of the digit polynomial.
int rs_emu_forward_digits(int cfg, const int32_t* coef, int q, double* out) {
  rs::PrimeSpec ps;
  const int l = cfg == 0 ? 3 : 10, bg = cfg == 0 ? 7 : 3;
  if (!rs::prime_for(l, bg, &ps)) return -1;
  rs::Tables t = rs::make_tables(ps, cfg == 0 ? rs::CfgDefault128::FUSE : rs::CfgRedsecV2::FUSE);
  std::vector<double> buf(rs::kBufDoubles);
  Wave w;
  static int32_t d[kLanes][kRegs];
  for (int lane = 0; lane < kLanes; ++lane)
    for (int r = 0; r < kRegs; ++r) d[lane][r] = coef[lane + 64 * r];
  if (cfg == 0) emu_forward_digits<rs::CfgDefault128>(w, d, q, rs::gadget_offset<rs::CfgDefault128>(), t.tw.data(), buf.data(), t.f);
  else emu_forward_digits<rs::CfgRedsecV2>(w, d, q, rs::gadget_offset<rs::CfgRedsecV2>(), t.tw.data(), buf.data(), t.f);
  for (int lane = 0; lane < kLanes; ++lane)
    for (int u = 0; u < kRegs; ++u) out[16 * lane + u] = w.x[lane][u];
  return 0;
}

// Number of inputs d = start + t * step (t < count, mod 2^32) for which the one-instruction digit
// (gadget_prepare + gadget_digit_prepared, FFT-mode kernels) differs from TFHE's formula (gadget_digit).
long rs_emu_digit_mismatches(int cfg, uint32_t start, uint32_t step, long count) {
  long bad = 0;
  uint32_t d = start;
  for (long t = 0; t < count; ++t, d += step) {
    if (cfg == 0) {
      using C = rs::CfgDefault128;
      const int32_t dx = rs::gadget_prepare<C>((int32_t)d);
      for (int q = 0; q < C::L; ++q) bad += rs::gadget_digit_prepared<C>(dx, q) != rs::gadget_digit<C>((int32_t)d, q, rs::gadget_offset<C>());
    } else {
      using C = rs::CfgRedsecV2;
      const int32_t dx = rs::gadget_prepare<C>((int32_t)d);
      for (int q = 0; q < C::L; ++q) bad += rs::gadget_digit_prepared<C>(dx, q) != rs::gadget_digit<C>((int32_t)d, q, rs::gadget_offset<C>());
    }
  }
  return bad;
}

uint64_t rs_emu_prime(int cfg) {
  rs::PrimeSpec ps;
  if (!rs::prime_for(cfg == 0 ? 3 : 10, cfg == 0 ? 7 : 3, &ps)) return 0;
  return ps.p;
}


// General ring path: split-key product through the device's own pass / exchange functions (rs_general.h)
int rs_emu_gen_polymul(int logn, const int32_t* a_small, const int32_t* b_torus, int32_t* out, double* max_dev) {
  switch (logn) {
    case 10: return GenEmu<10>().polymul(a_small, b_torus, out, max_dev);
    case 11: return GenEmu<11>().polymul(a_small, b_torus, out, max_dev);
    case 12: return GenEmu<12>().polymul(a_small, b_torus, out, max_dev);
    case 13: return GenEmu<13>().polymul(a_small, b_torus, out, max_dev);
  }
  return -1;
}
long rs_emu_gen_layout_violations(int logn) {
  switch (logn) {
    case 10: return GenEmu<10>::layout_violations<0>();
    case 11: return GenEmu<11>::layout_violations<0>();
    case 12: return GenEmu<12>::layout_violations<0>();
    case 13: return GenEmu<13>::layout_violations<0>();
  }
  return -1;
}
long rs_emu_plane_layout_violations() {
  return plane_violations<rs::kLayA, rs::kLayB, 1>() + plane_violations<rs::kLayB, rs::kLayA, 1>() +
         plane_violations<rs::kLayB, rs::kLayC, 2>() + plane_violations<rs::kLayC, rs::kLayB, 2>();
}
double rs_emu_gen_error_bound(int logn, int l, int bgbit) { return rs::gen_error_bound(logn, l, bgbit); }
// the copy plan of rs_allgather_rows: rows of (dst, src, round, lo, hi); returns the number of copies (out may be null)
long rs_emu_exchange_schedule(long rows, int n, long* out) {
  const std::vector<rs::SliceCopy> plan = rs::exchange_schedule((size_t)rows, n);
  if (out) for (size_t i = 0; i < plan.size(); ++i) {
    out[5 * i] = plan[i].dst; out[5 * i + 1] = plan[i].src; out[5 * i + 2] = plan[i].round; out[5 * i + 3] = (long)plan[i].lo; out[5 * i + 4] = (long)plan[i].hi;
  }
  return (long)plan.size();
}
// form: 0 coop<2>, 1 coop<4>, (2 / 3: the s_part exchange form of coop8, removed in round 5) 4 coops<2>, 5 coops<4>, 6 duo, 7 duos,
//       8 wgs<8>, 9 wgs<4>, 10 wg, 11 / 12 coop8 as shipped (sums by LDS atomics; l = 10 / 3)
// The tiled keyswitch kernels (rs_kernels.hip), four waves. Every wave touches the whole of each LDS table, so all that keeps the
// protocol sound is which barrier separates which phase:
//   per-digit kernel (comb = false): group g looks up s_ksk[g & 1]; the next group's rows are stored into s_ksk[(g + 1) & 1]
//     AFTER the lookups and before the group's one barrier (broken 1: into the buffer being read; broken 2: no barrier);
//   combined-digit kernel (comb = true): lookups read s_tab, then the next base rows go into s_base, barrier, the next sums are
//     built s_base -> s_tab, barrier (broken 1: sums built before the first barrier, i.e. while other waves still look up;
//     broken 2: second barrier missing, lookups of the next group race with the build).
long model_keyswitch(bool comb, int broken) {
  LdsModel m;
  const long base = LdsModel::KEY, tab = LdsModel::PART, bytes = 16384;
  auto buf = [&](int b) { return base + b * 0x100000L; };
  for (int g = 0; g < 3; ++g) {
    if (!comb) {
      for (int w = 0; w < 4; ++w) m.rd(w, buf(g & 1), bytes);                                   // lookups
      for (int w = 0; w < 4; ++w) m.wr(w, buf(broken == 1 ? (g & 1) : ((g + 1) & 1)) + w * 4096, 4096);   // next rows, this wave's share
      if (broken != 2) m.barrier();
    } else {
      for (int w = 0; w < 4; ++w) m.rd(w, tab, bytes);                                          // lookups
      for (int w = 0; w < 4; ++w) m.wr(w, base + w * 4096, 4096);                               // next base rows
      if (broken == 1) for (int w = 0; w < 4; ++w) { m.rd(w, base, bytes); m.wr(w, tab + w * 4096, 4096); }
      m.barrier();
      if (broken != 1) for (int w = 0; w < 4; ++w) { m.rd(w, base, bytes); m.wr(w, tab + w * 4096, 4096); }   // sums of the next group
      if (broken != 2) m.barrier();
    }
  }
  return m.conflicts();
}
long rs_emu_lds_protocol_conflicts(int form, int broken) {
  switch (form) {
    case 0: return model_coop(2, broken);
    case 1: return model_coop(4, broken);
    case 4: return model_coops<2>(broken);
    case 5: return model_coops<4>(broken);
    case 6: return model_duo(10, broken);
    case 7: return model_duos(10, broken);
    case 8: return model_wgs(8, 3, broken);
    case 9: return model_wgs(4, 10, broken);
    case 10: return model_wg(3, broken);
    case 11: return model_coop8_atomics(10, broken);
    case 12: return model_coop8_atomics(3, broken);
    case 13: return model_keyswitch(false, broken);
    case 14: return model_keyswitch(true, broken);
  }
  return -1;
}
// coop8: every digit row of both components belongs to exactly one wave; the SIMDs (waves s and s + 4) carry totals within one
// row of each other; on no SIMD does the younger wave (s + 4) carry more rows than the older one (rs_lds_plan.h: it would finish last)
long rs_emu_coop8_row_split_violations(int L) {
  long bad = 0;
  std::vector<int> owner(2 * L, 0);
  for (int w = 0; w < rs::kCoop8Waves; ++w)
    for (int r = 0; r < rs::coop8_row_count(L, w); ++r) {
      const int q = rs::coop8_row_first(L, w) + r;
      if (q < 0 || q >= L) { ++bad; continue; }
      ++owner[rs::coop8_comp(L, w) * L + q];
    }
  for (int v : owner) bad += v != 1;
  int lo = 1 << 30, hi = 0;
  for (int s = 0; s < 4; ++s) {
    const int older = rs::coop8_row_count(L, s), younger = rs::coop8_row_count(L, s + 4);
    bad += rs::coop8_by_age(L) && younger > older;
    lo = std::min(lo, older + younger); hi = std::max(hi, older + younger);
  }
  bad += hi - lo > 1;
  bad += (rs::coop8_inv_a(L) & 3) == (rs::coop8_inv_b(L) & 3);      // the two inverse transforms on different SIMDs
  for (int w = 0; w < rs::kCoop8Waves; ++w) bad += rs::coop8_row_count(L, w) < rs::coop8_row_count(L, rs::coop8_inv_a(L)) || rs::coop8_row_count(L, w) < rs::coop8_row_count(L, rs::coop8_inv_b(L));
  return bad;
}

// coop8, listed step: the 512 threads' shares of the shared rotated difference (rs_lds_plan.h: coop8_diff_comp / coop8_diff_coeff)
// cover every coefficient of both components exactly once, and a wave writes only inside its component
long rs_emu_coop8_diff_cover_violations() {
  long bad = 0;
  std::vector<int> hits(2 * kN, 0);
  for (int t = 0; t < 64 * rs::kCoop8Waves; ++t)
    for (int m = 0; m < rs::kCoop8DiffPerThread; ++m) {
      const int c = rs::coop8_diff_comp(t >> 6), j = rs::coop8_diff_coeff(t, m);
      if (c < 0 || c > 1 || j < 0 || j >= kN) { ++bad; continue; }
      ++hits[c * kN + j];
    }
  for (int v : hits) bad += v != 1;
  return bad;
}

// keyswitch with combined digits: for the word `aibar` and a (t, basebit, D) shape, the number of (group, k) positions whose
// digit, recovered from the group's row index, differs from the digit the per-digit kernel extracts (must be 0), plus groups whose
// row index leaves the table
long rs_emu_ks_comb_violations(uint32_t aibar, int t, int basebit, int D) {
  long bad = 0;
  const int NG = (t + D - 1) / D, DL = t - (NG - 1) * D;
  for (int gq = 0; gq < NG; ++gq) {
    const int dl = gq == NG - 1 ? DL : D;
    const uint32_t comb = rs::ks_comb_index(aibar, gq, D, dl, basebit);
    bad += comb >= (1u << (basebit * dl));
    for (int k = 0; k < dl; ++k) bad += (uint32_t)rs::ks_comb_digit((int)comb, k, dl, basebit) != rs::ks_digit(aibar, gq * D + k, basebit);
  }
  return bad;
}
// slices of a small-batch keyswitch launch and the scratch they need (rs_host.h)
long rs_emu_keyswitch_slices(long B, int W, int N) { return (long)rs::keyswitch_slices(B, W, N); }
long rs_emu_keyswitch_scratch_words(long B, int W, int N) { return (long)rs::keyswitch_scratch_words_for(B, W, N); }
// form of a keyswitch launch (rs_host.h keyswitch_form): form + 16 * slices; force = -1 (by batch size), 1 (never wide), 3 (wide)
long rs_emu_keyswitch_form(long B, int W, int N, int t, int basebit, int num_cus, int force) {
  const rs::KsPlan p = rs::keyswitch_form(B, W, N, t, basebit, num_cus, force);
  return (long)p.form + 16L * (long)p.slices;
}
// the operation list of rs_allgather_rows for n contexts on `devices`, peer[d * n + s] = direct access allowed; rows of
// (kind, ctx, other, path, lo, hi); returns the number of operations (out may be null)
long rs_emu_exchange_plan(long rows, int n, const int* devices, const unsigned char* peer, int force_staged, long* out) {
  const std::vector<rs::ExchangeOp> ops = rs::exchange_plan((size_t)rows, n, devices, peer, force_staged != 0);
  if (out) for (size_t i = 0; i < ops.size(); ++i) {
    out[6 * i] = ops[i].kind; out[6 * i + 1] = ops[i].ctx; out[6 * i + 2] = ops[i].other; out[6 * i + 3] = ops[i].path;
    out[6 * i + 4] = (long)ops[i].lo; out[6 * i + 5] = (long)ops[i].hi;
  }
  return (long)ops.size();
}
// the launches of a blind-rotation batch (rs_launch_plan.h). traits: (workgroup_form, L, coop4, listed_cfg, split); switches: bits, in
// this order, of no_coop, no_wg, no_duo, no_persist, no_wg4, no_tail, no_coop8, no_coop8_listed, no_cohort. out: the reported
// (form, waves, resident), then per step (form, waves, grid, block, first, rows, persistent, cohort, every, lag); returns the steps
long rs_emu_launch_plan(const int* traits, int n, long B, int num_cus, unsigned switches, int cohort_table_offered, long* out) {
  const rs::FormTraits t{traits[0] != 0, traits[1], traits[2] != 0, traits[3], traits[4] != 0};
  rs::LaunchOpts o;
  bool* const bits[9] = {&o.no_coop, &o.no_wg, &o.no_duo, &o.no_persist, &o.no_wg4, &o.no_tail, &o.no_coop8, &o.no_coop8_listed, &o.no_cohort};
  for (int k = 0; k < 9; ++k) *bits[k] = (switches >> k) & 1;
  const rs::LaunchPlan p = rs::plan_blind_rotate(t, n, B, num_cus, o, cohort_table_offered != 0);
  out[0] = p.info.form; out[1] = p.info.waves_per_block; out[2] = p.info.resident;
  for (int k = 0; k < p.steps; ++k) {
    const rs::LaunchStep& s = p.step[k];
    const long row[10] = {s.form, s.waves, s.grid, s.block, s.first, s.rows, s.persistent, s.cohort, s.cohort_every, s.cohort_lag};
    std::copy(row, row + 10, out + 3 + 10 * k);
  }
  return p.steps;
}
// measured transform errors (see GenEmu::transform_error_ratios) and the analysis' per-transform bounds g_f - 1, g_i - 1
int rs_emu_gen_transform_errors(int logn, uint64_t seed, int amplitude, double* measured2, double* bounds2) {
  const double u = std::ldexp(1.0, -53), r2 = std::sqrt(2.0);
  bounds2[0] = std::pow(1.0 + 8.3 * u / r2, logn - 1) - 1.0;
  bounds2[1] = std::pow(1.0 + 5.8 * u / r2, logn - 1) - 1.0;
  switch (logn) {
    case 10: { GenEmu<10> e; e.transform_error_ratios(seed, amplitude, measured2); return 0; }
    case 11: { GenEmu<11> e; e.transform_error_ratios(seed, amplitude, measured2); return 0; }
    case 12: { GenEmu<12> e; e.transform_error_ratios(seed, amplitude, measured2); return 0; }
    case 13: { GenEmu<13> e; e.transform_error_ratios(seed, amplitude, measured2); return 0; }
  }
  return -1;
}
// run-time gadget digits of the general path against TFHE's formula
long rs_emu_gen_digit_mismatches(int l, int bgbit, uint32_t start, uint32_t step, long count) {
  long bad = 0;
  const uint32_t off = rs::gen_gadget_offset(l, bgbit);
  uint32_t d = start;
  for (long t = 0; t < count; ++t, d += step) {
    const int32_t dx = rs::gen_gadget_prepare((int32_t)d, off);
    for (int q = 0; q < l; ++q) {
      const int decal = 32 - (q + 1) * bgbit;
      const int32_t want = (int32_t)(((d + off) >> decal) & ((1u << bgbit) - 1u)) - (1 << (bgbit - 1));
      bad += rs::gen_gadget_digit(dx, q, bgbit) != want;
    }
  }
  return bad;
}

// the random streams of key generation (rs_keygen.h), for the bit-exact comparison with redsec_amd/keygen.py
void rs_emu_chacha_block(const uint32_t* key8, uint32_t domain, uint64_t row, uint32_t block, uint32_t* out16) {
  uint32_t key[8], out[16];
  for (int k = 0; k < 8; ++k) key[k] = key8[k];
  rs::kg_chacha_block(key, domain, row, block, out);
  for (int k = 0; k < 16; ++k) out16[k] = out[k];
}
void rs_emu_keygen_uniforms(const uint32_t* w4, double* u1u2) {
  u1u2[0] = rs::kg_u1(w4[0], w4[1]);
  u1u2[1] = rs::kg_u2(w4[2], w4[3]);
}
int32_t rs_emu_keygen_noise(const uint32_t* w4, double sigma) { return rs::kg_noise32(w4[0], w4[1], w4[2], w4[3], sigma); }

// expansion of a compressed key (rs_expand_keys_dev) through the device functions its kernels call, lane by lane: one bk row
// (expand_bk_kernel: thread t of N / 16 stores mask block t, the body is copied word t + T r) -> out[2][N]
void rs_emu_expand_bk_row(const uint8_t* mask_seed, int N, uint64_t row, const int32_t* body_row, int32_t* out) {
  uint32_t key[8];
  rs::kg_seed_words(mask_seed, key);
  const int T = N / 16;
  for (int t = 0; t < T; ++t) {
    uint32_t w[16];
    rs::kg_bk_mask_block(key, row, t, w);
    for (int k = 0; k < 16; ++k) out[16 * t + k] = (int32_t)w[k];
    for (int r = 0; r < 16; ++r) out[N + t + T * r] = body_row[t + T * r];
  }
}
// one ksk sample s (expand_ksk_kernel: the 64 lanes of a wave, chunk by chunk through the LDS transpose) -> out[n + 1]
void rs_emu_expand_ksk_sample(const uint8_t* mask_seed, int n, int basebit, uint64_t s, int32_t body, int32_t* out) {
  if ((s & ((1ull << basebit) - 1)) == 0) {
    for (int k = 0; k <= n; ++k) out[k] = 0;
    return;
  }
  uint32_t key[8];
  rs::kg_seed_words(mask_seed, key);
  std::vector<uint32_t> buf(rs::kKgChunk);
  for (int k0 = 0; k0 < n; k0 += rs::kKgChunk) {
    for (int lane = 0; lane < 64; ++lane) {
      uint32_t w[16] = {};
      rs::kg_ksk_mask_block(key, s, k0, lane, n, w);
      for (int q = 0; q < 16; ++q) buf[16 * lane + q] = w[q];
    }
    for (int q = 0; q < 16; ++q)
      for (int lane = 0; lane < 64; ++lane) {
        const int idx = rs::kg_ksk_chunk_word(q, lane), k = k0 + idx;
        if (k < n) out[k] = (int32_t)buf[idx];
      }
  }
  out[n] = body;
}

// seeded ciphertexts (rs_encrypt_seeded_dev / rs_expand_ciphertexts_dev) through the functions and the placement of
// seeded_lwe_kernel, thread by thread: tiles of kg_ct_tile(n) ciphertexts, the flat (ciphertext, block) items in strides of
// kCtThreads, the LDS staging of kg_ct_lds_word, per-ciphertext sums, then the tile stored as one contiguous span.
// encrypt: lwe_key int32[n] 0/1, mu[B] -> body[B] and ct[B][n+1] (ct may be null); expand: body[B] -> ct[B][n+1]
static void emu_seeded(bool encrypt, const uint8_t* mask_seed, const uint8_t* noise_seed, int n, uint64_t first, long B,
                       const int32_t* mu, const int32_t* lwe_key, double sigma, int32_t* body, int32_t* ct) {
  uint32_t key[8], nkey[8] = {};
  rs::kg_seed_words(mask_seed, key);
  if (encrypt) rs::kg_seed_words(noise_seed, nkey);
  const int C = rs::kg_ct_tile(n), nblk = rs::kg_ct_blocks(n);
  std::vector<uint32_t> bits((size_t)(n + 31) / 32, 0u), acc((size_t)C), lds((size_t)C * (n + 1));
  for (int i = 0; encrypt && i < n; ++i) bits[(size_t)i >> 5] |= (uint32_t)(lwe_key[i] & 1) << (i & 31);
  for (long i0 = 0; i0 < B; i0 += C) {
    const int cnt = (int)std::min<long>(C, B - i0);
    for (int t = 0; t < cnt; ++t) {
      if (encrypt) acc[t] = 0u;
      else lds[rs::kg_ct_lds_word(t, n, n)] = (uint32_t)body[i0 + t];
    }
    for (int t = 0; t < rs::kCtThreads; ++t)
      for (int it = t; it < cnt * nblk; it += rs::kCtThreads) {
        const int c = it / nblk, blk = it - c * nblk;
        uint32_t w[16];
        rs::kg_ct_mask_block(key, first + (uint64_t)(i0 + c), blk, w);
        for (int q = 0; q < 16; ++q)
          if (16 * blk + q < n) lds[rs::kg_ct_lds_word(c, 16 * blk + q, n)] = w[q];
        if (encrypt) {
          const uint32_t kb = rs::kg_ct_key_bits(bits.data(), blk);
          for (int q = 0; q < 16; ++q) acc[c] += ((kb >> q) & 1u) ? w[q] : 0u;
        }
      }
    for (int t = 0; encrypt && t < cnt; ++t) {
      const uint32_t b = acc[t] + (uint32_t)rs::kg_ct_noise(nkey, first + (uint64_t)(i0 + t), sigma) + (uint32_t)mu[i0 + t];
      body[i0 + t] = (int32_t)b;
      lds[rs::kg_ct_lds_word(t, n, n)] = b;
    }
    if (ct)
      for (int j = 0; j < cnt * (n + 1); ++j) ct[i0 * (n + 1) + j] = (int32_t)lds[j];
  }
}
void rs_emu_encrypt_seeded(const uint8_t* mask_seed, const uint8_t* noise_seed, int n, uint64_t first, long B, const int32_t* mu,
                           const int32_t* lwe_key, double sigma, int32_t* body, int32_t* ct) {
  emu_seeded(true, mask_seed, noise_seed, n, first, B, mu, lwe_key, sigma, body, ct);
}
void rs_emu_expand_ciphertext(const uint8_t* mask_seed, int n, uint64_t first, long B, const int32_t* body, int32_t* ct) {
  emu_seeded(false, mask_seed, nullptr, n, first, B, nullptr, nullptr, 0.0, const_cast<int32_t*>(body), ct);
}
int rs_emu_ct_tile(int n) { return rs::kg_ct_tile(n); }

// public-key encryption (rs_pk_encrypt_dev): the selection words of ciphertext row `row` through kg_pk_select_block, chunk by chunk
// as pk_encrypt_kernel walks them -> words_out[ceil(m / 32)] (bit j of the ciphertext = bit j & 31 of word j >> 5; bits at j >= m of
// the last word are whatever the stream holds), and the kernel's tile of ciphertexts
void rs_emu_pk_select(const uint8_t* seed, uint64_t row, long m, uint32_t* words_out) {
  uint32_t key[8];
  rs::kg_seed_words(seed, key);
  const long words = (m + 31) / 32;
  for (long j0 = 0; j0 < m; j0 += rs::kPkChunk) {
    uint32_t w[16];
    rs::kg_pk_select_block(key, row, (uint32_t)(j0 / rs::kPkChunk), w);
    for (int q = 0; q < 16 && j0 / 32 + q < words; ++q) words_out[j0 / 32 + q] = w[q];
  }
}
int rs_emu_pk_tile() { return rs::kPkTile; }

// ---- compact RLWE public keys (rs_rlwe_pk_encrypt_dev, rs_rlwe_extract_dev) through the functions of rs_rlwe.h ----
// the selector words of ciphertext row `row` through rl_select_block, block by block as rlwe_pk_encrypt_kernel stages them
// -> words_out[N / 32] (u_k = bit k & 31 of word k >> 5)
void rs_emu_rlwe_select(const uint8_t* seed, uint64_t row, int N, uint32_t* words_out) {
  uint32_t key[8];
  rs::kg_seed_words(seed, key);
  for (int blk = 0; blk < N / 512; ++blk) {
    uint32_t w[16];
    rs::rl_select_block(key, row, (uint32_t)blk, w);
    for (int q = 0; q < 16; ++q) words_out[16 * blk + q] = w[q];
  }
}
int rs_emu_rlwe_term_index(int N, int k, int j) { return rs::rl_term_index(N, k, j); }
// source index in the mask polynomial of word j < N of the sample of coefficient c; *negate: the word is the negated coefficient
int rs_emu_rlwe_extract_word(int N, int c, int j, int* negate) {
  bool neg;
  const int idx = rs::rl_extract_index(N, c, j, neg);
  *negate = neg ? 1 : 0;
  return idx;
}
int rs_emu_rlwe_tile() { return rs::kRlTile; }
// rlwe_pk_encrypt_kernel, workgroup by workgroup and thread by thread as the kernel places them: the window of ext = (-p, p) a tile
// stages, one 4-word chunk per thread and four selector bits, the masked adds on the seven live words, noise and message at the store
void rs_emu_rlwe_pk_encrypt(const int32_t* pk, const int32_t* mu, long count, int N, const uint8_t* seed, uint64_t first, double sigma,
                            int32_t* rlwe) {
  uint32_t key[8];
  rs::kg_seed_words(seed, key);
  const long R = (count + N - 1) / N;
  const int tiles = N / rs::kRlTile;
  std::vector<uint32_t> win((size_t)N + rs::kRlTile), sel((size_t)N / 32);
  for (long blk = 0; blk < R * 2 * tiles; ++blk) {
    const int tile = (int)(blk % tiles), poly = (int)((blk / tiles) & 1);
    const long r = blk / (2 * tiles);
    const int k0 = tile * rs::kRlTile;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(pk) + (size_t)poly * N;
    for (int i = 0; i < N + rs::kRlTile; ++i) win[i] = rs::rl_ext_word(p, N, k0 + i);
    rs_emu_rlwe_select(seed, first + (uint64_t)r, N, sel.data());
    for (int t = 0; t < rs::kRlThreads; ++t) {
      uint32_t acc[rs::kRlKpt] = {0u, 0u, 0u, 0u};
      int c4 = t + N / 4;
      const uint32_t* hi = &win[4 * (size_t)c4];
      for (int wd = 0; wd < N / 32; ++wd)
        for (int g = 0; g < 8; ++g) {
          const uint32_t* lo = &win[4 * (size_t)(--c4)];
          const uint32_t w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          for (int b = 0; b < 4; ++b) {
            const uint32_t m = 0u - ((sel[wd] >> (4 * g + b)) & 1u);
            for (int q = 0; q < rs::kRlKpt; ++q) acc[q] += w[4 + q - b] & m;
          }
          hi = lo;
        }
      const int k = k0 + rs::kRlKpt * t;
      int32_t e[4];
      rs::rl_noise4(key, first + (uint64_t)r, poly, N, k, sigma, e);
      for (int q = 0; q < rs::kRlKpt; ++q) {
        uint32_t v = acc[q] + (uint32_t)e[q];
        const long i = r * (long)N + k + q;
        if (poly == 1 && i < count) v += (uint32_t)mu[i];
        rlwe[((size_t)r * 2 + poly) * N + k + q] = (int32_t)v;
      }
    }
  }
}
// rlwe_extract_kernel: rlwe [ceil(count / N)][2][N] -> u [count][N+1]
void rs_emu_rlwe_extract(const int32_t* rlwe, long count, int N, int32_t* u) {
  for (long i = 0; i < count; ++i) {
    const long r = i / N;
    const int c = (int)(i - r * N);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(rlwe) + (size_t)r * 2 * N;
    for (int j = 0; j <= N; ++j) u[(size_t)i * (N + 1) + j] = (int32_t)rs::rl_extract_word(a, a + N, N, c, j);
  }
}

// ---- packed results (rs_pack_dev) through the functions of rs_pack.h ----
uint32_t rs_emu_pack_offset(int basebit, int t) { return rs::pa_offset(basebit, t); }
uint32_t rs_emu_pack_digit(uint32_t abar, int basebit, int j) { return rs::pa_digit(abar, basebit, j); }
int rs_emu_pack_slot_blocks(long count, int N) { return rs::pa_slot_blocks(count, N); }
int rs_emu_pack_chunks(int n) { return rs::pa_chunks(n); }
long rs_emu_pack_groups(long count, int n, int N) { return rs::pa_groups(count, n, N); }
// window word of coefficient k0 + x and slot c0 + cc as an index into ext = (-p, p)
int rs_emu_pack_window_word(int N, int k0, int c0, int cpad, int x, int cc) {
  return rs::pa_window_base(N, k0, c0, cpad) + rs::pa_window_index(cpad, x, cc);
}
int rs_emu_pack_tile() { return rs::kPaTile; }
int rs_emu_pack_slots() { return rs::kPaSlots; }
// pack_init_kernel, then pack_kernel workgroup by workgroup and thread by thread as the kernel places them: the grid over (tile,
// polynomial, slot block, index chunk, ciphertext), the transposed sample words of the chunk, the staged window per key row,
// ring_sweep (rs_ring_sweep.h, the kernel's own) over the block's slots, the negated partial sums added into the output
void rs_emu_pack(const int32_t* ct, long count, int n, int N, const int32_t* pack_key, int basebit, int t, int32_t* rlwe) {
  if (count <= 0) return;
  const long R = (count + N - 1) / N;
  uint32_t* out = reinterpret_cast<uint32_t*>(rlwe);
  for (long idx = 0; idx < R * 2 * (long)N; ++idx) {
    const long r = idx / (2 * (long)N);
    const int w = (int)(idx - r * 2 * (long)N);
    const long s = r * (long)N + (w - N);
    out[idx] = (w >= N && s < count) ? (uint32_t)ct[(size_t)s * ((size_t)n + 1) + n] : 0u;
  }
  const int tiles = N / rs::kPaTile, sbs = rs::pa_slot_blocks(count, N), chunks = rs::pa_chunks(n);
  const uint32_t off = rs::pa_offset(basebit, t);
  const uint32_t* key = reinterpret_cast<const uint32_t*>(pack_key);
  std::vector<uint32_t> win((size_t)rs::kPaSlots + rs::kPaTile), sa((size_t)rs::kPaSeg * rs::kPaSlots);
  uint32_t acc[rs::kPaThreads][rs::kPaKpt];
  for (long blk = 0; blk < rs::pa_groups(count, n, N); ++blk) {
    long g = blk;
    const int tile = (int)(g % tiles); g /= tiles;
    const int poly = (int)(g & 1); g >>= 1;
    const int sb = (int)(g % sbs); g /= sbs;
    const int chunk = (int)(g % chunks);
    const long r = g / chunks;
    const int c0 = sb * rs::kPaSlots, slots = rs::pa_slots(count, N, r);
    if (c0 >= slots) continue;
    const int cn = slots - c0 < rs::kPaSlots ? slots - c0 : rs::kPaSlots, cpad = rs::pa_pad4(cn);
    const int i0 = chunk * rs::kPaSeg, segn = n - i0 < rs::kPaSeg ? n - i0 : rs::kPaSeg;
    const int k0 = tile * rs::kPaTile, wb = rs::pa_window_base(N, k0, c0, cpad);
    const uint32_t* cts = reinterpret_cast<const uint32_t*>(ct) + ((size_t)r * N + c0) * ((size_t)n + 1);
    std::memset(acc, 0, sizeof(acc));
    for (int idx = 0; idx < segn * cpad; ++idx) {
      const int cc = idx / segn, ii = idx - cc * segn;
      sa[(size_t)ii * cpad + cc] = cc < cn ? cts[(size_t)cc * ((size_t)n + 1) + i0 + ii] + off : 0u;
    }
    for (int ii = 0; ii < segn; ++ii)
      for (int j = 0; j < t; ++j) {
        const uint32_t* p = key + rs::pa_key_offset(N, t, i0 + ii, j, poly);
        for (int th = 0; th < rs::kPaThreads; ++th) rs::sweep_stage_window(win.data(), p, N, wb, cpad + rs::kPaTile, th, rs::kPaThreads);
        for (int th = 0; th < rs::kPaThreads; ++th)
          rs::ring_sweep(win.data(), &sa[(size_t)ii * cpad], cpad, th, [=](uint32_t abar) { return rs::pa_digit(abar, basebit, j); }, acc[th]);
      }
    uint32_t* o = out + ((size_t)r * 2 + poly) * N + k0;
    for (int x = 0; x < rs::kPaTile; ++x) o[x] += 0u - acc[x / rs::kPaKpt][x % rs::kPaKpt];
  }
}

// ---- re-keying (rs_rekey_dev) through the functions of rs_rekey.h ----
uint32_t rs_emu_rekey_offset(int basebit, int t) { return rs::rk_offset(basebit, t); }
uint32_t rs_emu_rekey_digit(uint32_t abar, int basebit, int j) { return rs::rk_digit(abar, basebit, j); }
int rs_emu_rekey_tile() { return rs::kRkTile; }
int rs_emu_rekey_wave_cts() { return rs::kRkWaveCts; }
int rs_emu_rekey_words() { return rs::kRkWords; }
int rs_emu_rekey_seg() { return rs::kRkSeg; }
int rs_emu_rekey_fill() { return rs::kRkFill; }
int rs_emu_rekey_chunks(int n_src) { return rs::rk_chunks(n_src); }
int rs_emu_rekey_span(long B, int n_src, int n_dst) { return rs::rk_span(B, n_src, n_dst); }
int rs_emu_rekey_splits(long B, int n_src, int n_dst) { return rs::rk_splits(B, n_src, n_dst); }
long rs_emu_rekey_groups(long B, int n_src, int n_dst) { return rs::rk_groups(B, n_src, n_dst); }
// rekey_init_kernel, then rekey_kernel workgroup by workgroup as the kernel places them: the grid over (word tile, index split,
// ciphertext tile), per chunk the transposed mask words of every wave, per source index the staged t x kRkWords key words, per wave
// and lane 32 accumulators fed by scalar digits in groups of kRkGroup, the negated partial sums added into the rows below B.
// span_override > 0 walks the same loops with that many chunks per workgroup instead of rk_span's (the CPU tests reach the
// splits of a large launch with a small one that way); 0 is the kernel's own plan.
void rs_emu_rekey(const int32_t* ct_, long B, int n_src, const int32_t* rekey_key, int n_dst, int basebit, int t, int span_override,
                  int32_t* out_) {
  if (B <= 0) return;
  const long W = (long)n_dst + 1;
  uint32_t* out = reinterpret_cast<uint32_t*>(out_);
  for (long idx = 0; idx < B * W; ++idx) {
    const long r = idx / W;
    const int w = (int)(idx - r * W);
    out[idx] = w == n_dst ? (uint32_t)ct_[(size_t)r * ((size_t)n_src + 1) + n_src] : 0u;
  }
  const int chunks = rs::rk_chunks(n_src), wtiles = rs::rk_word_tiles(n_dst);
  const int span = span_override > 0 ? span_override : rs::rk_span(B, n_src, n_dst);
  const int splits = (chunks + span - 1) / span;
  const long groups = rs::rk_ct_tiles(B) * wtiles * splits;
  const uint32_t off = rs::rk_offset(basebit, t), mask = (1u << basebit) - 1u;
  const uint32_t* key = reinterpret_cast<const uint32_t*>(rekey_key);
  std::vector<uint32_t> s_a((size_t)rs::kRkWaves * rs::kRkSeg * rs::kRkWaveCts), s_key((size_t)t * rs::kRkWords);
  std::vector<uint32_t> acc((size_t)rs::kRkThreads * rs::kRkWaveCts);
  for (long blk = 0; blk < groups; ++blk) {
    long g = blk;
    const int wt = (int)(g % wtiles); g /= wtiles;
    const int split = (int)(g % splits);
    const long ctile = g / splits;
    const int c_first = split * span, c_last = c_first + span < chunks ? c_first + span : chunks;
    std::fill(acc.begin(), acc.end(), 0u);
    int rows[rs::kRkWaves];
    const uint32_t* cts[rs::kRkWaves];
    for (int wave = 0; wave < rs::kRkWaves; ++wave) {
      const long r0 = ctile * rs::kRkTile + (long)wave * rs::kRkWaveCts, left = B - r0;
      rows[wave] = left >= rs::kRkWaveCts ? rs::kRkWaveCts : left > 0 ? (int)left : 0;
      cts[wave] = reinterpret_cast<const uint32_t*>(ct_) + (size_t)(rows[wave] > 0 ? r0 : 0) * ((size_t)n_src + 1);
    }
    for (int chunk = c_first; chunk < c_last; ++chunk) {
      const int i0 = chunk * rs::kRkSeg, segn = n_src - i0 < rs::kRkSeg ? n_src - i0 : rs::kRkSeg;
      for (int wave = 0; wave < rs::kRkWaves; ++wave) {
        uint32_t* sa = &s_a[(size_t)wave * rs::kRkSeg * rs::kRkWaveCts];
        for (int idx = 0; idx < segn * rs::kRkWaveCts; ++idx) {
          const int c = idx / segn, ii = idx - c * segn;
          sa[rs::rk_mask_index(ii, c)] = c < rows[wave] ? cts[wave][(size_t)c * ((size_t)n_src + 1) + i0 + ii] + off : 0u;
        }
      }
      for (int ii = 0; ii < segn; ++ii) {
        for (int j = 0; j < t; ++j)
          for (int lane = 0; lane < rs::kRkWords; ++lane) {
            const int w = wt * rs::kRkWords + lane;
            s_key[(size_t)j * rs::kRkWords + lane] = w <= n_dst ? key[rs::rk_key_offset(n_dst, t, i0 + ii, j) + w] : 0u;
          }
        for (int wave = 0; wave < rs::kRkWaves; ++wave) {
          if (rows[wave] == 0) continue;
          const uint32_t* abar = &s_a[(size_t)wave * rs::kRkSeg * rs::kRkWaveCts + rs::rk_mask_index(ii, 0)];
          for (int lane = 0; lane < rs::kRkWords; ++lane) {
            uint32_t* a32 = &acc[((size_t)wave * rs::kRkWords + lane) * rs::kRkWaveCts];
            for (int j = 0; j < t; ++j) {
              const uint32_t kw = s_key[(size_t)j * rs::kRkWords + lane];
              const int shift = 32 - (j + 1) * basebit;
              for (int q = 0; q < rs::kRkWaveCts / rs::kRkGroup; ++q) {
                if (q * rs::kRkGroup >= rows[wave]) continue;
                for (int c = q * rs::kRkGroup; c < (q + 1) * rs::kRkGroup; ++c) a32[c] += kw * ((abar[c] >> shift) & mask);
              }
            }
          }
        }
      }
    }
    for (int wave = 0; wave < rs::kRkWaves; ++wave)
      for (int lane = 0; lane < rs::kRkWords; ++lane) {
        const int w = wt * rs::kRkWords + lane;
        if (w > n_dst) continue;
        const long r0 = ctile * rs::kRkTile + (long)wave * rs::kRkWaveCts;
        for (int c = 0; c < rows[wave]; ++c)
          out[(size_t)(r0 + c) * W + w] += 0u - acc[((size_t)wave * rs::kRkWords + lane) * rs::kRkWaveCts + c];
      }
  }
}

// ---- ring re-keying (rs_ring_rekey_dev) through the functions of rs_ring_rekey.h ----
uint32_t rs_emu_ring_rekey_offset(int basebit, int t) { return rs::rr_offset(basebit, t); }
uint32_t rs_emu_ring_rekey_digit(uint32_t abar, int basebit, int j) { return rs::rr_digit(abar, basebit, j); }
int rs_emu_ring_rekey_tile() { return rs::kRrTile; }
int rs_emu_ring_rekey_slots() { return rs::kRrSlots; }
long rs_emu_ring_rekey_groups(long R, int N, int t) { return rs::rr_groups(R, N, t); }
int rs_emu_ring_rekey_window_base(int N, int k0, int c0) { return rs::ring_window_base(N, k0, c0); }
// ring_rekey_init_kernel, then ring_rekey_kernel workgroup by workgroup and thread by thread as the kernel places them: ring_place
// over (tile, polynomial, source block, digit, ciphertext), the staged window of the key row and the block's words a_k + offset,
// ring_sweep (rs_ring_sweep.h, the kernel's own) with the odd digit, the negated partial sums added into the output
void rs_emu_ring_rekey(const int32_t* rlwe, long R, int N, const int32_t* ring_key, int basebit, int t, int32_t* out_) {
  if (R <= 0) return;
  uint32_t* out = reinterpret_cast<uint32_t*>(out_);
  const uint32_t* in = reinterpret_cast<const uint32_t*>(rlwe);
  const uint32_t* key = reinterpret_cast<const uint32_t*>(ring_key);
  for (long idx = 0; idx < R * 2 * (long)N; ++idx) {
    const int w = (int)(idx & (2 * (long)N - 1));
    out[idx] = (w >= N ? in[idx] : 0u) - key[rs::rr_key_offset(N, t, 0) + (size_t)w];
  }
  const uint32_t off = rs::rr_offset(basebit, t);
  std::vector<uint32_t> win((size_t)rs::kRingWindow), sa((size_t)rs::kRingSlots);
  for (long blk = 0; blk < rs::rr_groups(R, N, t); ++blk) {
    const rs::RingPlace pl = rs::ring_place((unsigned)blk, N, t);
    const int j = pl.row, c0 = pl.sb * rs::kRingSlots, k0 = pl.tile * rs::kRingTile;
    const uint32_t* src = in + (size_t)pl.r * 2 * N + c0;
    const uint32_t* p = key + rs::rr_key_offset(N, j, pl.poly);
    for (int th = 0; th < rs::kRingThreads; ++th)
      rs::sweep_stage_window(win.data(), p, N, rs::ring_window_base(N, k0, c0), rs::kRingWindow, th, rs::kRingThreads);
    for (int cc = 0; cc < rs::kRingSlots; ++cc) sa[cc] = src[cc] + off;
    for (int th = 0; th < rs::kRingThreads; ++th) {
      uint32_t acc[rs::kSweepKpt] = {0u, 0u, 0u, 0u};
      rs::ring_sweep(win.data(), sa.data(), rs::kRingSlots, th, [=](uint32_t abar) { return rs::rr_digit(abar, basebit, j); }, acc);
      uint32_t* o = out + ((size_t)pl.r * 2 + pl.poly) * N + k0 + rs::kSweepKpt * th;
      for (int q = 0; q < rs::kSweepKpt; ++q) o[q] += 0u - acc[q];
    }
  }
}

// ---- encrypted selection (rs_ring_cmux_dev, rs_ring_lookup_dev) through the functions of rs_ring_cmux.h ----
uint32_t rs_emu_ring_cmux_offset(int basebit, int l) { return rs::rc_offset(basebit, l); }
uint32_t rs_emu_ring_cmux_digit(uint32_t xbar, int basebit, int j) { return rs::rc_digit(xbar, basebit, j); }
long rs_emu_ring_cmux_groups(long R, int N, int l) { return rs::rc_groups(R, N, l); }
long rs_emu_ring_lookup_scratch_rows(long entries) { return rs::rc_scratch_rows(entries); }
// ring_cmux_init_kernel, then ring_cmux_kernel workgroup by workgroup and thread by thread as the kernel places them: ring_place
// over (tile, polynomial, source block, selector row, ciphertext), the staged window of the selector row and the block's words
// d1 - d0 + offset (-d0 + offset under a null d1), ring_sweep (rs_ring_sweep.h, the kernel's own) with the signed digit, the
// partial sums added into the output. form = rs::kRcAlternating: ring_cmux_alt_kernel (rs_ring_cmux_alt.hip), which stages
// eps_k x_k + offset (the parity of k = c0 + cc is that of the slot cc) and sweeps with ring_sweep_parity and rc_digit_alt
static void emu_ring_cmux(const int32_t* d1_, const int32_t* d0_, long R, long stride, int N, const int32_t* sel_, int basebit, int l,
                          int form, int32_t* out_) {
  if (R <= 0) return;
  uint32_t* out = reinterpret_cast<uint32_t*>(out_);
  const uint32_t* d1 = reinterpret_cast<const uint32_t*>(d1_);
  const uint32_t* d0 = reinterpret_cast<const uint32_t*>(d0_);
  const uint32_t* sel = reinterpret_cast<const uint32_t*>(sel_);
  const long per = 2 * (long)N;
  for (long idx = 0; idx < R * per; ++idx) out[idx] = d0[(size_t)(idx / per) * (size_t)stride * (size_t)per + (size_t)(idx % per)];
  const uint32_t off = rs::rc_offset(basebit, l);
  std::vector<uint32_t> win((size_t)rs::kRingWindow), sx((size_t)rs::kRingSlots);
  for (long blk = 0; blk < rs::rc_groups(R, N, l); ++blk) {
    const rs::RingPlace pl = rs::ring_place((unsigned)blk, N, 2 * l);
    const int jr = pl.row, j = jr < l ? jr : jr - l, spoly = jr < l ? 0 : 1;
    const int c0 = pl.sb * rs::kRingSlots, k0 = pl.tile * rs::kRingTile;
    const size_t src_at = ((size_t)pl.r * (size_t)stride * 2 + (size_t)spoly) * (size_t)N + (size_t)c0;
    const uint32_t* p = sel + rs::rc_sel_offset(N, jr, pl.poly);
    for (int th = 0; th < rs::kRingThreads; ++th)
      rs::sweep_stage_window(win.data(), p, N, rs::ring_window_base(N, k0, c0), rs::kRingWindow, th, rs::kRingThreads);
    for (int th = 0; th < rs::kRingThreads; ++th)                      // thread th stages the slots th, th + kRingThreads, ..
      for (int cc = th; cc < rs::kRingSlots; cc += rs::kRingThreads) {
        const uint32_t x = (d1 ? d1[src_at + cc] : 0u) - d0[src_at + cc];
        sx[cc] = form == rs::kRcAlternating ? rs::rc_stage_alt(x, off, th & 1) : x + off;
      }
    for (int th = 0; th < rs::kRingThreads; ++th) {
      uint32_t acc[rs::kSweepKpt] = {0u, 0u, 0u, 0u};
      if (form == rs::kRcAlternating)
        rs::ring_sweep_parity(win.data(), sx.data(), rs::kRingSlots, th,
                              [=](uint32_t xbar, auto slot_odd) { return rs::rc_digit_alt(xbar, basebit, j, decltype(slot_odd)::value); }, acc);
      else
        rs::ring_sweep(win.data(), sx.data(), rs::kRingSlots, th, [=](uint32_t xbar) { return rs::rc_digit(xbar, basebit, j); }, acc);
      uint32_t* o = out + ((size_t)pl.r * 2 + pl.poly) * N + k0 + rs::kSweepKpt * th;
      for (int q = 0; q < rs::kSweepKpt; ++q) o[q] += acc[q];
    }
  }
}
void rs_emu_ring_cmux(const int32_t* d1, const int32_t* d0, long R, long stride, int N, const int32_t* sel, int basebit, int l,
                      int32_t* out) {
  emu_ring_cmux(d1, d0, R, stride, N, sel, basebit, l, rs::kRcSigned, out);
}
void rs_emu_ring_cmux_alt(const int32_t* d1, const int32_t* d0, long R, long stride, int N, const int32_t* sel, int basebit, int l,
                          int32_t* out) {
  emu_ring_cmux(d1, d0, R, stride, N, sel, basebit, l, rs::kRcAlternating, out);
}
// eps_k dig_j of the staged word xbar = eps_k x_k + offset, odd = k & 1
uint32_t rs_emu_ring_cmux_digit_alt(uint32_t xbar, int basebit, int j, int odd) { return rs::rc_digit_alt(xbar, basebit, j, odd); }
// rs_ring_lookup_dev's levels as the host code orders them: pairs at stride 2, an unpaired last row against the null d1, the two
// halves of scratch in turn, the last level into out
static void emu_ring_lookup(const int32_t* table, long entries, int N, const int32_t* sel, int depth, int basebit, int l, int form,
                            int32_t* scratch, int32_t* out) {
  const size_t ct = 2 * (size_t)N, sel_words = (size_t)2 * l * ct;
  int32_t* half[2] = {scratch, scratch ? scratch + (size_t)rs::rc_level_rows(entries) * ct : nullptr};
  const int32_t* in = table;
  long rows = entries;
  for (int k = 0; k < depth; ++k) {
    int32_t* o = k == depth - 1 ? out : half[k & 1];
    const long pairs = rows / 2;
    const int32_t* s = sel + (size_t)k * sel_words;
    if (pairs) emu_ring_cmux(in + ct, in, pairs, 2, N, s, basebit, l, form, o);
    if (rows & 1) emu_ring_cmux(nullptr, in + (size_t)(rows - 1) * ct, 1, 1, N, s, basebit, l, form, o + (size_t)pairs * ct);
    in = o;
    rows = rs::rc_level_rows(rows);
  }
}
void rs_emu_ring_lookup(const int32_t* table, long entries, int N, const int32_t* sel, int depth, int basebit, int l,
                        int32_t* scratch, int32_t* out) {
  emu_ring_lookup(table, entries, N, sel, depth, basebit, l, rs::kRcSigned, scratch, out);
}
void rs_emu_ring_lookup_alt(const int32_t* table, long entries, int N, const int32_t* sel, int depth, int basebit, int l,
                            int32_t* scratch, int32_t* out) {
  emu_ring_lookup(table, entries, N, sel, depth, basebit, l, rs::kRcAlternating, scratch, out);
}
// ---- batched encrypted lookup (rs_ring_lookup_rows_dev) through the functions of rs_ring_lookup.h ----
long rs_emu_ring_lookup_level_rows(long rows) { return rs::lk_level_rows(rows); }
long rs_emu_ring_lookup_rows_groups(long R, long rows, int N, int l) { return rs::lk_groups(R, rs::lk_level_rows(rows), N, l); }
long rs_emu_ring_lookup_rows_scratch_rows(long R, long entries) { return rs::lk_scratch_rows(R, entries); }
// (q, i) of output ciphertext g of a level that leaves P ciphertexts per row
void rs_emu_ring_lookup_rows_place(long g, long P, long* q, long* i) {
  const rs::LkPlace at = rs::lk_place(g, P);
  *q = at.q;
  *i = at.i;
}
// one level as launch_ring_lookup_level runs it: ring_lookup_init_kernel, then ring_lookup_level_kernel or
// ring_lookup_level_alt_kernel workgroup by workgroup and thread by thread: ring_place, (q, i) from the output ciphertext, the
// staged window of sample k of row q's set, the block's words d1 - d0 + offset, or -d0 + offset where the pair has no second row
// (rc_stage_alt in the alternating form, the parity that of the thread), ring_sweep / ring_sweep_parity, the partial sums added
// into the output
static void emu_ring_lookup_level(const int32_t* in_, long R, long rows, size_t row_stride, size_t entry_stride, int N,
                                  const int32_t* sel_, size_t sel_row_stride, int k, int basebit, int l, int form, int32_t* out_) {
  if (R <= 0) return;
  uint32_t* out = reinterpret_cast<uint32_t*>(out_);
  const uint32_t* in = reinterpret_cast<const uint32_t*>(in_);
  const uint32_t* sel = reinterpret_cast<const uint32_t*>(sel_);
  const long P = rs::lk_level_rows(rows);
  const size_t ct = 2 * (size_t)N;
  for (long g = 0; g < R * P; ++g) {
    const rs::LkPlace at = rs::lk_place(g, P);
    for (size_t w = 0; w < ct; ++w) out[(size_t)g * ct + w] = in[rs::lk_source(at.q, at.i, row_stride, entry_stride) * ct + w];
  }
  const uint32_t off = rs::rc_offset(basebit, l);
  std::vector<uint32_t> win((size_t)rs::kRingWindow), sx((size_t)rs::kRingSlots);
  for (long blk = 0; blk < rs::lk_groups(R, P, N, l); ++blk) {
    const rs::RingPlace pl = rs::ring_place((unsigned)blk, N, 2 * l);
    const rs::LkPlace at = rs::lk_place(pl.r, P);
    const int jr = pl.row, j = jr < l ? jr : jr - l, spoly = jr < l ? 0 : 1;
    const int c0 = pl.sb * rs::kRingSlots, k0 = pl.tile * rs::kRingTile;
    const size_t src_at = (rs::lk_source(at.q, at.i, row_stride, entry_stride) * 2 + (size_t)spoly) * (size_t)N + (size_t)c0;
    const uint32_t* s0 = in + src_at;
    const uint32_t* s1 = rs::lk_paired(at.i, rows) ? s0 + entry_stride * 2 * (size_t)N : nullptr;
    const uint32_t* p = sel + rs::lk_sel_offset(at.q, sel_row_stride, k, N, l) + rs::rc_sel_offset(N, jr, pl.poly);
    for (int th = 0; th < rs::kRingThreads; ++th)
      rs::sweep_stage_window(win.data(), p, N, rs::ring_window_base(N, k0, c0), rs::kRingWindow, th, rs::kRingThreads);
    for (int th = 0; th < rs::kRingThreads; ++th)
      for (int cc = th; cc < rs::kRingSlots; cc += rs::kRingThreads) {
        const uint32_t x = (s1 ? s1[cc] : 0u) - s0[cc];
        sx[cc] = form == rs::kRcAlternating ? rs::rc_stage_alt(x, off, th & 1) : x + off;
      }
    for (int th = 0; th < rs::kRingThreads; ++th) {
      uint32_t acc[rs::kSweepKpt] = {0u, 0u, 0u, 0u};
      if (form == rs::kRcAlternating)
        rs::ring_sweep_parity(win.data(), sx.data(), rs::kRingSlots, th,
                              [=](uint32_t xbar, auto slot_odd) { return rs::rc_digit_alt(xbar, basebit, j, decltype(slot_odd)::value); }, acc);
      else
        rs::ring_sweep(win.data(), sx.data(), rs::kRingSlots, th, [=](uint32_t xbar) { return rs::rc_digit(xbar, basebit, j); }, acc);
      uint32_t* o = out + ((size_t)pl.r * 2 + pl.poly) * N + k0 + rs::kSweepKpt * th;
      for (int q = 0; q < rs::kSweepKpt; ++q) o[q] += acc[q];
    }
  }
}
// rs_ring_lookup_rows_dev's levels as the host code orders them: level 0 from the tables at the caller's strides, the later ones
// from the previous target [R][P] at row stride P and entry stride 1, the two halves of scratch in turn, the last level into out
static void emu_ring_lookup_rows(const int32_t* table, long entries, size_t row_stride, size_t entry_stride, long R, int N,
                                 const int32_t* sel, int depth, int per_row, int basebit, int l, int form, int32_t* scratch, int32_t* out) {
  const size_t ct = 2 * (size_t)N, set_words = (size_t)depth * rs::lk_sel_words(N, l);
  int32_t* half[2] = {scratch, scratch ? scratch + (size_t)rs::lk_scratch_half(R, entries, 1) * ct : nullptr};
  const int32_t* in = table;
  long rows = entries;
  for (int k = 0; k < depth; ++k) {
    int32_t* o = k == depth - 1 ? out : half[k & 1];
    emu_ring_lookup_level(in, R, rows, row_stride, entry_stride, N, sel, per_row ? set_words : 0, k, basebit, l, form, o);
    in = o;
    rows = rs::lk_level_rows(rows);
    row_stride = (size_t)rows;
    entry_stride = 1;
  }
}
void rs_emu_ring_lookup_rows(const int32_t* table, long entries, long row_stride, long entry_stride, long R, int N, const int32_t* sel,
                             int depth, int per_row, int basebit, int l, int32_t* scratch, int32_t* out) {
  emu_ring_lookup_rows(table, entries, (size_t)row_stride, (size_t)entry_stride, R, N, sel, depth, per_row, basebit, l, rs::kRcSigned,
                       scratch, out);
}
void rs_emu_ring_lookup_rows_alt(const int32_t* table, long entries, long row_stride, long entry_stride, long R, int N,
                                 const int32_t* sel, int depth, int per_row, int basebit, int l, int32_t* scratch, int32_t* out) {
  emu_ring_lookup_rows(table, entries, (size_t)row_stride, (size_t)entry_stride, R, N, sel, depth, per_row, basebit, l,
                       rs::kRcAlternating, scratch, out);
}
// ---- encrypted rotation (rs_ring_rotate_dev, rs_ring_heads_dev) through the functions of rs_ring_rotate.h ----
int rs_emu_ring_rotate_exponent(int32_t step, int k, int N) { return rs::ro_exponent(step, k, N); }
// source index of coefficient c of X^e v; *negate: the word is the negated coefficient
int rs_emu_ring_rotate_source(int N, int e, int c, int* negate) {
  bool neg;
  const int idx = rs::ro_source(N, e, c, neg);
  *negate = neg ? 1 : 0;
  return idx;
}
// one level as launch_ring_rotate_level runs it: ring_rotate_init_kernel, then (e != 0) ring_rotate_kernel or ring_rotate_alt_kernel
// workgroup by workgroup and thread by thread: ring_place, the staged window of the row's selector sample, the block's words
// (X^e in)_c - in_c + offset read through ro_rotated_word (rc_stage_alt of the difference in the alternating form, the parity that
// of the thread), ring_sweep / ring_sweep_parity, the partial sums added into the output
static void emu_ring_rotate_level(const int32_t* in_, long R, long stride, int N, const int32_t* sel_, size_t sel_stride, int e,
                                  int basebit, int l, int form, int32_t* out_) {
  if (R <= 0) return;
  uint32_t* out = reinterpret_cast<uint32_t*>(out_);
  const uint32_t* in = reinterpret_cast<const uint32_t*>(in_);
  const uint32_t* sel = reinterpret_cast<const uint32_t*>(sel_);
  const long per = 2 * (long)N;
  for (long idx = 0; idx < R * per; ++idx) out[idx] = in[(size_t)(idx / per) * (size_t)stride * (size_t)per + (size_t)(idx % per)];
  if (e == 0) return;
  const uint32_t off = rs::rc_offset(basebit, l);
  std::vector<uint32_t> win((size_t)rs::kRingWindow), sx((size_t)rs::kRingSlots);
  for (long blk = 0; blk < rs::rc_groups(R, N, l); ++blk) {
    const rs::RingPlace pl = rs::ring_place((unsigned)blk, N, 2 * l);
    const int jr = pl.row, j = jr < l ? jr : jr - l, spoly = jr < l ? 0 : 1;
    const int c0 = pl.sb * rs::kRingSlots, k0 = pl.tile * rs::kRingTile;
    const uint32_t* v = in + ((size_t)pl.r * (size_t)stride * 2 + (size_t)spoly) * (size_t)N;
    const uint32_t* p = sel + (size_t)pl.r * sel_stride + rs::rc_sel_offset(N, jr, pl.poly);
    for (int th = 0; th < rs::kRingThreads; ++th)
      rs::sweep_stage_window(win.data(), p, N, rs::ring_window_base(N, k0, c0), rs::kRingWindow, th, rs::kRingThreads);
    for (int th = 0; th < rs::kRingThreads; ++th)
      for (int cc = th; cc < rs::kRingSlots; cc += rs::kRingThreads) {
        const uint32_t x = rs::ro_rotated_word(v, N, e, c0 + cc) - v[c0 + cc];
        sx[cc] = form == rs::kRcAlternating ? rs::rc_stage_alt(x, off, th & 1) : x + off;
      }
    for (int th = 0; th < rs::kRingThreads; ++th) {
      uint32_t acc[rs::kSweepKpt] = {0u, 0u, 0u, 0u};
      if (form == rs::kRcAlternating)
        rs::ring_sweep_parity(win.data(), sx.data(), rs::kRingSlots, th,
                              [=](uint32_t xbar, auto slot_odd) { return rs::rc_digit_alt(xbar, basebit, j, decltype(slot_odd)::value); }, acc);
      else
        rs::ring_sweep(win.data(), sx.data(), rs::kRingSlots, th, [=](uint32_t xbar) { return rs::rc_digit(xbar, basebit, j); }, acc);
      uint32_t* o = out + ((size_t)pl.r * 2 + pl.poly) * N + k0 + rs::kSweepKpt * th;
      for (int q = 0; q < rs::kSweepKpt; ++q) o[q] += acc[q];
    }
  }
}
// rs_ring_rotate_dev's levels as the host code orders them: level 0 from `in` at `stride`, the later ones from the previous target,
// scratch and out in turn so that the last level writes out
static void emu_ring_rotate(const int32_t* in, long R, long stride, int N, const int32_t* sel, int depth, int per_row, int32_t step,
                            int basebit, int l, int form, int32_t* scratch, int32_t* out) {
  const size_t sel_words = rs::ro_sel_words(N, l), set_words = (size_t)depth * sel_words;
  const int32_t* src = in;
  for (int k = 0; k < depth; ++k) {
    int32_t* o = ((depth - 1 - k) & 1) ? scratch : out;
    emu_ring_rotate_level(src, R, k ? 1 : stride, N, sel + (size_t)k * sel_words, per_row ? set_words : 0, rs::ro_exponent(step, k, N),
                          basebit, l, form, o);
    src = o;
  }
}
void rs_emu_ring_rotate(const int32_t* in, long R, long stride, int N, const int32_t* sel, int depth, int per_row, int32_t step,
                        int basebit, int l, int32_t* scratch, int32_t* out) {
  emu_ring_rotate(in, R, stride, N, sel, depth, per_row, step, basebit, l, rs::kRcSigned, scratch, out);
}
void rs_emu_ring_rotate_alt(const int32_t* in, long R, long stride, int N, const int32_t* sel, int depth, int per_row, int32_t step,
                            int basebit, int l, int32_t* scratch, int32_t* out) {
  emu_ring_rotate(in, R, stride, N, sel, depth, per_row, step, basebit, l, rs::kRcAlternating, scratch, out);
}
// ring_heads_kernel: rlwe [R][2][N] -> u [R width][N+1], one workgroup per output row
void rs_emu_ring_heads(const int32_t* rlwe, long R, long width, int N, int32_t* u) {
  for (long i = 0; i < R * width; ++i) {
    const long r = i / width;
    const int c = (int)(i - r * width);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(rlwe) + (size_t)r * 2 * N;
    for (int j = 0; j <= N; ++j) u[(size_t)i * (N + 1) + j] = (int32_t)rs::rl_extract_word(a, a + N, N, c, j);
  }
}
// ---- the refusal of an out that overlaps an input (rs_api_client.cpp refuse_overlap) through rs_host.h first_overlap ----
// written = (address, bytes); others [count][2] the same pairs -> the index of the first one that shares a byte with it, or -1.
// Addresses are plain numbers here: nothing is read or written through them.
int rs_emu_first_overlap(uint64_t address, uint64_t bytes, const uint64_t* others, int count) {
  std::vector<rs::Extent> x;
  for (int i = 0; i < count; ++i) x.push_back({"", (const void*)(uintptr_t)others[2 * i], (size_t)others[2 * i + 1]});
  return rs::first_overlap({"", (const void*)(uintptr_t)address, (size_t)bytes}, x.data(), count);
}
// ---- the selector keyswitch of circuit bootstrapping (rs_ring_selector_dev) through the functions of rs_ring_selector.h ----
uint32_t rs_emu_ring_selector_offset(int ks_basebit, int ks_t) { return rs::se_offset(ks_basebit, ks_t); }
long rs_emu_ring_selector_groups(long rows, int N, int n_src) { return rs::se_groups(rows, N, n_src); }
int rs_emu_ring_selector_chunk() { return rs::kSeChunk; }
int rs_emu_ring_selector_rows() { return rs::kSeRows; }
long rs_emu_circuit_scratch_words(int N, int l, long rows, int n) { return (long)rs::se_scratch_words(N, l, rows, n); }
// ring_selector_init_kernel, then ring_selector_kernel workgroup by workgroup and thread by thread as the kernel places them: the
// grid over (tile, polynomial, family, chunk, row block), the staged words x_i + off of the chunk's coordinates and the block's rows
// (zero where none), the chunk's key polynomials in storage order, four coefficients a thread, the negated partial sums added into
// the output
void rs_emu_ring_selector(const int32_t* ct_, int depth, int basebit, int l, int n_src, int N, const int32_t* key_, int ks_basebit,
                          int ks_t, int32_t* sel_) {
  const long rows = (long)depth * l;
  if (rows <= 0) return;
  uint32_t* sel = reinterpret_cast<uint32_t*>(sel_);
  const uint32_t* ct = reinterpret_cast<const uint32_t*>(ct_);
  const uint32_t* key = reinterpret_cast<const uint32_t*>(key_);
  for (long idx = 0; idx < rows * 4 * (long)N; ++idx) sel[idx] = 0u;
  const unsigned tiles = (unsigned)rs::se_tiles(N), chunks = (unsigned)rs::se_chunks(n_src);
  const uint32_t off = rs::se_offset(ks_basebit, ks_t), mask = (1u << ks_basebit) - 1u;
  uint32_t sx[rs::kSeChunk * rs::kSeRows];
  for (long blk = 0; blk < rs::se_groups(rows, N, n_src); ++blk) {
    unsigned g = (unsigned)blk;
    const int tile = (int)(g % tiles); g /= tiles;
    const int p = (int)(g & 1u); g >>= 1;
    const int f = (int)(g & 1u); g >>= 1;
    const int chunk = (int)(g % chunks);
    const int r0 = (int)(g / chunks) * rs::kSeRows;
    const int i0 = chunk * rs::kSeChunk, cn = n_src + 1 - i0 < rs::kSeChunk ? n_src + 1 - i0 : rs::kSeChunk;
    const int rn = (int)rows - r0 < rs::kSeRows ? (int)rows - r0 : rs::kSeRows;
    for (int t = 0; t < rs::kSeChunk * rs::kSeRows; ++t) {
      const int ii = t / rs::kSeRows, r = t - ii * rs::kSeRows;
      uint32_t x = 0u;
      if (ii < cn && r < rn) {
        const int i = i0 + ii;
        x = ct[(size_t)(r0 + r) * ((size_t)n_src + 1) + (size_t)i] + off;
        if (i == n_src) x += rs::se_half_step(basebit, (r0 + r) % l);
      }
      sx[t] = x;
    }
    for (int t = 0; t < rs::kSeThreads; ++t) {
      const int k0 = tile * rs::kSeTile + rs::kSeKpt * t;
      uint32_t acc[rs::kSeRows][rs::kSeKpt] = {};
      for (int ii = 0; ii < cn; ++ii)
        for (int q = 0; q < ks_t; ++q) {
          const uint32_t* kw = key + rs::se_key_offset(N, n_src, ks_t, f, i0 + ii, q, p) + k0;
          const int shift = 32 - (q + 1) * ks_basebit;
          for (int r = 0; r < rs::kSeRows; ++r) {
            const uint32_t d = (sx[ii * rs::kSeRows + r] >> shift) & mask;
            for (int c = 0; c < rs::kSeKpt; ++c) acc[r][c] += kw[c] * d;
          }
        }
      for (int r = 0; r < rn; ++r) {
        uint32_t* o = sel + rs::se_out_offset(N, l, r0 + r, f, p) + k0;
        for (int c = 0; c < rs::kSeKpt; ++c) o[c] += 0u - acc[r][c];
      }
    }
  }
}
// ---- the wide form of the selector keyswitch (rs_ring_selector_batch_dev) through the functions of rs_ring_selector.h ----
int rs_emu_ring_selector_wide_rows() { return rs::kSwRows; }
int rs_emu_ring_selector_wide_piece() { return rs::kSwPiece; }
int rs_emu_ring_selector_wide_lds_bytes() { return rs::kSwLdsBytes; }
long rs_emu_ring_selector_wide_groups(long rows, int N) { return rs::sw_groups(rows, N); }
// selector_form: form + 2 * workgroups; force = -1 (by row count), 0 (chunked), 1 (wide)
long rs_emu_selector_form(long rows, int N, int n_src, int num_cus, int force) {
  const rs::SePlan p = rs::selector_form(rows, N, n_src, num_cus, force);
  return (long)p.form + 2 * p.groups;
}
// ring_selector_wide_kernel workgroup by workgroup and thread by thread as the kernel places them: the grid over (tile, polynomial,
// family, row block), the pieces of kSwPiece coordinates staged as x_i + off (zero where no row or coordinate is), the key
// polynomials of all coordinates in storage order, four coefficients a thread, the negated sums stored once. sel is not read: words
// the kernel does not write keep what the caller put there.
void rs_emu_ring_selector_wide(const int32_t* ct_, long count, int basebit, int l, int n_src, int N, const int32_t* key_, int ks_basebit,
                               int ks_t, int32_t* sel_) {
  const long rows = count * l;
  if (rows <= 0) return;
  uint32_t* sel = reinterpret_cast<uint32_t*>(sel_);
  const uint32_t* ct = reinterpret_cast<const uint32_t*>(ct_);
  const uint32_t* key = reinterpret_cast<const uint32_t*>(key_);
  const unsigned tiles = (unsigned)rs::se_tiles(N);
  const uint32_t off = rs::se_offset(ks_basebit, ks_t), mask = (1u << ks_basebit) - 1u;
  std::vector<uint32_t> sx((size_t)rs::kSwPiece * rs::kSwRows);
  std::vector<uint32_t> acc((size_t)rs::kSeThreads * rs::kSwRows * rs::kSeKpt);
  for (long blk = 0; blk < rs::sw_groups(rows, N); ++blk) {
    unsigned g = (unsigned)blk;
    const int tile = (int)(g % tiles); g /= tiles;
    const int p = (int)(g & 1u); g >>= 1;
    const int f = (int)(g & 1u); g >>= 1;
    const long r0 = (long)g * rs::kSwRows;
    const int rn = rows - r0 < (long)rs::kSwRows ? (int)(rows - r0) : rs::kSwRows;
    std::fill(acc.begin(), acc.end(), 0u);
    for (int i0 = 0; i0 <= n_src; i0 += rs::kSwPiece) {
      const int cn = n_src + 1 - i0 < rs::kSwPiece ? n_src + 1 - i0 : rs::kSwPiece;
      for (int s = 0; s < rs::kSwPiece * rs::kSwRows; ++s) {
        const int r = s / rs::kSwPiece, ii = s - r * rs::kSwPiece;
        uint32_t x = 0u;
        if (ii < cn && r < rn) {
          const int i = i0 + ii;
          x = ct[(size_t)(r0 + r) * ((size_t)n_src + 1) + (size_t)i] + off;
          if (i == n_src) x += rs::se_half_step(basebit, (int)((r0 + r) % l));
        }
        sx[(size_t)ii * rs::kSwRows + r] = x;
      }
      for (int t = 0; t < rs::kSeThreads; ++t) {
        const int k0 = tile * rs::kSeTile + rs::kSeKpt * t;
        uint32_t* a = acc.data() + (size_t)t * rs::kSwRows * rs::kSeKpt;
        for (int ii = 0; ii < cn; ++ii)
          for (int q = 0; q < ks_t; ++q) {
            const uint32_t* kw = key + rs::se_key_offset(N, n_src, ks_t, f, i0 + ii, q, p) + k0;
            const int shift = 32 - (q + 1) * ks_basebit;
            for (int r = 0; r < rs::kSwRows; ++r) {
              const uint32_t d = (sx[(size_t)ii * rs::kSwRows + r] >> shift) & mask;
              for (int c = 0; c < rs::kSeKpt; ++c) a[r * rs::kSeKpt + c] += kw[c] * d;
            }
          }
      }
    }
    for (int t = 0; t < rs::kSeThreads; ++t) {
      const int k0 = tile * rs::kSeTile + rs::kSeKpt * t;
      const uint32_t* a = acc.data() + (size_t)t * rs::kSwRows * rs::kSeKpt;
      for (int r = 0; r < rn; ++r) {
        uint32_t* o = sel + rs::se_out_offset(N, l, (int)(r0 + r), f, p) + k0;
        for (int c = 0; c < rs::kSeKpt; ++c) o[c] = 0u - a[r * rs::kSeKpt + c];
      }
    }
  }
}
// ---- device decryption and the key audit (rs_phase_dev, rs_audit_keys_dev, rs_audit_compressed_keys_dev) through the functions of
// rs_audit.h, as the kernels of rs_audit.hip place them: a wave of 64 lanes per LWE sample, a workgroup of kAuThreads per bk row ----
static std::vector<uint32_t> emu_pack_bits(const int32_t* key, int count) {
  std::vector<uint32_t> bits((size_t)(count + 31) / 32, 0u);
  for (int i = 0; i < count; ++i) bits[(size_t)i >> 5] |= (uint32_t)(key[i] & 1) << (i & 31);
  return bits;
}
// lwe_phase_kernel: ct[B][dim+1], key int32[dim] 0/1 -> phase[B]
void rs_emu_phase(const int32_t* ct, long B, int dim, const int32_t* key, int32_t* phase) {
  const std::vector<uint32_t> bits = emu_pack_bits(key, dim);
  for (long i = 0; i < B; ++i) {
    const uint32_t* row = reinterpret_cast<const uint32_t*>(ct) + i * (dim + 1);
    uint32_t dot = 0u;
    for (int lane = 0; lane < 64; ++lane) dot += rs::au_lane_dot(row, dim, bits.data(), lane);
    phase[i] = (int32_t)(row[dim] - dot);
  }
}
// audit_bk_kernel: the noise words of bk row `row`. seeded = 0: stored = the full key's row int32[2][N]; seeded = 1: stored = the
// body row int32[N], the mask regenerated from mask_seed. -> noise[N]
void rs_emu_audit_bk_row(int seeded, const uint8_t* mask_seed, int N, int l, int bgbit, uint64_t row, const int32_t* stored,
                         const int32_t* lwe_key, int n, const int32_t* tlwe_key, int32_t* noise) {
  const std::vector<uint32_t> lwe = emu_pack_bits(lwe_key, n), S = emu_pack_bits(tlwe_key, N);
  std::vector<uint16_t> list((size_t)N);
  int cnt = 0;
  for (int w = 0; w < N / 32; ++w) cnt = rs::au_list_word(S[w], w, cnt, list.data());
  std::vector<uint32_t> a((size_t)N);
  const uint32_t* b_row;
  if (seeded) {
    uint32_t key[8];
    rs::kg_seed_words(mask_seed, key);
    for (int t = 0; t < rs::kAuThreads; ++t)
      for (int blk = t; blk < N / 16; blk += rs::kAuThreads) {
        uint32_t w[16];
        rs::kg_bk_mask_block(key, row, blk, w);
        for (int q = 0; q < 16; ++q) a[16 * blk + q] = w[q];
      }
    b_row = reinterpret_cast<const uint32_t*>(stored);
  } else {
    for (int k = 0; k < N; ++k) a[k] = (uint32_t)stored[k];
    b_row = reinterpret_cast<const uint32_t*>(stored) + N;
  }
  int i, c, j;
  rs::au_bk_row(row, l, i, c, j);
  const uint32_t s = rs::au_key_bit(lwe.data(), i), g = rs::au_gadget(j, bgbit);
  for (int t = 0; t < rs::kAuThreads; ++t)
    for (int k0 = t; k0 < N; k0 += rs::kAuThreads * rs::kAuKpt) {
      uint32_t acc[rs::kAuKpt];
      rs::au_bk_products(a.data(), N, list.data(), cnt, k0, acc);
      for (int q = 0; q < rs::kAuKpt; ++q) {
        const int k = k0 + rs::kAuThreads * q;
        noise[k] = (int32_t)rs::au_bk_noise(b_row[k], acc[q], rs::au_bk_message(c, s, g, k, rs::au_key_bit(S.data(), k)));
      }
    }
}
// audit_ksk_kernel: the noise word of ksk sample s. seeded = 0: stored = the sample int32[n+1]; seeded = 1: stored = its body word.
// *zero_bad = 1 for a v = 0 sample of a full key with a non-zero word
int32_t rs_emu_audit_ksk_word(int seeded, const uint8_t* mask_seed, int n, int t, int basebit, uint64_t s, const int32_t* stored,
                              const int32_t* lwe_key, int32_t S_i_of_sample, int* zero_bad) {
  const std::vector<uint32_t> lwe = emu_pack_bits(lwe_key, n);
  const uint32_t* row = reinterpret_cast<const uint32_t*>(stored);
  int i, j, v;
  rs::au_ksk_sample(s, t, basebit, i, j, v);
  *zero_bad = 0;
  if (v == 0) {
    uint32_t any = 0u;
    for (int lane = 0; !seeded && lane < 64; ++lane) any |= rs::au_lane_or(row, n, lane);
    *zero_bad = any != 0u;
    return 0;
  }
  uint32_t dot = 0u, b;
  if (seeded) {
    uint32_t key[8];
    rs::kg_seed_words(mask_seed, key);
    for (int lane = 0; lane < 64; ++lane)
      for (int k0 = 0; k0 < n; k0 += rs::kKgChunk) dot += rs::au_ksk_seeded_lane_dot(key, s, k0, lane, n, lwe.data());
    b = row[0];
  } else {
    for (int lane = 0; lane < 64; ++lane) dot += rs::au_lane_dot(row, n, lwe.data(), lane);
    b = row[n];
  }
  return (int32_t)rs::au_ksk_noise(b, dot, rs::au_ksk_message((uint32_t)(S_i_of_sample & 1), v, j, basebit));
}
// the report reduction: `count` noise words tallied by `parts` threads (word w by thread w % parts), the tallies then merged
void rs_emu_audit_reduce(const int32_t* noise, long count, uint32_t limit, int parts, uint32_t* max_abs, uint64_t* over) {
  std::vector<rs::AuTally> tally((size_t)parts, rs::AuTally{0u, 0ull});
  for (long w = 0; w < count; ++w) rs::au_tally_word(tally[(size_t)(w % parts)], (uint32_t)noise[w], limit);
  rs::AuTally all{0u, 0ull};
  for (int p = parts - 1; p >= 0; --p) rs::au_tally_merge(all, tally[(size_t)p]);
  *max_abs = all.max_abs;
  *over = all.over;
}

// ---- the packing key on the device (rs_pack_keygen_dev, rs_pack_expand_dev, rs_audit_pack_key_dev) through the functions of
// rs_packkey.h and rs_audit.h ----
static_assert(rs::kAuPackMask == (uint32_t)rs::kKgPackMask, "the audit restates the packing-key mask domain");
int rs_emu_pack_keygen_tile() { return rs::kPgTile; }
// pack_keygen_kernel for one row, tile by tile and thread by thread as the kernel places them: the window of ext = (-a, a) filled
// block by block from the row's ChaCha stream, one 4-word chunk per thread and four bits of S, the masked adds on the seven live
// words, noise and gadget word at the store -> body_row[N]
void rs_emu_pack_keygen_row(const uint8_t* mask_seed, const uint8_t* noise_seed, int N, int basebit, int t, uint64_t row,
                            const int32_t* lwe_key, int n, const int32_t* tlwe_key, double sigma, int32_t* body_row) {
  uint32_t key[8], nkey[8];
  rs::kg_seed_words(mask_seed, key);
  rs::kg_seed_words(noise_seed, nkey);
  const std::vector<uint32_t> lwe = emu_pack_bits(lwe_key, n), S = emu_pack_bits(tlwe_key, N);
  const int tiles = N / rs::kPgTile;
  std::vector<uint32_t> win((size_t)N + rs::kPgTile);
  for (int tile = 0; tile < tiles; ++tile) {
    const int k0 = tile * rs::kPgTile;
    for (int th = 0; th < rs::kPgThreads; ++th)
      for (int wb = th; wb < rs::pg_window_blocks(N); wb += rs::kPgThreads) {
        uint32_t w[16];
        rs::pg_window_block(key, row, N, k0, wb, w);
        for (int q = 0; q < 16; ++q) win[16 * (size_t)wb + q] = w[q];
      }
    for (int th = 0; th < rs::kPgThreads; ++th) {
      uint32_t acc[rs::kPgKpt] = {0u, 0u, 0u, 0u};
      int c4 = th + N / 4;
      const uint32_t* hi = &win[4 * (size_t)c4];
      for (int wd = 0; wd < N / 32; ++wd)
        for (int g = 0; g < 8; ++g) {
          const uint32_t* lo = &win[4 * (size_t)(--c4)];
          const uint32_t w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          for (int b = 0; b < 4; ++b) {
            const uint32_t m = 0u - ((S[wd] >> (4 * g + b)) & 1u);
            for (int q = 0; q < rs::kPgKpt; ++q) acc[q] += w[4 + q - b] & m;
          }
          hi = lo;
        }
      const int k = k0 + rs::kPgKpt * th;
      int32_t e[4];
      rs::pg_noise4(nkey, row, k, sigma, e);
      uint32_t v[rs::kPgKpt];
      for (int q = 0; q < rs::kPgKpt; ++q) v[q] = acc[q] + (uint32_t)e[q];
      if (k == 0) {
        int i, j;
        rs::pg_row(row, t, i, j);
        v[0] += rs::pg_key_bit(lwe.data(), i) * rs::pg_gadget(j, basebit);
      }
      for (int q = 0; q < rs::kPgKpt; ++q) body_row[k + q] = (int32_t)v[q];
    }
  }
}
// pack_expand_kernel for one row (the items row N/16 + blk of the flat grid): thread blk stores mask block blk, the body is copied
// word blk + T r -> out[2][N]
void rs_emu_pack_expand_row(const uint8_t* mask_seed, int N, uint64_t row, const int32_t* body_row, int32_t* out) {
  uint32_t key[8];
  rs::kg_seed_words(mask_seed, key);
  const int T = N / 16;
  for (int blk = 0; blk < T; ++blk) {
    uint32_t w[16];
    rs::pg_mask_block(key, row, blk, w);
    for (int q = 0; q < 16; ++q) out[16 * blk + q] = (int32_t)w[q];
    for (int r = 0; r < 16; ++r) out[N + blk + T * r] = body_row[blk + T * r];
  }
}
// audit_pack_kernel: the noise words of packing-key row `row`. seeded = 0: stored = the full key's row int32[2][N]; seeded = 1:
// stored = the body row int32[N], the mask regenerated from mask_seed. -> noise[N]
void rs_emu_audit_pack_row(int seeded, const uint8_t* mask_seed, int N, int t, int basebit, uint64_t row, const int32_t* stored,
                           const int32_t* lwe_key, int n, const int32_t* tlwe_key, int32_t* noise) {
  const std::vector<uint32_t> lwe = emu_pack_bits(lwe_key, n), S = emu_pack_bits(tlwe_key, N);
  std::vector<uint16_t> list((size_t)N);
  int cnt = 0;
  for (int w = 0; w < N / 32; ++w) cnt = rs::au_list_word(S[w], w, cnt, list.data());
  std::vector<uint32_t> a((size_t)N);
  const uint32_t* b_row;
  if (seeded) {
    uint32_t key[8];
    rs::kg_seed_words(mask_seed, key);
    for (int th = 0; th < rs::kAuThreads; ++th)
      for (int blk = th; blk < N / 16; blk += rs::kAuThreads) {
        uint32_t w[16];
        rs::au_pack_mask_block(key, row, blk, w);
        for (int q = 0; q < 16; ++q) a[16 * blk + q] = w[q];
      }
    b_row = reinterpret_cast<const uint32_t*>(stored);
  } else {
    for (int k = 0; k < N; ++k) a[k] = (uint32_t)stored[k];
    b_row = reinterpret_cast<const uint32_t*>(stored) + N;
  }
  int i, j;
  rs::au_pack_row(row, t, i, j);
  const uint32_t s = rs::au_key_bit(lwe.data(), i), g = rs::au_gadget(j, basebit);
  for (int th = 0; th < rs::kAuThreads; ++th)
    for (int k0 = th; k0 < N; k0 += rs::kAuThreads * rs::kAuKpt) {
      uint32_t acc[rs::kAuKpt];
      rs::au_bk_products(a.data(), N, list.data(), cnt, k0, acc);
      for (int q = 0; q < rs::kAuKpt; ++q) {
        const int k = k0 + rs::kAuThreads * q;
        noise[k] = (int32_t)rs::au_bk_noise(b_row[k], acc[q], rs::au_bk_message(1, s, g, k, 0u));
      }
    }
}

// ---- indexed gate batches (rs_gate_rows_dev, rs_gate3_dev) through the functions of rs_rows.h, as gate_rows_kernel places them: a
// wave of 64 lanes per row ----
// the row-op table: out4 = (c0, c1, c2, bconst); returns 0 for an op outside the table
int rs_emu_row_coef(int op, int32_t* out4) {
  rs::RowCoef g;
  if (!rs::row_coef(op, &g)) return 0;
  for (int j = 0; j < 3; ++j) out4[j] = g.c[j];
  out4[3] = (int32_t)g.bconst;
  return 1;
}
// gate_rows_kernel: the materialised combinations out[B][W]. src0..2: the three bases ([in_rows][W]); idx int32[B][3] or null (identity);
// n_groups groups of (ops[g], counts[g]) whose counts sum to B. Returns 0, or -1 for arguments the host entry points refuse.
int rs_emu_gate_rows(const int32_t* src0, const int32_t* src1, const int32_t* src2, long in_rows, const int32_t* idx, const int32_t* ops,
                     const long* counts, int n_groups, int W, long B, int32_t* out) {
  if (n_groups < 1 || n_groups > rs::kRowMaxGroups) return -1;
  rs::GateRowsArgs a{};
  long total = 0;
  for (int g = 0; g < n_groups; ++g) {
    rs::RowCoef unused;
    if (!rs::row_coef(ops[g], &unused) || counts[g] < 0) return -1;
    total += counts[g];
    a.groups.end[g] = total;
    a.groups.op[g] = ops[g];
  }
  if (total != B) return -1;
  a.groups.count = n_groups;
  a.src[0] = src0; a.src[1] = src1; a.src[2] = src2;
  a.idx = idx; a.in_rows = in_rows; a.out = out; a.B = B; a.W = W;
  for (long r = 0; r < B; ++r)
    for (int lane = 0; lane < 64; ++lane) rs::row_lane(a, r, lane);
  return 0;
}

// ---- compiled circuits (rs_circuit_create, rs_circuit_run_dev) through the functions of rs_circuit.h ----
// the host validation of rs_circuit_create: 0, or -1 for what it refuses. cells: rs_cell[n_cells]
int rs_emu_circuit_check(const void* cells, size_t n_cells, const uint32_t* level_end, size_t n_levels, size_t n_inputs) {
  return rs::circuit_check(static_cast<const rs::Cell*>(cells), n_cells, level_end, n_levels, n_inputs, nullptr);
}
// circuit_rows_kernel on one level (cells [first, first + C), the last M of them MUX): the staged rows out[(C + M) lanes][W] from
// arena[wires][lanes][W], a wave of 64 lanes per row. Returns 0, or -1 for a shape the launcher refuses.
int rs_emu_circuit_rows(const void* cells, long first, long C_, long M, long lanes, const int32_t* arena, int W, int32_t* out) {
  if (C_ <= 0 || M < 0 || M > C_ || lanes <= 0 || first < 0 || W < 1 || !cells || !arena || !out) return -1;
  rs::CircuitLevelArgs a{};
  a.cells = static_cast<const rs::Cell*>(cells); a.arena = arena; a.out = out;
  a.first = first; a.C = C_; a.M = M; a.lanes = lanes; a.W = W;
  for (long r = 0; r < rs::circuit_level_rows(a); ++r)
    for (int lane = 0; lane < 64; ++lane) rs::circuit_row_lane(a, r, lane);
  return 0;
}
// circuit_fold_kernel: u[(B + mux_rows)][words], MUX row m (the row B - mux_rows + m) += row B + m + (0, 1/8)
int rs_emu_circuit_fold(int32_t* u, long B, long mux_rows, int words) {
  if (!u || mux_rows < 0 || mux_rows > B || words < 1) return -1;
  rs::CircuitFoldArgs a{u, B, mux_rows, words};
  for (long m = 0; m < mux_rows; ++m)
    for (int lane = 0; lane < 64; ++lane) rs::circuit_fold_lane(a, m, lane);
  return 0;
}

// ---- sparse bootstraps (rs_bootstrap_sparse_dev) through the functions of rs_sparse.h, as the kernels of rs_sparse.hip place them:
// a wave of 64 lanes per row ----
// the b word of the bootstrapped trivial sample (0, ..., 0, b) on the ring N = 2^logn
int32_t rs_emu_sparse_trivial(int32_t b, int32_t mu, int logn) { return rs::sparse_trivial_word(b, mu, logn); }
// the host validation of rs_bootstrap_sparse_dev: 0, or -1 for what it refuses (the pointers are only compared with null)
int rs_emu_sparse_check(const void* out, const void* in, const void* live, size_t B, size_t n_live, size_t W) {
  return rs::sparse_check(out, in, live, B, n_live, W, nullptr);
}
// sparse_gather_kernel: rows[n_live][W] = in[live[i]], the zero sample for an entry outside [0, B)
int rs_emu_sparse_gather(const int32_t* in, const int32_t* live, long n_live, long B, int W, int32_t* rows) {
  if (rs::sparse_check(in, in, live, (size_t)B, (size_t)n_live, (size_t)W, nullptr) != 0 || B < 0 || n_live < 0 || W < 1 || !rows) return -1;
  rs::SparseArgs a{};
  a.in = in; a.live = live; a.rows = rows; a.B = B; a.n_live = n_live; a.W = W;
  for (long i = 0; i < n_live; ++i)
    for (int lane = 0; lane < 64; ++lane) rs::sparse_gather_lane(a, i, lane);
  return 0;
}
// sparse_fill_kernel: out[B][W] = the trivial results of in's b words; out may be in (word n of a row is read before its lanes store)
int rs_emu_sparse_fill(const int32_t* in, int32_t* out, long B, int W, int32_t mu, int logn) {
  if (!in || !out || B < 0 || W < 1 || logn < rs::kGenMinLogN || logn > rs::kGenMaxLogN) return -1;
  rs::SparseArgs a{};
  a.in = in; a.out = out; a.B = B; a.W = W; a.mu = mu; a.logn = logn;
  for (long r = 0; r < B; ++r) {
    const int32_t b = a.in[r * a.W + a.W - 1];
    for (int lane = 0; lane < 64; ++lane) rs::sparse_fill_lane(a, r, lane, b);
  }
  return 0;
}
// sparse_scatter_kernel: out[live[i]] = boot[i]; an entry outside [0, B) writes nothing
int rs_emu_sparse_scatter(int32_t* out, const int32_t* boot, const int32_t* live, long n_live, long B, int W) {
  if (rs::sparse_check(out, out, live, (size_t)B, (size_t)n_live, (size_t)W, nullptr) != 0 || B < 0 || n_live < 0 || W < 1 || !boot) return -1;
  rs::SparseArgs a{};
  a.out = out; a.boot = boot; a.live = live; a.B = B; a.n_live = n_live; a.W = W;
  for (long i = 0; i < n_live; ++i)
    for (int lane = 0; lane < 64; ++lane) rs::sparse_scatter_lane(a, i, lane);
  return 0;
}

}  // extern "C"
