// rs_api_internal.h -- what the three units of the C ABI share (rs_api.cpp, rs_api_keys.cpp, rs_api_client.cpp): the error
// report, the context and its per-stream lanes, and the few functions that cross a unit boundary. Host code only; not installed.
//
//   rs_api.cpp          context, lanes, the bootstrapped path, the linear stage, certificates, timing, memory helpers
//   rs_api_keys.cpp     loading an evaluation key; generating and expanding one on the device
//   rs_api_client.cpp   key material and client-side calls that need no lane, no launch plan and no loaded key; the ONE path of
//                       a secret key onto the device and back off it (with_secret_copy)
#pragma once

#include "redsec_hip.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <vector>

#include "rs_circuit.h"
#include "rs_host.h"
#include "rs_kernels.h"
#include "rs_ring_selector.h"

#define RS_HIP(call)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) return rs::fail(RS_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// Everything a launch writes besides its outputs lives in a LANE = the per-stream slice of a context:
// the extracted-sample workspace between blind rotation and keyswitch, the persistent-wave work counter,
// the certificate slots, the convolution scratch and the timing events. Calls on DIFFERENT streams of one
// context therefore never share mutable state (calls on one stream are ordered by the stream itself).
constexpr unsigned kCertSlots = 1024;   // ring of per-call certificate slots; slot kCertSlots = running max, +1 = recomputed calls
struct Lane {
  hipStream_t stream = nullptr;
  int32_t* d_u0 = nullptr;
  int32_t* d_u1 = nullptr;
  size_t ws_batch = 0;
  size_t sample_words = rs::kN + 1;       // words of one extracted sample (N + 1)
  unsigned int* d_counter = nullptr;      // work counter of the persistent blind-rotate launches
  unsigned long long* d_cert = nullptr;   // [kCertSlots + 2]
  unsigned slot_next = 0;
  uint32_t* d_conv_scratch = nullptr;     // expanded weights of the tiled convolution (grown on demand)
  size_t conv_scratch_words = 0;
  uint32_t* d_ks_scratch = nullptr;       // partial sums of the sliced (small-batch) keyswitch (grown on demand; <= ~50 MB)
  size_t ks_scratch_words = 0;
  int* d_progress = nullptr;              // XCD cohort table of the split lock-step kernel: [8][kCohortSlots] step counts
  int32_t* d_rows = nullptr;              // materialised combinations of the indexed gate batches: [rows_batch][n + 1] (grown on demand)
  size_t rows_batch = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool ev_valid = false;
  rs::LaunchInfo last;
  rs::KsPlan last_ks; bool ks_ran = false;   // form of the last keyswitch on this stream (rs_last_keyswitch)
  // enforced split-mode certificate: the lane's running maximum is copied here (pinned host memory) behind every general-kernel
  // call, and looked at by the next call, rs_certify and rs_sync
  unsigned long long* h_split_max = nullptr;
};

// A compiled circuit (rs_circuit_create): the validated cell table on the device and the level cuts on the host. It belongs to
// its context, which keeps the set of live handles: a handle that is not in the set is refused, never followed.
struct rs_circuit {
  rs::Cell* d_cells = nullptr;
  std::vector<uint32_t> level_end, level_mux;   // per level: one past its last cell, and how many of its cells (the last ones) are MUX
  size_t n_cells = 0, n_inputs = 0;
  size_t widest = 0;                            // max over the levels of cells + MUX cells: staged rows per lane
};

struct rs_ctx {
  rs_params p{};
  int device = 0;
  int cfg = 0;  // 0 default128-shaped gadget, 1 redsec_v2-shaped gadget
  rs::Tables tables;
  int mode = 1;  // RS_MODE_FFT by default; RS_MODE_EXACT_NTT = 0
  double cert_limit = RS_CERTIFICATE_LIMIT;
  rs::LaunchOpts opts;
  int ks_force = rs::kKsAuto;      // RS_KS_FORM=wide|tiled (diagnostic, read once in rs_create): rs_host.h keyswitch_form
  int sel_force = rs::kSeAuto;     // RS_SEL_FORM=wide|chunked (diagnostic, read once in rs_create): rs_ring_selector.h selector_form
  std::atomic<int> sel_form{-1};   // form and workgroups of the last selector keyswitch of this context (rs_last_selector)
  std::atomic<long> sel_groups{0};
  double* d_tw = nullptr;          // exact-NTT tables (kTwTotal doubles)
  double* d_tw_fft = nullptr;      // FFT tables (kFftTwDoubles doubles)
  double* d_bk_ntt = nullptr;      // key in the NTT domain
  double* d_bk_fft = nullptr;      // key in the FFT domain
  // general ring path (rs_general.h): every parameter set has it; sets outside the specialised N = 1024 kernels
  // (`general`) have nothing else
  bool general = false;
  int wgs_cfg = -1;                // gadget id of the lock-step split-key kernel, or -1 (general kernels only)
  int logn = 10;
  double split_bound = 0.0;        // a-priori error bound of the split-key product (rs_general.h; the mode is offered below 1/2)
  double split_cert_limit = 0.25;    // enforced on the general kernels' rounding distances (REDSEC_SPLIT_CERT_LIMIT lowers it: tests)
  std::atomic<bool> inexact{false};  // a split-mode call rounded a value 1/4 or more away from an integer: sticky, RS_ERR_INEXACT
  double* d_tw_gen = nullptr;      // gen_make_twiddles(logn)
  double* d_bk_gen = nullptr;      // split key in the FFT domain
  int32_t* d_ksk = nullptr;
  size_t bk_bytes = 0, ksk_bytes = 0;
  bool keys = false;
  int num_cus = 256;
  bool timing = false;
  std::mutex lanes_mu;                              // guards the map (a lane itself belongs to its stream's caller)
  std::map<hipStream_t, std::unique_ptr<Lane>> lanes;
  std::mutex host_mu;                               // serialises the synchronous host-pointer calls (shared staging buffers)
  int32_t* d_io[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t io_batch = 0;
  // rs_allgather_rows: private copy stream, "my slice is computed" / "my copies are done" events, peers already enabled
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_slice = nullptr, ev_copied = nullptr, ev_staged = nullptr;
  bool copied_recorded = false;
  std::vector<int> peers_enabled, peers_denied;
  int32_t* h_stage = nullptr;                       // pinned staging buffer of this context's slice (host-staged exchange only)
  size_t h_stage_bytes = 0;
  std::mutex circuits_mu;
  std::set<rs_circuit*> circuits;                   // live handles of rs_circuit_create
};

// what crosses a unit boundary (linked across objects, as the launch_* functions of the kernel units)
namespace rs {

// rs_api.cpp
int fail(int code, const char* fmt, ...);   // sets rs_last_error() of this thread; returns code
int use_device(rs_ctx* c);                      // refuses a null context; hipSetDevice

// rs_api_client.cpp: secret keys and seeds
inline bool deviation_ok(double stdev) { return std::isfinite(stdev) && stdev >= 0.0; }
// RS_OK, or the refusal of a noise seed that equals the public mask seed
int refuse_equal_seeds(const uint8_t* mask_seed, const uint8_t* noise_seed);
// lwe_key [n] then tlwe_key [N], 0/1 words, appended to `out` `per_word` to a word (32: bits; 1: the words themselves), each key
// from a fresh word on; *lwe_words = the words lwe_key took. A word outside {0, 1} wipes `out` and is refused by key and index.
int pack_key_pair(const rs_params& p, const int32_t* lwe_key, const int32_t* tlwe_key, int per_word, std::vector<uint32_t>& out,
                  size_t* lwe_words);
// run(d_words, d_extra) with a private device buffer that holds `words` followed, at the next 16-byte boundary, by `extra` zeroed
// bytes. The secret leaves the device (and `words`) before this returns, on the error paths too.
int with_secret_copy(std::vector<uint32_t>& words, size_t extra, const std::function<int(const uint32_t*, char*)>& run);

}  // namespace rs
