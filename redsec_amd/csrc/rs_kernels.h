// rs_kernels.h -- kernel argument blocks and launchers (internal; the public boundary is
// include/redsec_hip.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_launch_plan.h"
#include "rs_ntt.h"
#include "rs_rows.h"

namespace rs {

struct BlindRotateArgs {
  const int32_t* in0;   // [B][W]
  const int32_t* in1;   // [B][W] or nullptr
  int32_t c0, c1;       // x = c0*in0 + c1*in1 (word-wise, wrapping)
  int32_t bconst;       // added to the b word
  int32_t mu;           // test-vector value
  const double* bk_x;   // transform-domain key of the active mode: [n][2l][2][8][64][2]
  const double* tw;     // twiddle tables of the active mode
  Field f;
  int32_t n;
  int32_t W;            // n + 1
  long B;
  int32_t* u_out;       // [B][N+1] extracted samples
  unsigned int* counter;  // persistent-wave work counter (device), or nullptr
  unsigned long long* dev_flag;  // FFT mode: this CALL's certificate slot (max rounding distance, double bits), or nullptr
  // Programmable form (tfhe_blindRotateAndExtract_FFT's test polynomial): ciphertext b starts from
  // lut[(b % lut_count)][N] instead of the constant mu. nullptr = constant test vector.
  const int32_t* lut = nullptr;
  int32_t lut_count = 0;
  int32_t lut_first = 0;   // table of ciphertext 0 (a caller's shard offset modulo lut_count)
  // Conditional exact recomputation (exact-NTT kernels launched behind an FFT call): the grid reads the
  // FFT call's certificate slot and returns at once unless it reached `gate_limit_bits`; either way it folds
  // the slot into the stream's running maximum and counts the recomputed calls.
  const unsigned long long* gate_flag = nullptr;
  unsigned long long gate_limit_bits = 0;
  unsigned long long* running_flag = nullptr;
  unsigned long long* fallback_count = nullptr;
  // XCD cohorts (blind_rotate_wgs_kernel): progress[xcd * kCohortSlots + slot] = CMUX steps workgroup (xcd, slot) has done,
  // INT_MAX-like for a workgroup that is absent or finished (the launcher fills the table with 0x7f bytes). A workgroup that
  // is more than `cohort_lag` steps ahead of the slowest workgroup on its XCD waits (bounded) every `cohort_every` steps, so
  // the workgroups of an XCD stay within what their L2 holds of the key. nullptr: free-running.
  int* progress = nullptr;
  int32_t cohort_every = 0, cohort_lag = 0;
};
// (LaunchOpts, the kForm* ids, LaunchInfo and kCohortSlots: rs_launch_plan.h)

struct KeyswitchArgs {
  const int32_t* u0;    // [B][N+1]
  const int32_t* u1;    // optional second addend (bootsMUX)
  int32_t bconst;       // added to the b word of u
  const int32_t* ksk;   // [N][t][base][W]
  int32_t W, t, basebit;
  long B;
  int32_t* out;         // [B][W]
  int32_t N = kN;       // ring degree of the extracted samples (the tiled kernels are N = 1024 only)
  // Small batches: the N input coefficients are cut into slices (blockIdx.z) so that enough workgroups exist; with a scratch
  // of keyswitch_scratch_words() words every slice stores its partial sums there ([slice][W][B], ciphertext fastest: coalesced)
  // and keyswitch_reduce_kernel sums them into `out`. Without one (or one too small) the slices meet by integer atomics in a
  // zeroed output (the round-1 form: 17 G uncoalesced atomics/s were what bounded it, profiles/r03/y_ab_*).
  uint32_t* scratch = nullptr;
  size_t scratch_words = 0;
};
size_t keyswitch_scratch_words(const KeyswitchArgs& a);   // 0 when the launch will not be sliced

// General ring path (rs_general.h / rs_general.hip): any N = 2^logn in [1024, 8192], any gadget, split key.
struct GenArgs {
  const int32_t* in0;   // [B][W]
  const int32_t* in1;   // [B][W] or nullptr
  int32_t c0, c1, bconst, mu;
  const double* bk_x;   // [n][2l][2 halves][2 columns][8][N/16][2]
  const double* tw;     // gen_make_twiddles(logn)
  int32_t n, W, l, bgbit;
  long B;
  int32_t* u_out;       // [B][N+1]
  const int32_t* lut = nullptr;   // programmable form, as in BlindRotateArgs
  int32_t lut_count = 0, lut_first = 0;
  unsigned long long* dev_flag = nullptr;   // optional: largest rounding distance (diagnostic; exactness does not depend on it)
};

struct ConvShape { int32_t H, Wd, Cin, Cout, fh, fw, stride_h, stride_w, off_h, off_w, Ho, Wo; };
struct PoolShape { int32_t H, Wd, C, win_h, win_w, stride_h, stride_w, off_h, off_w, Ho, Wo; };

// cfg: 0 = CfgDefault128 (l=3, Bgbit=7), 1 = CfgRedsecV2 (l=10, Bgbit=3); mode: 0 = exact NTT, 1 = FFT
hipError_t launch_blind_rotate(int cfg, int mode, const BlindRotateArgs& a, int num_cus, const LaunchOpts& opts, hipStream_t st,
                               LaunchInfo* info = nullptr);
hipError_t launch_blind_rotate_split_wg(int cfg, const BlindRotateArgs& a, int num_cus, const LaunchOpts& opts, hipStream_t st, LaunchInfo* info);
hipError_t launch_bk_transform(int cfg, int mode, const int32_t* bk, double* bk_x, const double* tw, Field f, double scale,
                               long n_polys, hipStream_t st);
// Dispatches on keyswitch_form (rs_host.h): `force` is a KsForm (kKsAuto = -1: by batch size), `ran` receives the form taken.
struct KsPlan;
hipError_t launch_keyswitch(const KeyswitchArgs& a, hipStream_t st, int num_cus, int force = -1, KsPlan* ran = nullptr);
hipError_t launch_keyswitch_wide(const KeyswitchArgs& a, hipStream_t st);   // rs_keyswitch_wide.hip: 1,024 ciphertexts per workgroup
hipError_t launch_gen_blind_rotate(int logn, const GenArgs& a, int num_cus, hipStream_t st);
long gen_resident_ciphertexts(int logn, int num_cus);   // workgroups (= ciphertexts) the general kernel keeps resident
hipError_t launch_gen_bk_transform(int logn, const int32_t* bk, double* bk_x, const double* tw, long n_polys, int num_cus, hipStream_t st);
hipError_t launch_gen_polymul(int logn, const int32_t* a_small, const int32_t* b_torus, int32_t* out, double* scratch, const double* tw,
                              long count, unsigned long long* dev_flag, int num_cus, hipStream_t st);
// evaluation-key generation (rs_keygen_dev; streams of rs_keygen.h): bk rows [n][2l][2][N] and ksk samples [N][t][2^basebit][n+1]
struct KeygenArgs {
  int32_t* bk; int32_t* ksk;                          // compressed: the bodies bk_body [n][2l][N], ksk_body [N][t][2^basebit]
  const int32_t* lwe_key; const int32_t* tlwe_key;   // device copies, values 0 / 1
  uint32_t seed[8];                                   // masks (domains 3, 5); noise too unless compressed
  uint32_t noise_seed[8];                             // compressed: noise (domains 4, 6)
  int compressed;                                     // 1: bodies only, the c = 0 gadget term moved into the body (rs_keygen_compressed_dev)
  int n, N, l, bgbit, t, basebit;
  double bk_sigma, ks_sigma;
  unsigned long long* dev_flag;                       // largest rounding distance of the a*S products
};
hipError_t launch_keygen_bk(int logn, const KeygenArgs& a, const double* tw, int num_cus, hipStream_t st);
hipError_t launch_keygen_ksk(const KeygenArgs& a, int num_cus, hipStream_t st);
// expansion of a compressed key (rs_expand_keys_dev): the masks regenerated from the mask seed, the bodies copied beside them
struct ExpandArgs {
  int32_t* bk; int32_t* ksk;                          // full layouts of rs_load_keys (bk 16-byte aligned)
  const int32_t* bk_body; const int32_t* ksk_body;    // [n][2l][N], [N][t][2^basebit]
  uint32_t seed[8];                                   // the mask seed
  int n, N, l, t, basebit;
};
hipError_t launch_expand_bk(int logn, const ExpandArgs& a, int num_cus, hipStream_t st);
hipError_t launch_expand_ksk(const ExpandArgs& a, int num_cus, hipStream_t st);
// seeded LWE ciphertexts (rs_encrypt_seeded_dev, rs_expand_ciphertexts_dev; streams and placement of rs_keygen.h): ciphertext i has
// row first + i, its mask the domain-7 words of the mask seed; encryption forms body = sum_k a_k s_k + e + mu
struct SeededArgs {
  int32_t* ct;                                        // [B][n+1] (16-byte alignment not needed), or nullptr: bodies only (encryption)
  int32_t* body;                                      // [B]: written by encryption, read by expansion
  const int32_t* mu;                                  // [B] torus messages (encryption)
  const uint32_t* key_bits;                           // private device copy of the LWE key, 32 bits per word, zero past n (encryption)
  uint32_t seed[8];                                   // mask seed (domain 7)
  uint32_t noise_seed[8];                             // noise seed (domain 8, encryption)
  uint64_t first;
  long B;
  int n, tile;                                        // tile = kg_ct_tile(n)
  double sigma;
};
hipError_t launch_encrypt_seeded(const SeededArgs& a, int num_cus, hipStream_t st);
hipError_t launch_expand_ciphertexts(const SeededArgs& a, int num_cus, hipStream_t st);
// public-key encryption (rs_pk_encrypt_dev; selection stream and placement of rs_keygen.h): ciphertext i has row first + i, its
// selection bits the domain-9 words of the rand seed; ct[i] = base[i] + (0, mu[i]) + the selected rows of pk
struct PkArgs {
  int32_t* ct;                                        // [B][n+1]; may be `base`
  const int32_t* pk;                                  // [m][n+1] encryptions of zero
  const int32_t* mu;                                  // [B] torus messages, or nullptr
  const int32_t* base;                                // [B][n+1], or nullptr
  uint32_t seed[8];                                   // the encryptor's rand seed (domain 9): travels as a kernel argument only
  uint64_t first;
  long B, m;
  int n;
};
hipError_t launch_pk_encrypt(const PkArgs& a, hipStream_t st);
// compact RLWE public keys (rs_rlwe_pk_encrypt_dev, rs_rlwe_extract_dev; streams, placement and index arithmetic of rs_rlwe.h):
// ciphertext r has row first + r of the rand seed and carries messages rN .. rN + N - 1
struct RlweEncArgs {
  int32_t* rlwe;                                      // [ceil(count / N)][2][N]
  const int32_t* pk;                                  // [2][N]: a, then b = a*S + e
  const int32_t* mu;                                  // [count] torus messages
  uint32_t seed[8];                                   // the encryptor's rand seed (domains 12, 13): travels as a kernel argument only
  uint64_t first;
  long count;
  int N;
  double sigma;
};
hipError_t launch_rlwe_pk_encrypt(const RlweEncArgs& a, hipStream_t st);
struct RlweExtractArgs {
  int32_t* u;                                         // [count][N+1]
  const int32_t* rlwe;                                // [ceil(count / N)][2][N]
  long count;
  int N;
};
hipError_t launch_rlwe_extract(const RlweExtractArgs& x, hipStream_t st);
// packed results (rs_pack_dev; placement and index arithmetic of rs_pack.h): ciphertext r packs samples rN .. rN + N - 1
struct PackArgs {
  int32_t* rlwe;                                      // [ceil(count / N)][2][N]
  const int32_t* ct;                                  // [count][n+1]
  const int32_t* key;                                 // [n][t][2][N]: the packing key
  long count;
  int n, N, basebit, t;
};
hipError_t launch_pack(const PackArgs& a, hipStream_t st);
// re-keying (rs_rekey_dev; placement and index arithmetic of rs_rekey.h): both dimensions are the caller's, not the context's
struct RekeyArgs {
  int32_t* out;                                       // [B][n_dst+1]
  const int32_t* ct;                                  // [B][n_src+1]
  const int32_t* key;                                 // [n_src][t][n_dst+1]: the re-keying key
  long B;
  int n_src, n_dst, basebit, t;
};
hipError_t launch_rekey(const RekeyArgs& a, hipStream_t st);
// ring re-keying (rs_ring_rekey_dev; placement and index arithmetic of rs_ring_rekey.h)
struct RingRekeyArgs {
  int32_t* out;                                       // [R][2][N]
  const int32_t* rlwe;                                // [R][2][N]
  const int32_t* key;                                 // [t+1][2][N]: the ring re-keying key, row t the constant row
  long R;
  int N, basebit, t;
};
hipError_t launch_ring_rekey(const RingRekeyArgs& a, hipStream_t st);
// encrypted selection (rs_ring_cmux_dev, rs_ring_lookup_dev; placement and index arithmetic of rs_ring_cmux.h)
struct RingCmuxArgs {
  int32_t* out;                                       // [R][2][N], contiguous
  const int32_t* d1;                                  // row r at d1 + r stride 2 N; null: the all-zero ciphertext
  const int32_t* d0;                                  // row r at d0 + r stride 2 N
  const int32_t* sel;                                 // [2l][2][N]: one RGSW sample
  long R, stride;
  int N, basebit, l;
  int form = 0;                                       // kRcSigned (rs_ring_cmux.h) or kRcAlternating: the digit
};
hipError_t launch_ring_cmux(const RingCmuxArgs& a, hipStream_t st);      // ring_cmux_init_kernel, then the kernel of a.form
hipError_t launch_ring_cmux_alt(const RingCmuxArgs& a, hipStream_t st);  // ring_cmux_alt_kernel alone (rs_ring_cmux_alt.hip): launch_ring_cmux calls it
// encrypted rotation (rs_ring_rotate_dev, rs_ring_heads_dev; index arithmetic of rs_ring_rotate.h): ONE level of a chain
struct RingRotateArgs {
  int32_t* out;                                       // [R][2][N], contiguous
  const int32_t* in;                                  // row r at in + r stride 2 N (stride 0: every row reads in[0])
  const int32_t* sel;                                 // the level's sample [2l][2][N] of row r at sel + r sel_stride
  long R, stride;
  size_t sel_stride;                                  // words between the samples of consecutive rows; 0: one sample for all
  int N, basebit, l;
  int e;                                              // the level's exponent, 0 .. 2 N - 1
  int form;                                           // kRcSigned or kRcAlternating (rs_ring_cmux.h)
};
hipError_t launch_ring_rotate_level(const RingRotateArgs& a, hipStream_t st);   // ring_rotate_init_kernel, then the kernel of a.form (e = 0: the copy alone)
struct RingHeadsArgs {
  int32_t* u;                                         // [R width][N+1]
  const int32_t* rlwe;                                // [R][2][N]
  long R;
  int width, N;
};
hipError_t launch_ring_heads(const RingHeadsArgs& x, hipStream_t st);
// batched encrypted lookup (rs_ring_lookup_rows_dev; index arithmetic of rs_ring_lookup.h): ONE level of R CMUX trees
struct RingLookupArgs {
  int32_t* out;                                       // [R][ceil(rows / 2)][2][N], contiguous
  const int32_t* in;                                  // entry e < rows of row q at in + (q row_stride + e entry_stride) 2 N
  const int32_t* sel;                                 // sample k [2l][2][N] of row q at sel + q sel_row_stride + k 2l 2 N
  long R, rows;                                       // tables, and the ciphertexts of each that enter this level (1 .. 2^30)
  size_t row_stride, entry_stride;                    // in ciphertexts
  size_t sel_row_stride;                              // words between the sets of consecutive rows; 0: one set for all
  int k;                                              // the level
  int N, basebit, l;
  int form;                                           // kRcSigned or kRcAlternating (rs_ring_cmux.h)
};
hipError_t launch_ring_lookup_level(const RingLookupArgs& a, hipStream_t st);   // ring_lookup_init_kernel, then the kernel of a.form
// the selector keyswitch of circuit bootstrapping (rs_ring_selector_dev; placement and index arithmetic of rs_ring_selector.h)
struct RingSelectorArgs {
  int32_t* sel;                                       // [rows / l][2l][2][N]
  const int32_t* ct;                                  // [rows][n_src+1]: row k l + j the bootstrap of bit k at level j
  const int32_t* key;                                 // [2][n_src+1][ks_t][2][N], 16-byte aligned
  long rows;                                          // depth l
  int N, n_src, basebit, l, ks_basebit, ks_t;
};
hipError_t launch_ring_selector(const RingSelectorArgs& a, hipStream_t st);
// the same words from ring_selector_wide_kernel (rs_ring_selector_wide.hip): all coordinates in one workgroup, plain 16-byte stores;
// sel 16-byte aligned. Which of the two a batch call takes: selector_form (rs_ring_selector.h)
hipError_t launch_ring_selector_wide(const RingSelectorArgs& a, hipStream_t st);
// rs_circuit_bootstrap_dev: lut[j] = the constant polynomial h_j / 2, index[r] = r / l (the gather that replicates each bit l times)
struct CircuitPrepareArgs {
  int32_t* lut;                                       // [l][N]
  int32_t* index;                                     // [rows]
  long rows;
  int N, basebit, l;
};
hipError_t launch_circuit_prepare(const CircuitPrepareArgs& a, hipStream_t st);
// the packing key on the device (rs_pack_keygen_dev, rs_pack_expand_dev; streams and placement of rs_packkey.h): row i t + j is
// (a, a*S + e + s_i g_j X^0), a the domain-14 words of the mask seed, e the domain-15 Gaussians of the noise seed
struct PackKeygenArgs {
  int32_t* body;                                      // [n][t][N]
  const uint32_t* lwe_bits; const uint32_t* tlwe_bits;   // private device copies, 32 bits per word: [ceil(n / 32)], [N / 32]
  uint32_t seed[8];                                   // mask seed (domain 14)
  uint32_t noise_seed[8];                             // noise seed (domain 15): travels as a kernel argument only
  int n, N, basebit, t;
  double sigma;
};
hipError_t launch_pack_keygen(const PackKeygenArgs& a, hipStream_t st);
struct PackExpandArgs {
  int32_t* key;                                       // [n][t][2][N]
  const int32_t* body;                                // [n][t][N]
  uint32_t seed[8];                                   // mask seed (domain 14)
  long rows;                                          // n t
  int N;
};
hipError_t launch_pack_expand(const PackExpandArgs& a, hipStream_t st);
// device decryption and the exact noise audit of evaluation keys (rs_phase_dev, rs_audit_keys_dev, rs_audit_compressed_keys_dev;
// per-word arithmetic of rs_audit.h, 32-bit integer only). Secret keys are private device copies packed 32 bits per word.
constexpr int kAuMaxDim = 16384;                      // largest LWE dimension a packed key in LDS serves (rs_create's limit on n)
struct PhaseArgs {
  int32_t* phase;                                     // [B]
  const int32_t* ct;                                  // [B][dim+1]
  const uint32_t* key_bits;                           // [ceil(dim / 32)], zero past dim
  long B;
  int dim;
};
hipError_t launch_lwe_phase(const PhaseArgs& a, int num_cus, hipStream_t st);
struct AuditReportDev { unsigned long long bk_over, ksk_over, ksk_zero_bad; unsigned int bk_max_abs, ksk_max_abs; };   // zeroed by the caller
struct AuditArgs {
  const int32_t* bk; const int32_t* ksk;              // full key: layouts of rs_load_keys; compressed: the bodies [n][2l][N], [N][t][2^basebit]
  int32_t* bk_noise; int32_t* ksk_noise;              // optional outputs [n][2l][N], [N][t][2^basebit]
  const uint32_t* lwe_bits; const uint32_t* tlwe_bits;   // [ceil(n / 32)], [N / 32]
  uint32_t seed[8];                                   // compressed: the mask seed (domains 3, 5)
  int n, N, l, bgbit, t, basebit;
  uint32_t bk_limit, ksk_limit;
  AuditReportDev* report;
};
hipError_t launch_audit_bk(const AuditArgs& a, bool seeded, int num_cus, hipStream_t st);
hipError_t launch_audit_ksk(const AuditArgs& a, bool seeded, int num_cus, hipStream_t st);
// the same audit of a packing key (rs_audit_pack_key_dev): the c = 1 formula of a bk row with t digits of basebit bits; the tallies
// go to the bk fields of the report
struct AuditPackArgs {
  const int32_t* key;                                 // full key [n][t][2][N]; seeded: the bodies [n][t][N]
  int32_t* noise;                                     // optional output [n][t][N]
  const uint32_t* lwe_bits; const uint32_t* tlwe_bits;   // [ceil(n / 32)], [N / 32]
  uint32_t seed[8];                                   // seeded: the mask seed (domain 14)
  int n, N, t, basebit;
  uint32_t limit;
  AuditReportDev* report;
};
hipError_t launch_audit_pack(const AuditPackArgs& a, bool seeded, int num_cus, hipStream_t st);
// indexed gate batches (rs_gate_rows_dev, rs_gate3_dev): the combinations of GateRowsArgs (rs_rows.h) written to a.out
hipError_t launch_gate_rows(const GateRowsArgs& a, int num_cus, hipStream_t st);
// compiled circuits (rs_circuit_run_dev), per level: the staged combinations of CircuitLevelArgs (rs_circuit.h) written to a.out,
// and the fold of the MUX rows on the extracted samples
struct CircuitLevelArgs;
struct CircuitFoldArgs;
hipError_t launch_circuit_rows(const CircuitLevelArgs& a, int num_cus, hipStream_t st);
hipError_t launch_circuit_fold(const CircuitFoldArgs& a, int num_cus, hipStream_t st);
// sparse bootstraps (rs_bootstrap_sparse_dev): the rows of SparseArgs (rs_sparse.h) gathered into a.rows, the trivial results
// written to all of a.out, and a.boot scattered over the live rows of a.out
struct SparseArgs;
hipError_t launch_sparse_gather(const SparseArgs& a, int num_cus, hipStream_t st);
hipError_t launch_sparse_fill(const SparseArgs& a, int num_cus, hipStream_t st);
hipError_t launch_sparse_scatter(const SparseArgs& a, int num_cus, hipStream_t st);
hipError_t launch_polymul(int cfg, int mode, const int32_t* a_small, const int32_t* b_torus, int32_t* out, double* scratch,
                          const double* tw, Field f, double scale, long count, unsigned long long* dev_flag, hipStream_t st);
hipError_t launch_lincomb(int32_t* out, const int32_t* x, int32_t cx, const int32_t* y, int32_t cy, int32_t bconst, int W, long B,
                          hipStream_t st);
hipError_t launch_synthetic_words(int32_t* out, uint64_t seed, size_t total, hipStream_t st);
hipError_t launch_gather_rows(int32_t* out, const int32_t* in, const int32_t* idx, int W, long B, hipStream_t st);
hipError_t launch_linear_fc(int32_t* out, const int32_t* in, const uint8_t* sign, const uint8_t* zero, int K, int M, int W,
                            int32_t zero_tap_b, const int32_t* bias_b, int bias_depth, hipStream_t st);
size_t conv_tiled_scratch_words(const ConvShape& s);
hipError_t launch_conv_ternary_tiled(int32_t* out, const int32_t* in, const uint8_t* sign, const uint8_t* zero, const ConvShape& s, int W,
                                     const int32_t* bias_b, int bias_depth, uint32_t* scratch, hipStream_t st);
hipError_t launch_conv_ternary(int32_t* out, const int32_t* in, const uint8_t* sign, const uint8_t* zero, const ConvShape& s, int W,
                               int32_t zero_tap_b, int32_t pad_tap_b, const int32_t* bias_b, int bias_depth, hipStream_t st);
hipError_t launch_fp64_rate(double* out, int num_cus, int iters, double* lane_ops, hipStream_t st);
hipError_t launch_sumpool(int32_t* out, const int32_t* in, const PoolShape& s, int W, const int32_t* bias_b, int bias_depth,
                          hipStream_t st);

}  // namespace rs
