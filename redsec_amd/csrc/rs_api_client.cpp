// rs_api_client.cpp -- key material and client-side calls of the C ABI (include/redsec_hip.h) that need no lane, no launch plan
// and no loaded key: seeded ciphertexts, the two public-key encryptions, RLWE extract, pack, re-keying (LWE and ring), encrypted
// selection, the selector keyswitch (and rs_circuit_bootstrap_dev, the one call here that needs a loaded key: it composes public
// calls around that keyswitch) and the packing key, device decryption and the three audits. Also the home of the ONE path a secret key takes onto the device and back off it
// (rs::with_secret_copy; rs_keygen_dev of rs_api_keys.cpp goes through it too) and of the refusals these calls share.
#include "rs_api_internal.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <initializer_list>

#include "rs_keygen.h"
#include "rs_pack.h"
#include "rs_packkey.h"
#include "rs_rekey.h"
#include "rs_ring_cmux.h"
#include "rs_ring_lookup.h"
#include "rs_ring_rekey.h"
#include "rs_ring_rotate.h"
#include "rs_ring_selector.h"
#include "rs_rlwe.h"

using rs::fail;
using rs::use_device;

namespace {

// a 0/1 key appended to `out`, `per_word` to a word from a fresh word on; the index of the first word outside {0, 1}, or -1
int pack_key_bits(const int32_t* key, int count, int per_word, std::vector<uint32_t>& out) {
  const size_t base = out.size();
  out.resize(base + ((size_t)count + per_word - 1) / per_word, 0u);
  for (int i = 0; i < count; ++i) {
    if (key[i] != 0 && key[i] != 1) return i;
    out[base + (size_t)(i / per_word)] |= (uint32_t)key[i] << (i % per_word);
  }
  return -1;
}

// `rc` behind the host copy of a secret that is not needed any more
int wiped(std::vector<uint32_t>& words, int rc) {
  std::fill(words.begin(), words.end(), 0u);
  return rc;
}

// the host copy of seed words does not outlive the call
void wipe_seed(uint32_t (&seed)[8]) {
  for (uint32_t& w : seed) *const_cast<volatile uint32_t*>(&w) = 0u;
}

int refuse_deviation(double stdev) {
  if (!rs::deviation_ok(stdev)) return fail(RS_ERR_INVALID, "noise deviation must be finite and non-negative (%g)", stdev);
  return RS_OK;
}

// `count` consecutive indices from `first` on stay below 2^64 (`what`: B ciphertexts, R ring ciphertexts)
int refuse_overflow(uint64_t first, size_t count, char what) {
  if (count > 0 && count - 1 > UINT64_MAX - first)
    return fail(RS_ERR_INVALID, "first + %c = %llu + %zu passes 2^64", what, (unsigned long long)first, count);
  return RS_OK;
}

// the digits of a packing key: t of them (`digits`: of basebit bits each, inside one 32-bit word)
int refuse_digits(int32_t basebit, int32_t t, bool digits) {
  if (digits && (basebit < 1 || basebit > 8)) return fail(RS_ERR_INVALID, "basebit = %d is outside 1 .. 8", (int)basebit);
  if (t < 1) return fail(RS_ERR_INVALID, "t = %d is below 1", (int)t);
  if (digits && (int64_t)t * basebit > 32) return fail(RS_ERR_INVALID, "t basebit = %d x %d passes 32 bits", (int)t, (int)basebit);
  return RS_OK;
}

// `written` (the out of a call, or its scratch) shares no byte with any of `others`: the kernels add into what they write with
// atomics after an init kernel has set it, so an overlap would give words that depend on scheduling. Inputs may overlap each other.
int refuse_overlap(const rs::Extent& written, std::initializer_list<rs::Extent> others) {
  const int i = rs::first_overlap(written, others.begin(), (int)others.size());
  if (i >= 0) return fail(RS_ERR_INVALID, "%s overlaps %s", written.name, others.begin()[i].name);
  return RS_OK;
}
// The same refusal, with the same text, for a call that lists its ranges once: the first `n_written` of `ranges` are written (out,
// then scratch), and each of them shares no byte with any range behind it.
int refuse_written(std::initializer_list<rs::Extent> ranges, int n_written) {
  for (int w = 0; w < n_written; ++w) {
    const rs::Extent* x = ranges.begin() + w;
    const int i = rs::first_overlap(*x, x + 1, (int)ranges.size() - w - 1);
    if (i >= 0) return fail(RS_ERR_INVALID, "%s overlaps %s", x->name, x[1 + i].name);
  }
  return RS_OK;
}
constexpr size_t kWord = sizeof(int32_t);

}  // namespace

namespace rs {

int refuse_equal_seeds(const uint8_t* mask_seed, const uint8_t* noise_seed) {
  if (memcmp(mask_seed, noise_seed, 32) == 0)
    return fail(RS_ERR_INVALID, "mask seed and noise seed are equal: the public mask seed would reveal the noise");
  return RS_OK;
}

int pack_key_pair(const rs_params& p, const int32_t* lwe_key, const int32_t* tlwe_key, int per_word, std::vector<uint32_t>& out,
                  size_t* lwe_words) {
  int bad = pack_key_bits(lwe_key, p.n, per_word, out);
  if (bad >= 0) return wiped(out, fail(RS_ERR_INVALID, "lwe_key[%d] = %d is not 0 or 1", bad, lwe_key[bad]));
  *lwe_words = out.size();
  bad = pack_key_bits(tlwe_key, p.N, per_word, out);
  if (bad >= 0) return wiped(out, fail(RS_ERR_INVALID, "tlwe_key[%d] = %d is not 0 or 1", bad, tlwe_key[bad]));
  return RS_OK;
}

int with_secret_copy(std::vector<uint32_t>& words, size_t extra, const std::function<int(const uint32_t*, char*)>& run) {
  const size_t key_bytes = (words.size() * sizeof(uint32_t) + 15) & ~(size_t)15, bytes = key_bytes + extra;
  char* d = nullptr;
  auto body = [&]() -> int {
    RS_HIP(hipMalloc(&d, bytes));
    RS_HIP(hipMemset(d, 0, bytes));
    RS_HIP(hipMemcpy(d, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return run(reinterpret_cast<const uint32_t*>(d), d + key_bytes);
  };
  const int rc = body();
  std::fill(words.begin(), words.end(), 0u);
  if (!d) return rc;
  (void)hipDeviceSynchronize();
  const hipError_t ez = hipMemset(d, 0, bytes);
  const hipError_t es = hipDeviceSynchronize();
  (void)hipFree(d);
  if (rc != RS_OK) return rc;
  if (ez != hipSuccess || es != hipSuccess) return fail(RS_ERR_HIP, "clearing the device copy of the secret key failed");
  return RS_OK;
}

}  // namespace rs

using rs::pack_key_pair;
using rs::with_secret_copy;

// seeded LWE ciphertexts (include/redsec_hip.h): the checks both directions share
static int seeded_args(const rs_ctx* c, rs::SeededArgs* a, const uint8_t* mask_seed, uint64_t first, size_t B) {
  const int rc = refuse_overflow(first, B, 'B');
  if (rc) return rc;
  if (B > (size_t)LONG_MAX) return fail(RS_ERR_INVALID, "B = %zu is too large", B);
  rs::kg_seed_words(mask_seed, a->seed);
  a->first = first; a->B = (long)B;
  a->n = c->p.n; a->tile = rs::kg_ct_tile(c->p.n);
  return RS_OK;
}

extern "C" {

int rs_encrypt_seeded_dev(rs_ctx* c, int32_t* body, int32_t* ct, const int32_t* mu, size_t B, const int32_t* lwe_key,
                          const uint8_t* mask_seed, const uint8_t* noise_seed, uint64_t first, double stdev) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!body || !mu || !lwe_key || !mask_seed || !noise_seed) return fail(RS_ERR_INVALID, "null pointer");
  if ((rc = rs::refuse_equal_seeds(mask_seed, noise_seed)) != RS_OK) return rc;
  if ((rc = refuse_deviation(stdev)) != RS_OK) return rc;
  // the key, one bit per word, zero past n
  std::vector<uint32_t> bits;
  const int bad = pack_key_bits(lwe_key, c->p.n, 32, bits);
  if (bad >= 0) return wiped(bits, fail(RS_ERR_INVALID, "lwe_key[%d] = %d is not 0 or 1", bad, lwe_key[bad]));
  rs::SeededArgs a{};
  rc = seeded_args(c, &a, mask_seed, first, B);
  if (rc || B == 0) return wiped(bits, rc);
  return with_secret_copy(bits, 0, [&](const uint32_t* d_bits, char*) -> int {
    a.ct = ct; a.body = body; a.mu = mu; a.key_bits = d_bits;
    rs::kg_seed_words(noise_seed, a.noise_seed);
    a.sigma = stdev;
    RS_HIP(rs::launch_encrypt_seeded(a, c->num_cus, nullptr));
    RS_HIP(hipDeviceSynchronize());
    return RS_OK;
  });
}

int rs_expand_ciphertexts_dev(rs_ctx* c, int32_t* ct, const uint8_t* mask_seed, uint64_t first, const int32_t* body, size_t B,
                              void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!ct || !mask_seed || !body) return fail(RS_ERR_INVALID, "null pointer");
  rs::SeededArgs a{};
  rc = seeded_args(c, &a, mask_seed, first, B);
  if (rc) return rc;
  if (B == 0) return RS_OK;
  a.ct = ct; a.body = const_cast<int32_t*>(body);
  RS_HIP(rs::launch_expand_ciphertexts(a, c->num_cus, (hipStream_t)stream));
  return RS_OK;
}

// public-key encryption (include/redsec_hip.h; kernel of rs_pubkey.hip): needs no key, the rand seed travels as a kernel argument
int rs_pk_encrypt_dev(rs_ctx* c, int32_t* ct, const int32_t* pk, size_t m, const int32_t* mu, const int32_t* base, size_t B,
                      const uint8_t* rand_seed, uint64_t first, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!ct || !pk || !rand_seed) return fail(RS_ERR_INVALID, "null pointer");
  if (m < 1 || m > (size_t)INT32_MAX) return fail(RS_ERR_INVALID, "m = %zu is outside 1 .. 2^31 - 1", m);
  if ((rc = refuse_overflow(first, B, 'B')) != RS_OK) return rc;
  const size_t row_bytes = ((size_t)c->p.n + 1) * sizeof(int32_t);
  if (B > (size_t)LONG_MAX / row_bytes || m > (size_t)LONG_MAX / row_bytes || (B + rs::kPkTile - 1) / rs::kPkTile > (size_t)INT32_MAX)
    return fail(RS_ERR_INVALID, "B = %zu or m = %zu is too large for rows of %zu bytes", B, m, row_bytes);
  if (B == 0) return RS_OK;
  rs::PkArgs a{};
  a.ct = ct; a.pk = pk; a.mu = mu; a.base = base;
  rs::kg_seed_words(rand_seed, a.seed);
  a.first = first; a.B = (long)B; a.m = (long)m; a.n = c->p.n;
  const hipError_t e = rs::launch_pk_encrypt(a, (hipStream_t)stream);
  wipe_seed(a.seed);
  if (e != hipSuccess) return fail(RS_ERR_HIP, "launch_pk_encrypt failed: %s", hipGetErrorString(e));
  return RS_OK;
}

// compact RLWE public keys (include/redsec_hip.h; kernels of rs_rlwe.hip): neither call needs a key, the ring is the context's
int rs_rlwe_pk_encrypt_dev(rs_ctx* c, int32_t* rlwe, const int32_t* pk, const int32_t* mu, size_t count, const uint8_t* rand_seed,
                           uint64_t first, double stdev, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!rlwe || !pk || !mu || !rand_seed) return fail(RS_ERR_INVALID, "null pointer");
  if ((rc = refuse_deviation(stdev)) != RS_OK) return rc;
  const size_t N = (size_t)c->p.N;
  if (N < (size_t)rs::kRlMinN || N > (size_t)rs::kRlMaxN) return fail(RS_ERR_INVALID, "unsupported ring N = %zu", N);
  const size_t R = count / N + (count % N ? 1 : 0), tiles = N / rs::kRlTile;
  if ((rc = refuse_overflow(first, R, 'R')) != RS_OK) return rc;
  if (count > (size_t)LONG_MAX / (2 * sizeof(int32_t)) - N || R > (size_t)INT32_MAX / (2 * tiles))
    return fail(RS_ERR_INVALID, "count = %zu is too large for ciphertexts of 2 x %zu words", count, N);
  if (count == 0) return RS_OK;
  rs::RlweEncArgs a{};
  a.rlwe = rlwe; a.pk = pk; a.mu = mu;
  rs::kg_seed_words(rand_seed, a.seed);
  a.first = first; a.count = (long)count; a.N = (int)N; a.sigma = stdev;
  const hipError_t e = rs::launch_rlwe_pk_encrypt(a, (hipStream_t)stream);
  wipe_seed(a.seed);
  if (e != hipSuccess) return fail(RS_ERR_HIP, "launch_rlwe_pk_encrypt failed: %s", hipGetErrorString(e));
  return RS_OK;
}

int rs_rlwe_extract_dev(rs_ctx* c, int32_t* u, const int32_t* rlwe, size_t count, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!u || !rlwe) return fail(RS_ERR_INVALID, "null pointer");
  const size_t row_bytes = ((size_t)c->p.N + 1) * sizeof(int32_t);
  if (count > (size_t)LONG_MAX / row_bytes || count > (size_t)INT32_MAX)
    return fail(RS_ERR_INVALID, "count = %zu is too large for rows of %zu bytes", count, row_bytes);
  if (count == 0) return RS_OK;
  const rs::RlweExtractArgs x{u, rlwe, (long)count, c->p.N};
  RS_HIP(rs::launch_rlwe_extract(x, (hipStream_t)stream));
  return RS_OK;
}

// packed results (include/redsec_hip.h; kernels of rs_pack.hip, integer arithmetic only): needs no key, the ring and n are the context's
int rs_pack_dev(rs_ctx* c, int32_t* rlwe, const int32_t* ct, size_t count, const int32_t* pack_key, int32_t basebit, int32_t t,
                void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!rlwe || !ct || !pack_key) return fail(RS_ERR_INVALID, "null pointer");
  if ((rc = refuse_digits(basebit, t, true)) != RS_OK) return rc;
  const size_t N = (size_t)c->p.N, n = (size_t)c->p.n;
  if (N < (size_t)rs::kPaMinN || N > (size_t)rs::kPaMaxN) return fail(RS_ERR_INVALID, "unsupported ring N = %zu", N);
  const size_t row_bytes = (n + 1) * sizeof(int32_t), R = count / N + (count % N ? 1 : 0);
  if (count > (size_t)LONG_MAX / row_bytes || count > (size_t)LONG_MAX / (2 * sizeof(int32_t)) - N)
    return fail(RS_ERR_INVALID, "count = %zu is too large for rows of %zu bytes", count, row_bytes);
  if (count == 0) return RS_OK;
  const size_t per_r = 2 * (N / rs::kPaTile) * (size_t)rs::pa_slot_blocks((long)count, (int)N) * (size_t)rs::pa_chunks((int)n);
  if (R > (size_t)INT32_MAX / per_r)                                        // workgroups of one launch (rs::pa_groups)
    return fail(RS_ERR_INVALID, "count = %zu is too large for one launch", count);
  if ((rc = refuse_overlap({"rlwe", rlwe, R * 2 * N * kWord}, {{"ct", ct, count * row_bytes}, {"pack_key", pack_key, n * (size_t)t * 2 * N * kWord}})) != RS_OK)
    return rc;
  const rs::PackArgs a{rlwe, ct, pack_key, (long)count, (int)n, (int)N, (int)basebit, (int)t};
  RS_HIP(rs::launch_pack(a, (hipStream_t)stream));
  return RS_OK;
}

// re-keying (include/redsec_hip.h; kernels of rs_rekey.hip, integer arithmetic only): needs no key, both dimensions are arguments
int rs_rekey_dev(rs_ctx* c, int32_t* out, const int32_t* ct, size_t B, int32_t n_src, const int32_t* rekey_key, int32_t n_dst,
                 int32_t basebit, int32_t t, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!out || !ct || !rekey_key) return fail(RS_ERR_INVALID, "null pointer");
  if (n_src < rs::kRkMinDim || n_src > rs::kRkMaxDim) return fail(RS_ERR_INVALID, "n_src = %d is outside 1 .. %d", (int)n_src, rs::kRkMaxDim);
  if (n_dst < rs::kRkMinDim || n_dst > rs::kRkMaxDim) return fail(RS_ERR_INVALID, "n_dst = %d is outside 1 .. %d", (int)n_dst, rs::kRkMaxDim);
  if ((rc = refuse_digits(basebit, t, true)) != RS_OK) return rc;
  const size_t row_bytes = ((size_t)std::max(n_src, n_dst) + 1) * sizeof(int32_t);
  if (B > (size_t)LONG_MAX / row_bytes) return fail(RS_ERR_INVALID, "B = %zu is too large for rows of %zu bytes", B, row_bytes);
  if (B == 0) return RS_OK;
  // workgroups of the two launches: one per kRkInitThreads output words, and rs::rk_groups
  const size_t init_groups = (B * ((size_t)n_dst + 1) + rs::kRkInitThreads - 1) / rs::kRkInitThreads;
  const size_t per_tile = (size_t)rs::rk_word_tiles(n_dst) * (size_t)rs::rk_splits((long)B, n_src, n_dst);
  if (init_groups > (size_t)INT32_MAX || (size_t)rs::rk_ct_tiles((long)B) > (size_t)INT32_MAX / per_tile)
    return fail(RS_ERR_INVALID, "B = %zu is too large for one launch", B);
  const size_t dst_words = (size_t)n_dst + 1;
  if ((rc = refuse_overlap({"out", out, B * dst_words * kWord}, {{"ct", ct, B * ((size_t)n_src + 1) * kWord},
                                                                  {"rekey_key", rekey_key, (size_t)n_src * (size_t)t * dst_words * kWord}})) != RS_OK)
    return rc;
  const rs::RekeyArgs a{out, ct, rekey_key, (long)B, (int)n_src, (int)n_dst, (int)basebit, (int)t};
  RS_HIP(rs::launch_rekey(a, (hipStream_t)stream));
  return RS_OK;
}

// ring re-keying (include/redsec_hip.h; kernels of rs_ring_rekey.hip, integer arithmetic only): needs no key, the ring is the context's
int rs_ring_rekey_dev(rs_ctx* c, int32_t* out, const int32_t* rlwe, size_t R, const int32_t* ring_key, int32_t basebit, int32_t t,
                      void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!out || !rlwe || !ring_key) return fail(RS_ERR_INVALID, "null pointer");
  if ((rc = refuse_digits(basebit, t, true)) != RS_OK) return rc;
  if ((int64_t)t * basebit > rs::kRrMaxBits)
    return fail(RS_ERR_INVALID, "t basebit = %d x %d passes %d bits", (int)t, (int)basebit, rs::kRrMaxBits);
  const size_t N = (size_t)c->p.N;
  if (N < (size_t)rs::kRrMinN || N > (size_t)rs::kRrMaxN || (N & (N - 1))) return fail(RS_ERR_INVALID, "unsupported ring N = %zu", N);
  if (R > (size_t)LONG_MAX / (2 * N * sizeof(int32_t))) return fail(RS_ERR_INVALID, "R = %zu is too large for ciphertexts of %zu bytes", R, 2 * N * sizeof(int32_t));
  if (R == 0) return RS_OK;
  // workgroups of the two launches: one per kRrInitThreads output words, and rs::rr_groups
  const size_t init_per_r = 2 * N / rs::kRrInitThreads, per_r = (size_t)rs::rr_groups_per_ct((int)N, (int)t);
  if (R > (size_t)INT32_MAX / init_per_r || R > (size_t)INT32_MAX / per_r) return fail(RS_ERR_INVALID, "R = %zu is too large for one launch", R);
  if ((rc = refuse_overlap({"out", out, R * 2 * N * kWord}, {{"rlwe", rlwe, R * 2 * N * kWord},
                                                            {"ring_key", ring_key, ((size_t)t + 1) * 2 * N * kWord}})) != RS_OK)
    return rc;
  const rs::RingRekeyArgs a{out, rlwe, ring_key, (long)R, (int)N, (int)basebit, (int)t};
  RS_HIP(rs::launch_ring_rekey(a, (hipStream_t)stream));
  return RS_OK;
}

// encrypted selection (include/redsec_hip.h; kernels of rs_ring_cmux.hip, integer arithmetic only): needs no key, the ring is the
// context's. The checks of digit shape and ring that the two calls share.
static int ring_cmux_shape(const rs_ctx* c, int32_t basebit, int32_t l, size_t* N_) {
  if (basebit < 1 || basebit > 8) return fail(RS_ERR_INVALID, "basebit = %d is outside 1 .. 8", (int)basebit);
  if (l < 1) return fail(RS_ERR_INVALID, "l = %d is below 1", (int)l);
  if ((int64_t)l * basebit > rs::kRcMaxBits)
    return fail(RS_ERR_INVALID, "l basebit = %d x %d passes %d bits", (int)l, (int)basebit, rs::kRcMaxBits);
  const size_t N = (size_t)c->p.N;
  if (N < (size_t)rs::kRcMinN || N > (size_t)rs::kRcMaxN || (N & (N - 1))) return fail(RS_ERR_INVALID, "unsupported ring N = %zu", N);
  *N_ = N;
  return RS_OK;
}
// R rows read at `stride`: the row arithmetic and the workgroups of the two launches (one per kRcInitThreads output words, and
// rs::rc_groups)
static int ring_cmux_rows(size_t R, size_t stride, size_t N, int32_t l) {
  const size_t ct_bytes = 2 * N * sizeof(int32_t);
  if (R > (size_t)LONG_MAX / ct_bytes || (R && stride > (size_t)LONG_MAX / ct_bytes / R))
    return fail(RS_ERR_INVALID, "R = %zu at stride %zu is too large for ciphertexts of %zu bytes", R, stride, ct_bytes);
  const size_t init_per_r = 2 * N / rs::kRcInitThreads, per_r = (size_t)rs::rc_groups_per_ct((int)N, (int)l);
  if (R > (size_t)INT32_MAX / init_per_r || R > (size_t)INT32_MAX / per_r) return fail(RS_ERR_INVALID, "R = %zu is too large for one launch", R);
  return RS_OK;
}

// one CMUX of either digit form (rs::kRcSigned, rs::kRcAlternating): the checks, the refusals and the launch are the same
static int ring_cmux_any(rs_ctx* c, int32_t* out, const int32_t* d1, const int32_t* d0, size_t R, size_t stride, const int32_t* sel,
                         int32_t basebit, int32_t l, int form, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!out || !d0 || !sel) return fail(RS_ERR_INVALID, "null pointer");
  size_t N = 0;
  if ((rc = ring_cmux_shape(c, basebit, l, &N)) != RS_OK) return rc;
  if (stride == 0) return fail(RS_ERR_INVALID, "stride = 0");
  if ((rc = ring_cmux_rows(R, stride, N, l)) != RS_OK) return rc;
  if (R == 0) return RS_OK;
  const size_t ct_bytes = 2 * N * kWord, read_bytes = ((R - 1) * stride + 1) * ct_bytes;     // rows 0, stride, .. (R - 1) stride
  if ((rc = refuse_overlap({"out", out, R * ct_bytes}, {{"d0", d0, read_bytes}, {"d1", d1, read_bytes}, {"sel", sel, (size_t)2 * l * ct_bytes}})) != RS_OK)
    return rc;
  const rs::RingCmuxArgs a{out, d1, d0, sel, (long)R, (long)stride, (int)N, (int)basebit, (int)l, form};
  RS_HIP(rs::launch_ring_cmux(a, (hipStream_t)stream));
  return RS_OK;
}
int rs_ring_cmux_dev(rs_ctx* c, int32_t* out, const int32_t* d1, const int32_t* d0, size_t R, size_t stride, const int32_t* sel,
                     int32_t basebit, int32_t l, void* stream) {
  return ring_cmux_any(c, out, d1, d0, R, stride, sel, basebit, l, rs::kRcSigned, stream);
}
int rs_ring_cmux_alt_dev(rs_ctx* c, int32_t* out, const int32_t* d1, const int32_t* d0, size_t R, size_t stride, const int32_t* sel,
                         int32_t basebit, int32_t l, void* stream) {
  return ring_cmux_any(c, out, d1, d0, R, stride, sel, basebit, l, rs::kRcAlternating, stream);
}

// the CMUX tree: level k pairs rows (2r, 2r + 1) of the previous level under selector k; an unpaired last row meets the all-zero
// ciphertext. The levels alternate between the two halves of scratch, ceil(E / 2) and ceil(E / 4) rows; the last one writes out.
// Either digit form: every level's launches carry `form`.
static int ring_lookup_any(rs_ctx* c, int32_t* out, const int32_t* table, size_t entries, const int32_t* sel, int32_t depth,
                           int32_t basebit, int32_t l, int32_t* scratch, int form, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!out || !table || !sel) return fail(RS_ERR_INVALID, "null pointer");
  size_t N = 0;
  if ((rc = ring_cmux_shape(c, basebit, l, &N)) != RS_OK) return rc;
  if (depth < 1 || depth > rs::kRcMaxDepth) return fail(RS_ERR_INVALID, "depth = %d is outside 1 .. %d", (int)depth, rs::kRcMaxDepth);
  if (entries < 1 || entries > ((size_t)1 << depth))
    return fail(RS_ERR_INVALID, "entries = %zu is outside 1 .. 2^%d", entries, (int)depth);
  if (depth > 1 && !scratch) return fail(RS_ERR_INVALID, "null scratch with depth = %d", (int)depth);
  if ((rc = ring_cmux_rows(entries / 2 + 1, 2, N, l)) != RS_OK) return rc;     // level 0, the largest launch: entries / 2 pairs at stride 2
  const size_t ct = 2 * N, sel_words = (size_t)2 * l * ct;
  const rs::Extent x_table{"table", table, entries * ct * kWord}, x_sel{"sel", sel, (size_t)depth * sel_words * kWord};
  const rs::Extent x_scratch{"scratch", depth > 1 ? scratch : nullptr, (size_t)rs::rc_scratch_rows((long)entries) * ct * kWord};
  if ((rc = refuse_overlap({"out", out, ct * kWord}, {x_table, x_sel, x_scratch})) != RS_OK) return rc;
  if ((rc = refuse_overlap(x_scratch, {x_table, x_sel})) != RS_OK) return rc;
  int32_t* half[2] = {scratch, scratch ? scratch + (size_t)rs::rc_level_rows((long)entries) * ct : nullptr};
  const int32_t* in = table;
  size_t rows = entries;
  for (int k = 0; k < depth; ++k) {
    int32_t* o = k == depth - 1 ? out : half[k & 1];
    const size_t pairs = rows / 2;
    const int32_t* s = sel + (size_t)k * sel_words;
    if (pairs) {
      const rs::RingCmuxArgs a{o, in + ct, in, s, (long)pairs, 2, (int)N, (int)basebit, (int)l, form};
      RS_HIP(rs::launch_ring_cmux(a, (hipStream_t)stream));
    }
    if (rows & 1) {
      const rs::RingCmuxArgs a{o + pairs * ct, nullptr, in + (rows - 1) * ct, s, 1, 1, (int)N, (int)basebit, (int)l, form};
      RS_HIP(rs::launch_ring_cmux(a, (hipStream_t)stream));
    }
    in = o;
    rows = (size_t)rs::rc_level_rows((long)rows);
  }
  return RS_OK;
}
int rs_ring_lookup_dev(rs_ctx* c, int32_t* out, const int32_t* table, size_t entries, const int32_t* sel, int32_t depth,
                       int32_t basebit, int32_t l, int32_t* scratch, void* stream) {
  return ring_lookup_any(c, out, table, entries, sel, depth, basebit, l, scratch, rs::kRcSigned, stream);
}
int rs_ring_lookup_alt_dev(rs_ctx* c, int32_t* out, const int32_t* table, size_t entries, const int32_t* sel, int32_t depth,
                           int32_t basebit, int32_t l, int32_t* scratch, void* stream) {
  return ring_lookup_any(c, out, table, entries, sel, depth, basebit, l, scratch, rs::kRcAlternating, stream);
}

// R of those trees side by side (include/redsec_hip.h; kernels of rs_ring_lookup.hip): one init and one sweep launch per level for
// all rows, the unpaired last row of every table inside the same launch. Level 0 reads the tables at the caller's strides; level k
// writes [R][P_k] ciphertexts into half k & 1 of scratch, which the next level reads with row stride P_k and entry stride 1; the
// last level writes out. Either digit form: every level carries `form`.
static int ring_lookup_rows_any(rs_ctx* c, int32_t* out, const int32_t* table, size_t entries, size_t row_stride, size_t entry_stride,
                                size_t R, const int32_t* sel, int32_t depth, int32_t per_row, int32_t basebit, int32_t l,
                                int32_t* scratch, int form, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!out || !table || !sel) return fail(RS_ERR_INVALID, "null pointer");
  size_t N = 0;
  if ((rc = ring_cmux_shape(c, basebit, l, &N)) != RS_OK) return rc;
  if (depth < 1 || depth > rs::kLkMaxDepth) return fail(RS_ERR_INVALID, "depth = %d is outside 1 .. %d", (int)depth, rs::kLkMaxDepth);
  if (entries < 1 || entries > ((size_t)1 << depth))
    return fail(RS_ERR_INVALID, "entries = %zu is outside 1 .. 2^%d", entries, (int)depth);
  if (entry_stride == 0) return fail(RS_ERR_INVALID, "entry_stride = 0");
  if (depth > 1 && !scratch) return fail(RS_ERR_INVALID, "null scratch with depth = %d", (int)depth);
  // the extents in bytes, each below LONG_MAX; `over` collects an overflow of the row arithmetic itself
  const size_t ct = 2 * N, ct_bytes = ct * kWord, set_words = (size_t)depth * rs::lk_sel_words((int)N, (int)l);
  bool over = false;
  auto mul = [&over](size_t a, size_t b) { size_t r; over |= __builtin_mul_overflow(a, b, &r); return r; };
  auto add = [&over](size_t a, size_t b) { size_t r; over |= __builtin_add_overflow(a, b, &r); return r; };
  const size_t read_bytes = mul(add(add(mul(R ? R - 1 : 0, row_stride), mul(entries - 1, entry_stride)), 1), ct_bytes);
  if (over || read_bytes > (size_t)LONG_MAX)
    return fail(RS_ERR_INVALID, "R = %zu at row_stride %zu with %zu entries at entry_stride %zu is too large for ciphertexts of %zu bytes",
                R, row_stride, entries, entry_stride, ct_bytes);
  const size_t sel_bytes = mul(per_row ? R : 1, set_words * kWord);
  if (over || sel_bytes > (size_t)LONG_MAX)
    return fail(RS_ERR_INVALID, "R = %zu is too large for selector sets of %zu bytes", R, set_words * kWord);
  const size_t scratch_rows = (size_t)rs::rc_scratch_rows((long)entries), scratch_bytes = mul(mul(R, scratch_rows), ct_bytes);
  if (over || scratch_bytes > (size_t)LONG_MAX)
    return fail(RS_ERR_INVALID, "R = %zu is too large for a scratch of %zu ciphertexts of %zu bytes per row", R, scratch_rows, ct_bytes);
  // level 0, the largest launch: R ceil(entries / 2) output ciphertexts
  const size_t P0 = (size_t)rs::lk_level_rows((long)entries);
  const size_t per_out = std::max((size_t)rs::rc_groups_per_ct((int)N, (int)l), 2 * N / rs::kLkInitThreads);
  if (mul(mul(R, P0), per_out) > (size_t)INT32_MAX || over)
    return fail(RS_ERR_INVALID, "R = %zu with %zu pairs per row is too large for one launch", R, P0);
  if (R == 0) return RS_OK;
  const rs::Extent x_table{"table", table, read_bytes}, x_sel{"sel", sel, sel_bytes};
  const rs::Extent x_scratch{"scratch", depth > 1 ? scratch : nullptr, scratch_bytes};
  if ((rc = refuse_written({{"out", out, R * ct_bytes}, x_scratch, x_table, x_sel}, 2)) != RS_OK) return rc;
  int32_t* half[2] = {scratch, scratch ? scratch + (size_t)rs::lk_scratch_half((long)R, (long)entries, 1) * ct : nullptr};
  const int32_t* in = table;
  size_t rows = entries;
  for (int k = 0; k < depth; ++k) {
    int32_t* o = k == depth - 1 ? out : half[k & 1];
    const rs::RingLookupArgs a{o, in, sel, (long)R, (long)rows, row_stride, entry_stride, per_row ? set_words : 0, k,
                               (int)N, (int)basebit, (int)l, form};
    RS_HIP(rs::launch_ring_lookup_level(a, (hipStream_t)stream));
    in = o;
    rows = (size_t)rs::lk_level_rows((long)rows);
    row_stride = rows;                                           // the level wrote [R][rows] ciphertexts
    entry_stride = 1;
  }
  return RS_OK;
}
int rs_ring_lookup_rows_dev(rs_ctx* c, int32_t* out, const int32_t* table, size_t entries, size_t row_stride, size_t entry_stride,
                            size_t R, const int32_t* sel, int32_t depth, int32_t per_row, int32_t basebit, int32_t l,
                            int32_t* scratch, void* stream) {
  return ring_lookup_rows_any(c, out, table, entries, row_stride, entry_stride, R, sel, depth, per_row, basebit, l, scratch,
                              rs::kRcSigned, stream);
}
int rs_ring_lookup_rows_alt_dev(rs_ctx* c, int32_t* out, const int32_t* table, size_t entries, size_t row_stride, size_t entry_stride,
                                size_t R, const int32_t* sel, int32_t depth, int32_t per_row, int32_t basebit, int32_t l,
                                int32_t* scratch, void* stream) {
  return ring_lookup_rows_any(c, out, table, entries, row_stride, entry_stride, R, sel, depth, per_row, basebit, l, scratch,
                              rs::kRcAlternating, stream);
}

// encrypted rotation (include/redsec_hip.h; kernels of rs_ring_rotate.hip): a chain of `depth` CMUXes between acc and X^(e_k) acc,
// e_k = (step 2^k) mod 2N. The levels alternate between scratch and out so that the last one writes out; level 0 reads `in` at
// `stride`, the later ones the previous level's rows. Either digit form: every level carries `form`.
static int ring_rotate_any(rs_ctx* c, int32_t* out, const int32_t* in, size_t R, size_t stride, const int32_t* sel, int32_t depth,
                           int32_t per_row, int32_t step, int32_t basebit, int32_t l, int32_t* scratch, int form, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!out || !in || !sel) return fail(RS_ERR_INVALID, "null pointer");
  size_t N = 0;
  if ((rc = ring_cmux_shape(c, basebit, l, &N)) != RS_OK) return rc;
  if (depth < 1 || depth > rs::kRoMaxDepth) return fail(RS_ERR_INVALID, "depth = %d is outside 1 .. %d", (int)depth, rs::kRoMaxDepth);
  if (depth > 1 && !scratch) return fail(RS_ERR_INVALID, "null scratch with depth = %d", (int)depth);
  if ((rc = ring_cmux_rows(R, stride, N, l)) != RS_OK) return rc;
  const size_t ct = 2 * N, sel_words = rs::ro_sel_words((int)N, (int)l), set_words = (size_t)depth * sel_words;
  if (per_row && R > (size_t)LONG_MAX / kWord / set_words)
    return fail(RS_ERR_INVALID, "R = %zu is too large for selector sets of %zu bytes", R, set_words * kWord);
  if (R == 0) return RS_OK;
  const rs::Extent x_in{"in", in, ((R - 1) * stride + 1) * ct * kWord}, x_sel{"sel", sel, (per_row ? R : 1) * set_words * kWord};
  const rs::Extent x_scratch{"scratch", depth > 1 ? scratch : nullptr, R * ct * kWord};
  if ((rc = refuse_written({{"out", out, R * ct * kWord}, x_scratch, x_in, x_sel}, 2)) != RS_OK) return rc;
  const int32_t* src = in;
  for (int k = 0; k < depth; ++k) {
    int32_t* o = ((depth - 1 - k) & 1) ? scratch : out;          // the last level writes out
    const rs::RingRotateArgs a{o, src, sel + (size_t)k * sel_words, (long)R, (long)(k ? 1 : stride), per_row ? set_words : 0,
                               (int)N, (int)basebit, (int)l, rs::ro_exponent(step, k, (int)N), form};
    RS_HIP(rs::launch_ring_rotate_level(a, (hipStream_t)stream));
    src = o;
  }
  return RS_OK;
}
int rs_ring_rotate_dev(rs_ctx* c, int32_t* out, const int32_t* in, size_t R, size_t stride, const int32_t* sel, int32_t depth,
                       int32_t per_row, int32_t step, int32_t basebit, int32_t l, int32_t* scratch, void* stream) {
  return ring_rotate_any(c, out, in, R, stride, sel, depth, per_row, step, basebit, l, scratch, rs::kRcSigned, stream);
}
int rs_ring_rotate_alt_dev(rs_ctx* c, int32_t* out, const int32_t* in, size_t R, size_t stride, const int32_t* sel, int32_t depth,
                           int32_t per_row, int32_t step, int32_t basebit, int32_t l, int32_t* scratch, void* stream) {
  return ring_rotate_any(c, out, in, R, stride, sel, depth, per_row, step, basebit, l, scratch, rs::kRcAlternating, stream);
}

// the samples of coefficients 0 .. width - 1 of each of R ciphertexts (ring_heads_kernel): what rs_keyswitch_dev takes
int rs_ring_heads_dev(rs_ctx* c, int32_t* u, const int32_t* rlwe, size_t R, size_t width, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!u || !rlwe) return fail(RS_ERR_INVALID, "null pointer");
  const size_t N = (size_t)c->p.N;
  if (N < (size_t)rs::kRlMinN || N > (size_t)rs::kRlMaxN) return fail(RS_ERR_INVALID, "unsupported ring N = %zu", N);
  if (width < 1 || width > N) return fail(RS_ERR_INVALID, "width = %zu is outside 1 .. %zu", width, N);
  const size_t row_bytes = (N + 1) * sizeof(int32_t);
  if (R > (size_t)INT32_MAX / width || R * width > (size_t)LONG_MAX / row_bytes)
    return fail(RS_ERR_INVALID, "R = %zu at width %zu is too large for rows of %zu bytes", R, width, row_bytes);
  if (R == 0) return RS_OK;
  if ((rc = refuse_written({{"u", u, R * width * row_bytes}, {"rlwe", rlwe, R * 2 * N * kWord}}, 1)) != RS_OK) return rc;
  const rs::RingHeadsArgs x{u, rlwe, (long)R, (int)width, (int)N};
  RS_HIP(rs::launch_ring_heads(x, (hipStream_t)stream));
  return RS_OK;
}

// circuit bootstrapping (include/redsec_hip.h; kernels of rs_ring_selector.hip, integer arithmetic only). The checks the two calls
// share: digit shapes, ring, depth, source dimension, and the workgroups of the launches. The keyswitch itself needs no key.
static int selector_digits_shape(int32_t basebit, int32_t l, int32_t ks_basebit, int32_t ks_t) {
  if (basebit < 1 || basebit > 8) return fail(RS_ERR_INVALID, "basebit = %d is outside 1 .. 8", (int)basebit);
  if (l < 1) return fail(RS_ERR_INVALID, "l = %d is below 1", (int)l);
  if ((int64_t)l * basebit > rs::kSeMaxBits)
    return fail(RS_ERR_INVALID, "l basebit = %d x %d passes %d bits", (int)l, (int)basebit, rs::kSeMaxBits);
  if (ks_basebit < 1 || ks_basebit > 8) return fail(RS_ERR_INVALID, "ks_basebit = %d is outside 1 .. 8", (int)ks_basebit);
  if (ks_t < 1) return fail(RS_ERR_INVALID, "ks_t = %d is below 1", (int)ks_t);
  if ((int64_t)ks_t * ks_basebit > 32) return fail(RS_ERR_INVALID, "ks_t ks_basebit = %d x %d passes 32 bits", (int)ks_t, (int)ks_basebit);
  return RS_OK;
}
// the key's words and the grid of `form` (rs::kSeChunked: the init kernel's workgroups and rs::se_groups; rs::kSeWide: rs::sw_groups),
// each inside what a launch and a long can index; `what` names the caller's count in the refusal
static int selector_ring_shape(const rs_ctx* c, size_t rows, int form, const char* what, int32_t n_src, const int32_t* sel_key, int32_t ks_t,
                               size_t* N_) {
  if (n_src < 1 || n_src > rs::kSeMaxSrc) return fail(RS_ERR_INVALID, "n_src = %d is outside 1 .. %d", (int)n_src, rs::kSeMaxSrc);
  const size_t N = (size_t)c->p.N;
  if (N < (size_t)rs::kSeMinN || N > (size_t)rs::kSeMaxN || (N & (N - 1))) return fail(RS_ERR_INVALID, "unsupported ring N = %zu", N);
  if ((uintptr_t)sel_key & 15u) return fail(RS_ERR_INVALID, "sel_key must be 16-byte aligned");
  const size_t key_polys = 2 * ((size_t)n_src + 1) * (size_t)ks_t * 2;
  if (key_polys > (size_t)LONG_MAX / sizeof(int32_t) / N) return fail(RS_ERR_INVALID, "a key of %zu polynomials is too large", key_polys);
  const bool fits = rows > (size_t)INT32_MAX ? false
                    : form == rs::kSeWide   ? (size_t)rs::sw_row_blocks((long)rows) <= (size_t)INT32_MAX / (size_t)rs::sw_groups_per_block((int)N)
                                            : rows * 4 * N / rs::kSeInitThreads <= (size_t)INT32_MAX &&
                                                  (size_t)rs::se_row_blocks((long)rows) <= (size_t)INT32_MAX / (size_t)rs::se_groups_per_block((int)N, (int)n_src);
  if (!fits) return fail(RS_ERR_INVALID, "%s l = %zu rows are too many for one launch", what, rows);
  *N_ = N;
  return RS_OK;
}
static int ring_selector_shape(const rs_ctx* c, int32_t depth, int32_t basebit, int32_t l, int32_t n_src, const int32_t* sel_key,
                               int32_t ks_basebit, int32_t ks_t, size_t* N_) {
  const int rc = selector_digits_shape(basebit, l, ks_basebit, ks_t);
  if (rc) return rc;
  if (depth < 0 || depth > rs::kSeMaxDepth) return fail(RS_ERR_INVALID, "depth = %d is outside 0 .. %d", (int)depth, rs::kSeMaxDepth);
  return selector_ring_shape(c, (size_t)depth * (size_t)l, rs::kSeChunked, "depth", n_src, sel_key, ks_t, N_);
}
// the batch calls: any count whose rows one launch of the planned form can index; *plan = that form and its workgroups
static int ring_selector_batch_shape(const rs_ctx* c, size_t count, int32_t basebit, int32_t l, int32_t n_src, const int32_t* sel_key,
                                     int32_t ks_basebit, int32_t ks_t, size_t* N_, rs::SePlan* plan) {
  const int rc = selector_digits_shape(basebit, l, ks_basebit, ks_t);
  if (rc) return rc;
  const size_t rows = count > (size_t)INT32_MAX ? SIZE_MAX : count * (size_t)l;
  const long plan_rows = rows > (size_t)INT32_MAX ? (long)INT32_MAX : (long)rows;
  const int N = c->p.N;
  *plan = rs::selector_form(plan_rows, N >= rs::kSeMinN ? N : rs::kSeMinN, n_src, c->num_cus, c->sel_force);
  return selector_ring_shape(c, rows, plan->form, "count", n_src, sel_key, ks_t, N_);
}

// What both forms of a call share behind their shape checks. `batch` = the batch form: sel 16-byte aligned (the wide kernel's
// stores), the planned kernel; else the chunked kernel, whatever RS_SEL_FORM says.
static int ring_selector_run(rs_ctx* c, int32_t* sel, const int32_t* ct, size_t rows, size_t N, bool batch, rs::SePlan plan, int32_t basebit,
                             int32_t l, int32_t n_src, const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, void* stream) {
  const size_t src_words = (size_t)n_src + 1;
  const int rc = refuse_overlap({"sel", sel, rows * 4 * N * kWord}, {{"ct", ct, rows * src_words * kWord},
                                                                  {"sel_key", sel_key, 2 * src_words * (size_t)ks_t * 2 * N * kWord}});
  if (rc != RS_OK) return rc;
  if (batch && ((uintptr_t)sel & 15u)) return fail(RS_ERR_INVALID, "sel must be 16-byte aligned");
  const rs::RingSelectorArgs a{sel, ct, sel_key, (long)rows, (int)N, (int)n_src, (int)basebit, (int)l, (int)ks_basebit, (int)ks_t};
  if (!batch) plan = rs::SePlan{rs::kSeChunked, rs::se_groups(a.rows, a.N, a.n_src)};
  if (plan.form == rs::kSeWide) RS_HIP(rs::launch_ring_selector_wide(a, (hipStream_t)stream));
  else RS_HIP(rs::launch_ring_selector(a, (hipStream_t)stream));
  c->sel_form = plan.form; c->sel_groups = plan.groups;
  return RS_OK;
}

int rs_ring_selector_dev(rs_ctx* c, int32_t* sel, const int32_t* ct, int32_t depth, int32_t basebit, int32_t l, int32_t n_src,
                         const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!sel || !ct || !sel_key) return fail(RS_ERR_INVALID, "null pointer");
  size_t N = 0;
  if ((rc = ring_selector_shape(c, depth, basebit, l, n_src, sel_key, ks_basebit, ks_t, &N)) != RS_OK) return rc;
  if (depth == 0) return RS_OK;
  return ring_selector_run(c, sel, ct, (size_t)depth * (size_t)l, N, false, rs::SePlan{}, basebit, l, n_src, sel_key, ks_basebit, ks_t, stream);
}

// The batch form: `count` bits instead of depth <= 30, the same arithmetic, checks and refusals with the extents computed from
// count, and the kernel rs::selector_form plans for count l rows (rs_ring_selector.h; RS_SEL_FORM forces one).
int rs_ring_selector_batch_dev(rs_ctx* c, int32_t* sel, const int32_t* ct, size_t count, int32_t basebit, int32_t l, int32_t n_src,
                               const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!sel || !ct || !sel_key) return fail(RS_ERR_INVALID, "null pointer");
  size_t N = 0;
  rs::SePlan plan{};
  if ((rc = ring_selector_batch_shape(c, count, basebit, l, n_src, sel_key, ks_basebit, ks_t, &N, &plan)) != RS_OK) return rc;
  if (count == 0) return RS_OK;
  return ring_selector_run(c, sel, ct, count * (size_t)l, N, true, plan, basebit, l, n_src, sel_key, ks_basebit, ks_t, stream);
}

// LWE bit -> l bootstraps at the gadget's levels -> selector keyswitch. The steps are the public calls: the gather that replicates
// each bit l times, ONE programmable bootstrap over the count l rows whose test polynomial of level j is the constant h_j / 2, and
// rs_ring_selector_dev (batch: rs_ring_selector_batch_dev) from the context's n. scratch (rs_ring_selector.h se_scratch_*): test
// polynomials, row index, replicated bits, bootstraps.
static int circuit_bootstrap_run(rs_ctx* c, int32_t* sel, const int32_t* bits, size_t count, size_t N, bool batch, int32_t basebit, int32_t l,
                                 const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, int32_t* scratch, void* stream) {
  int rc = RS_OK;
  const int n = c->p.n;
  const long rows = (long)(count * (size_t)l);
  const size_t src_words = (size_t)n + 1;
  const rs::Extent x_bits{"bits", bits, count * src_words * kWord};
  const rs::Extent x_key{"sel_key", sel_key, 2 * src_words * (size_t)ks_t * 2 * N * kWord};
  const rs::Extent x_scratch{"scratch", scratch, rs::se_scratch_words((int)N, (int)l, rows, n) * kWord};
  if ((rc = refuse_overlap({"sel", sel, (size_t)rows * 4 * N * kWord}, {x_bits, x_key, x_scratch})) != RS_OK) return rc;
  if ((rc = refuse_overlap(x_scratch, {x_bits, x_key})) != RS_OK) return rc;
  if (batch && ((uintptr_t)sel & 15u)) return fail(RS_ERR_INVALID, "sel must be 16-byte aligned");
  int32_t* lut = scratch;
  int32_t* index = scratch + rs::se_scratch_index((int)N, (int)l, rows);
  int32_t* rep = scratch + rs::se_scratch_bits((int)N, (int)l, rows);
  int32_t* boot = scratch + rs::se_scratch_boot((int)N, (int)l, rows, n);
  const rs::CircuitPrepareArgs pa{lut, index, rows, (int)N, (int)basebit, (int)l};
  RS_HIP(rs::launch_circuit_prepare(pa, (hipStream_t)stream));
  if ((rc = rs_gather_rows_dev(c, rep, bits, index, (size_t)rows, stream)) != RS_OK) return rc;
  if ((rc = rs_bootstrap_lut_dev(c, boot, rep, lut, (size_t)l, 0, (size_t)rows, stream)) != RS_OK) return rc;
  if (batch) return rs_ring_selector_batch_dev(c, sel, boot, count, basebit, l, n, sel_key, ks_basebit, ks_t, stream);
  return rs_ring_selector_dev(c, sel, boot, (int32_t)count, basebit, l, n, sel_key, ks_basebit, ks_t, stream);
}

int rs_circuit_bootstrap_dev(rs_ctx* c, int32_t* sel, const int32_t* bits, int32_t depth, int32_t basebit, int32_t l,
                             const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, int32_t* scratch, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!c->keys) return fail(RS_ERR_STATE, "rs_load_keys has not been called");
  if (!sel || !bits || !sel_key || !scratch) return fail(RS_ERR_INVALID, "null pointer");
  size_t N = 0;
  if ((rc = ring_selector_shape(c, depth, basebit, l, c->p.n, sel_key, ks_basebit, ks_t, &N)) != RS_OK) return rc;
  if (depth == 0) return RS_OK;
  return circuit_bootstrap_run(c, sel, bits, (size_t)depth, N, false, basebit, l, sel_key, ks_basebit, ks_t, scratch, stream);
}

int rs_circuit_bootstrap_batch_dev(rs_ctx* c, int32_t* sel, const int32_t* bits, size_t count, int32_t basebit, int32_t l,
                                   const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, int32_t* scratch, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!c->keys) return fail(RS_ERR_STATE, "rs_load_keys has not been called");
  if (!sel || !bits || !sel_key || !scratch) return fail(RS_ERR_INVALID, "null pointer");
  size_t N = 0;
  rs::SePlan plan{};
  if ((rc = ring_selector_batch_shape(c, count, basebit, l, c->p.n, sel_key, ks_basebit, ks_t, &N, &plan)) != RS_OK) return rc;
  if (count == 0) return RS_OK;
  return circuit_bootstrap_run(c, sel, bits, count, N, true, basebit, l, sel_key, ks_basebit, ks_t, scratch, stream);
}

int rs_last_selector(rs_ctx* c, int32_t* form, int64_t* workgroups) {
  if (!c) return fail(RS_ERR_INVALID, "null context");
  if (c->sel_form.load() < 0) return fail(RS_ERR_STATE, "no selector keyswitch launched on this context yet");
  if (form) *form = c->sel_form.load();
  if (workgroups) *workgroups = (int64_t)c->sel_groups.load();
  return RS_OK;
}

// the packing key on the device (include/redsec_hip.h; kernels of rs_packkey.hip): the checks the three calls share. rows = n t.
static int pack_key_shape(const rs_ctx* c, int32_t basebit, int32_t t, bool digits, size_t* rows) {
  const int rc = refuse_digits(basebit, t, digits);
  if (rc) return rc;
  const size_t N = (size_t)c->p.N, n = (size_t)c->p.n;
  if (N < (size_t)rs::kPgMinN || N > (size_t)rs::kPgMaxN) return fail(RS_ERR_INVALID, "unsupported ring N = %zu", N);
  // rows x tiles workgroups of the generator, rows N / 16 threads of the expansion and 2 rows N words of the key, all below 2^31 x 256
  if (n < 1 || (size_t)t > (size_t)INT32_MAX / (N / 16) / n)
    return fail(RS_ERR_INVALID, "n t = %zu x %d is too large for rows of %zu words", n, (int)t, N);
  *rows = n * (size_t)t;
  return RS_OK;
}

int rs_pack_keygen_dev(rs_ctx* c, int32_t* body, const int32_t* lwe_key, const int32_t* tlwe_key, const uint8_t* mask_seed,
                       const uint8_t* noise_seed, int32_t basebit, int32_t t, double stdev) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!body || !lwe_key || !tlwe_key || !mask_seed || !noise_seed) return fail(RS_ERR_INVALID, "null pointer");
  if ((rc = rs::refuse_equal_seeds(mask_seed, noise_seed)) != RS_OK) return rc;
  if ((rc = refuse_deviation(stdev)) != RS_OK) return rc;
  size_t rows = 0;
  rc = pack_key_shape(c, basebit, t, true, &rows);
  if (rc) return rc;
  const rs_params& p = c->p;
  std::vector<uint32_t> bits;
  size_t lwe_words = 0;
  rc = pack_key_pair(p, lwe_key, tlwe_key, 32, bits, &lwe_words);
  if (rc) return rc;
  return with_secret_copy(bits, 0, [&](const uint32_t* d_bits, char*) -> int {
    rs::PackKeygenArgs a{};
    a.body = body; a.lwe_bits = d_bits; a.tlwe_bits = d_bits + lwe_words;
    rs::kg_seed_words(mask_seed, a.seed);
    rs::kg_seed_words(noise_seed, a.noise_seed);
    a.n = p.n; a.N = p.N; a.basebit = basebit; a.t = t; a.sigma = stdev;
    const hipError_t e = rs::launch_pack_keygen(a, nullptr);
    wipe_seed(a.noise_seed);
    if (e != hipSuccess) return fail(RS_ERR_HIP, "launch_pack_keygen failed: %s", hipGetErrorString(e));
    RS_HIP(hipDeviceSynchronize());
    return RS_OK;
  });
}

int rs_pack_expand_dev(rs_ctx* c, int32_t* pack_key, const uint8_t* mask_seed, const int32_t* body, int32_t t, void* stream) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!pack_key || !mask_seed || !body) return fail(RS_ERR_INVALID, "null pointer");
  size_t rows = 0;
  rc = pack_key_shape(c, 0, t, false, &rows);
  if (rc) return rc;
  rs::PackExpandArgs a{};
  a.key = pack_key; a.body = body;
  rs::kg_seed_words(mask_seed, a.seed);
  a.rows = (long)rows; a.N = c->p.N;
  RS_HIP(rs::launch_pack_expand(a, (hipStream_t)stream));
  return RS_OK;
}

// ---- device decryption and the noise audit of evaluation keys (CLIENT side; kernels of rs_audit.hip, integer arithmetic only) ----

int rs_phase_dev(rs_ctx* c, int32_t* phase, const int32_t* ct, size_t B, const int32_t* key, int32_t dim) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!phase || !ct || !key) return fail(RS_ERR_INVALID, "null pointer");
  if (dim != c->p.n && dim != c->p.k * c->p.N) return fail(RS_ERR_INVALID, "dim = %d is neither n = %d nor k N = %d", dim, c->p.n, c->p.k * c->p.N);
  if (B > (size_t)LONG_MAX) return fail(RS_ERR_INVALID, "B = %zu is too large", B);
  std::vector<uint32_t> bits;
  const int bad = pack_key_bits(key, dim, 32, bits);
  if (bad >= 0) return wiped(bits, fail(RS_ERR_INVALID, "key[%d] = %d is not 0 or 1", bad, key[bad]));
  if (B == 0) return wiped(bits, RS_OK);
  return with_secret_copy(bits, 0, [&](const uint32_t* d_bits, char*) -> int {
    RS_HIP(hipDeviceSynchronize());   // everything queued on the device, side streams included, has written ct
    rs::PhaseArgs a{phase, ct, d_bits, (long)B, dim};
    RS_HIP(rs::launch_lwe_phase(a, c->num_cus, nullptr));
    RS_HIP(hipDeviceSynchronize());
    return RS_OK;
  });
}

// rs_audit_keys_dev (mask_seed null: bk / ksk are the full key) and rs_audit_compressed_keys_dev (the bodies)
static int audit_impl(rs_ctx* c, rs_key_audit* report, int32_t* bk_noise, int32_t* ksk_noise, const uint8_t* mask_seed, bool compressed,
                      const int32_t* bk, const int32_t* ksk, const int32_t* lwe_key, const int32_t* tlwe_key, uint32_t bk_limit,
                      uint32_t ksk_limit) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!report || !lwe_key || !tlwe_key || (compressed && !mask_seed)) return fail(RS_ERR_INVALID, "null pointer");
  if (!bk && !ksk) return fail(RS_ERR_INVALID, "both halves of the key are null: nothing to audit");
  const rs_params& p = c->p;
  std::vector<uint32_t> bits;
  size_t lwe_words = 0;
  rc = pack_key_pair(p, lwe_key, tlwe_key, 32, bits, &lwe_words);
  if (rc) return rc;
  rs::AuditReportDev dev{};
  rc = with_secret_copy(bits, sizeof(rs::AuditReportDev), [&](const uint32_t* d_bits, char* d_report) -> int {
    RS_HIP(hipDeviceSynchronize());   // everything queued on the device has written the key
    rs::AuditArgs a{};
    a.bk = bk; a.ksk = ksk; a.bk_noise = bk_noise; a.ksk_noise = ksk_noise;
    a.lwe_bits = d_bits; a.tlwe_bits = d_bits + lwe_words;
    if (compressed) rs::kg_seed_words(mask_seed, a.seed);
    a.n = p.n; a.N = p.N; a.l = p.bk_l; a.bgbit = p.bk_Bgbit; a.t = p.ks_t; a.basebit = p.ks_basebit;
    a.bk_limit = bk_limit; a.ksk_limit = ksk_limit;
    a.report = reinterpret_cast<rs::AuditReportDev*>(d_report);
    if (bk) RS_HIP(rs::launch_audit_bk(a, compressed, c->num_cus, nullptr));
    if (ksk) RS_HIP(rs::launch_audit_ksk(a, compressed, c->num_cus, nullptr));
    RS_HIP(hipDeviceSynchronize());
    RS_HIP(hipMemcpy(&dev, d_report, sizeof dev, hipMemcpyDeviceToHost));
    return RS_OK;
  });
  if (rc != RS_OK) return rc;
  report->bk_max_abs = dev.bk_max_abs; report->ksk_max_abs = dev.ksk_max_abs;
  report->bk_over = dev.bk_over; report->ksk_over = dev.ksk_over; report->ksk_zero_bad = dev.ksk_zero_bad;
  report->bk_words = bk ? (uint64_t)p.n * (uint64_t)(2 * p.bk_l) * (uint64_t)p.N : 0u;
  report->ksk_words = ksk ? (uint64_t)p.N * (uint64_t)p.ks_t * (((uint64_t)1 << p.ks_basebit) - 1u) : 0u;
  return RS_OK;
}

int rs_audit_keys_dev(rs_ctx* c, rs_key_audit* report, int32_t* bk_noise, int32_t* ksk_noise, const int32_t* bk, const int32_t* ksk,
                      const int32_t* lwe_key, const int32_t* tlwe_key, uint32_t bk_limit, uint32_t ksk_limit) {
  return audit_impl(c, report, bk_noise, ksk_noise, nullptr, false, bk, ksk, lwe_key, tlwe_key, bk_limit, ksk_limit);
}
int rs_audit_compressed_keys_dev(rs_ctx* c, rs_key_audit* report, int32_t* bk_noise, int32_t* ksk_noise, const uint8_t* mask_seed,
                                 const int32_t* bk_body, const int32_t* ksk_body, const int32_t* lwe_key, const int32_t* tlwe_key,
                                 uint32_t bk_limit, uint32_t ksk_limit) {
  return audit_impl(c, report, bk_noise, ksk_noise, mask_seed, true, bk_body, ksk_body, lwe_key, tlwe_key, bk_limit, ksk_limit);
}

// the same audit of a packing key (mask_seed null: key is the full key [n][t][2][N]; else the bodies, the masks regenerated)
int rs_audit_pack_key_dev(rs_ctx* c, rs_pack_key_audit* report, int32_t* noise, const int32_t* key, const uint8_t* mask_seed,
                          const int32_t* lwe_key, const int32_t* tlwe_key, int32_t basebit, int32_t t, uint32_t limit) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!report || !key || !lwe_key || !tlwe_key) return fail(RS_ERR_INVALID, "null pointer");
  size_t rows = 0;
  rc = pack_key_shape(c, basebit, t, true, &rows);
  if (rc) return rc;
  const rs_params& p = c->p;
  std::vector<uint32_t> bits;
  size_t lwe_words = 0;
  rc = pack_key_pair(p, lwe_key, tlwe_key, 32, bits, &lwe_words);
  if (rc) return rc;
  rs::AuditReportDev dev{};
  rc = with_secret_copy(bits, sizeof(rs::AuditReportDev), [&](const uint32_t* d_bits, char* d_report) -> int {
    RS_HIP(hipDeviceSynchronize());   // everything queued on the device has written the key
    rs::AuditPackArgs a{};
    a.key = key; a.noise = noise;
    a.lwe_bits = d_bits; a.tlwe_bits = d_bits + lwe_words;
    if (mask_seed) rs::kg_seed_words(mask_seed, a.seed);
    a.n = p.n; a.N = p.N; a.t = t; a.basebit = basebit; a.limit = limit;
    a.report = reinterpret_cast<rs::AuditReportDev*>(d_report);
    RS_HIP(rs::launch_audit_pack(a, mask_seed != nullptr, c->num_cus, nullptr));
    RS_HIP(hipDeviceSynchronize());
    RS_HIP(hipMemcpy(&dev, d_report, sizeof dev, hipMemcpyDeviceToHost));
    return RS_OK;
  });
  if (rc != RS_OK) return rc;
  report->max_abs = dev.bk_max_abs;
  report->over = dev.bk_over;
  report->words = (uint64_t)rows * (uint64_t)p.N;
  return RS_OK;
}

}  // extern "C"
