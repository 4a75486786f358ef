// rs_api_keys.cpp -- the evaluation key of the C ABI (include/redsec_hip.h): loading one from its five sources, and generating
// and expanding one on the device. The three share the key's shape arithmetic and expand_args. A secret key reaches the device
// through rs::with_secret_copy (rs_api_client.cpp) alone.
#include "rs_api_internal.h"

#include <cstring>

#include "rs_general.h"
#include "rs_keygen.h"

using rs::fail;
using rs::use_device;

namespace {

// where load_keys_impl takes the key words from
enum class KeySource { kHost, kDevice, kSynthetic, kCompressedHost, kCompressedDevice };

// drops every key buffer of the context (a failed load leaves no half-built transform key behind)
void free_keys(rs_ctx* c) {
  c->keys = false;
  if (c->d_bk_ntt) { (void)hipFree(c->d_bk_ntt); c->d_bk_ntt = nullptr; }
  if (c->d_bk_fft) { (void)hipFree(c->d_bk_fft); c->d_bk_fft = nullptr; }
  if (c->d_bk_gen) { (void)hipFree(c->d_bk_gen); c->d_bk_gen = nullptr; }
  if (c->d_ksk) { (void)hipFree(c->d_ksk); c->d_ksk = nullptr; }
  c->bk_bytes = c->ksk_bytes = 0;
}

// the expansion arguments of this context's parameter set (outputs and bodies filled in by the caller)
rs::ExpandArgs expand_args(const rs_ctx* c, const uint8_t* mask_seed) {
  rs::ExpandArgs e{};
  rs::kg_seed_words(mask_seed, e.seed);
  e.n = c->p.n; e.N = c->p.N; e.l = c->p.bk_l; e.t = c->p.ks_t; e.basebit = c->p.ks_basebit;
  return e;
}

// bk / ksk: host arrays, device arrays, unused for the synthetic key of `seed` generated on the device (rs_load_synthetic_keys),
// or the bodies of a compressed key (host or device) whose masks are regenerated from mask_seed
int load_keys_impl(rs_ctx* c, KeySource src, const int32_t* bk, const int32_t* ksk, uint64_t seed,
                   const uint8_t* mask_seed = nullptr) {
  int rc = use_device(c);
  if (rc) return rc;
  if (src != KeySource::kSynthetic && (!bk || !ksk)) return fail(RS_ERR_INVALID, "null key pointer");
  const bool compressed = src == KeySource::kCompressedHost || src == KeySource::kCompressedDevice;
  if (compressed && !mask_seed) return fail(RS_ERR_INVALID, "null mask seed");
  const rs_params& p = c->p;
  const size_t n_polys = (size_t)p.n * (size_t)(2 * p.bk_l) * 2;
  const size_t bk_words = n_polys * (size_t)p.N;
  const size_t ksk_samples = (size_t)p.N * p.ks_t * ((size_t)1 << p.ks_basebit);
  const size_t ksk_words = ksk_samples * (size_t)(p.n + 1);
  free_keys(c);
  int32_t* d_bk = nullptr;     // staging copy of the key words (freed on every path)
  int32_t* d_body = nullptr;   // staging copy of host bodies of a compressed key (freed on every path)
  auto body = [&]() -> int {
    RS_HIP(hipMalloc(&d_bk, bk_words * sizeof(int32_t)));
    if (src == KeySource::kSynthetic) RS_HIP(rs::launch_synthetic_words(d_bk, seed, bk_words, nullptr));
    else if (compressed) {
      const int32_t* bk_body = bk;
      if (src == KeySource::kCompressedHost) {
        RS_HIP(hipMalloc(&d_body, bk_words / 2 * sizeof(int32_t)));
        RS_HIP(hipMemcpy(d_body, bk, bk_words / 2 * sizeof(int32_t), hipMemcpyHostToDevice));
        bk_body = d_body;
      }
      rs::ExpandArgs e = expand_args(c, mask_seed);
      e.bk = d_bk; e.bk_body = bk_body;
      RS_HIP(rs::launch_expand_bk(c->logn, e, c->num_cus, nullptr));
      RS_HIP(hipDeviceSynchronize());
      if (d_body) { RS_HIP(hipFree(d_body)); d_body = nullptr; }
    } else RS_HIP(hipMemcpy(d_bk, bk, bk_words * sizeof(int32_t), src == KeySource::kHost ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
    if (!c->general) {
      // both transform domains are kept resident (62 + 62 MB default-128, 115 + 115 MB REDsec): the FFT mode's
      // gated exact recomputation needs the NTT-domain key, and the mode can be switched per call
      RS_HIP(hipMalloc(&c->d_bk_ntt, bk_words * sizeof(double)));
      RS_HIP(hipMalloc(&c->d_bk_fft, bk_words * sizeof(double)));
      RS_HIP(rs::launch_bk_transform(c->cfg, 0, d_bk, c->d_bk_ntt, c->d_tw, c->tables.f, c->tables.ninv, (long)n_polys, nullptr));
      RS_HIP(rs::launch_bk_transform(c->cfg, 1, d_bk, c->d_bk_fft, c->d_tw_fft, c->tables.f, 0.0, (long)n_polys, nullptr));
      c->bk_bytes = bk_words * sizeof(double);
    }
    if (c->d_tw_gen) {
      // the split key: two transformed halves per polynomial (twice the bytes of one domain)
      RS_HIP(hipMalloc(&c->d_bk_gen, 2 * bk_words * sizeof(double)));
      RS_HIP(rs::launch_gen_bk_transform(c->logn, d_bk, c->d_bk_gen, c->d_tw_gen, (long)n_polys, c->num_cus, nullptr));
      if (c->general) c->bk_bytes = 2 * bk_words * sizeof(double);
    }
    RS_HIP(hipDeviceSynchronize());
    RS_HIP(hipFree(d_bk));
    d_bk = nullptr;
    RS_HIP(hipMalloc(&c->d_ksk, ksk_words * sizeof(int32_t)));
    if (src == KeySource::kSynthetic) { RS_HIP(rs::launch_synthetic_words(c->d_ksk, seed ^ 0x6b73ull, ksk_words, nullptr)); RS_HIP(hipDeviceSynchronize()); }
    else if (src == KeySource::kHost) RS_HIP(hipMemcpy(c->d_ksk, ksk, ksk_words * sizeof(int32_t), hipMemcpyHostToDevice));
    else if (src == KeySource::kDevice) { RS_HIP(hipMemcpy(c->d_ksk, ksk, ksk_words * sizeof(int32_t), hipMemcpyDeviceToDevice)); RS_HIP(hipDeviceSynchronize()); }
    else {
      const int32_t* ksk_body = ksk;
      if (src == KeySource::kCompressedHost) {
        RS_HIP(hipMalloc(&d_body, ksk_samples * sizeof(int32_t)));
        RS_HIP(hipMemcpy(d_body, ksk, ksk_samples * sizeof(int32_t), hipMemcpyHostToDevice));
        ksk_body = d_body;
      }
      rs::ExpandArgs e = expand_args(c, mask_seed);
      e.ksk = c->d_ksk; e.ksk_body = ksk_body;
      RS_HIP(rs::launch_expand_ksk(e, c->num_cus, nullptr));
      RS_HIP(hipDeviceSynchronize());
      if (d_body) { RS_HIP(hipFree(d_body)); d_body = nullptr; }
    }
    c->ksk_bytes = ksk_words * sizeof(int32_t);
    return RS_OK;
  };
  rc = body();
  if (rc != RS_OK) {
    (void)hipDeviceSynchronize();
    if (d_bk) (void)hipFree(d_bk);
    if (d_body) (void)hipFree(d_body);
    free_keys(c);
    return rc;
  }
  c->keys = true;
  return RS_OK;
}

// a failed compressed load leaves no key, invalid arguments included
int load_compressed(rs_ctx* c, KeySource src, const uint8_t* mask_seed, const int32_t* bk_body, const int32_t* ksk_body) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!mask_seed || !bk_body || !ksk_body) { free_keys(c); return fail(RS_ERR_INVALID, "null pointer"); }
  return load_keys_impl(c, src, bk_body, ksk_body, 0, mask_seed);
}

// rs_keygen_dev (noise_seed null) and rs_keygen_compressed_dev (the bodies only, masks of `seed`, noise of noise_seed)
int keygen_impl(rs_ctx* c, int32_t* bk, int32_t* ksk, const int32_t* lwe_key, const int32_t* tlwe_key, const uint8_t* seed,
                const uint8_t* noise_seed, double bk_stdev, double ks_stdev) {
  int rc = use_device(c);
  if (rc) return rc;
  const bool compressed = noise_seed != nullptr;
  if (!bk || !ksk || !lwe_key || !tlwe_key || !seed) return fail(RS_ERR_INVALID, "null pointer");
  if (((uintptr_t)bk & 15u) != 0) return fail(RS_ERR_INVALID, "bk must be 16-byte aligned");
  if (compressed && (rc = rs::refuse_equal_seeds(seed, noise_seed)) != RS_OK) return rc;
  if (!rs::deviation_ok(bk_stdev) || !rs::deviation_ok(ks_stdev))
    return fail(RS_ERR_INVALID, "noise deviations must be finite and non-negative (bk %g, ks %g)", bk_stdev, ks_stdev);
  if (!c->d_tw_gen) return fail(RS_ERR_INVALID, "split-key product not offered for this set: a-priori bound %.3g", c->split_bound);
  const rs_params& p = c->p;
  // what the kernels read: the key words themselves, int32 [n + N], and the rounding-distance flag behind them
  std::vector<uint32_t> words;
  size_t lwe_words = 0;
  rc = rs::pack_key_pair(p, lwe_key, tlwe_key, 1, words, &lwe_words);
  if (rc) return rc;
  unsigned long long flag = 0;
  rc = rs::with_secret_copy(words, sizeof flag, [&](const uint32_t* d_words, char* d_flag) -> int {
    rs::KeygenArgs a{};
    a.bk = bk; a.ksk = ksk;
    a.lwe_key = reinterpret_cast<const int32_t*>(d_words);
    a.tlwe_key = a.lwe_key + lwe_words;
    rs::kg_seed_words(seed, a.seed);
    if (compressed) rs::kg_seed_words(noise_seed, a.noise_seed);
    a.compressed = compressed ? 1 : 0;
    a.n = p.n; a.N = p.N; a.l = p.bk_l; a.bgbit = p.bk_Bgbit; a.t = p.ks_t; a.basebit = p.ks_basebit;
    a.bk_sigma = bk_stdev; a.ks_sigma = ks_stdev;
    a.dev_flag = reinterpret_cast<unsigned long long*>(d_flag);
    RS_HIP(rs::launch_keygen_bk(c->logn, a, c->d_tw_gen, c->num_cus, nullptr));
    RS_HIP(rs::launch_keygen_ksk(a, c->num_cus, nullptr));
    RS_HIP(hipDeviceSynchronize());
    RS_HIP(hipMemcpy(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost));
    return RS_OK;
  });
  if (rc != RS_OK) return rc;
  double dist = 0.0;
  memcpy(&dist, &flag, sizeof dist);
  if (!(dist < rs::kSplitBoundEnforce))
    return fail(RS_ERR_INEXACT, "key generation: a rounding distance of %.3g was observed in the a*S products (limit 1/4)", dist);
  return RS_OK;
}

}  // namespace

extern "C" {

int rs_load_keys(rs_ctx* c, const int32_t* bk, const int32_t* ksk) {
  if (!bk || !ksk) return fail(RS_ERR_INVALID, "null key pointer");
  return load_keys_impl(c, KeySource::kHost, bk, ksk, 0);
}
int rs_load_keys_dev(rs_ctx* c, const int32_t* bk, const int32_t* ksk) {
  if (!bk || !ksk) return fail(RS_ERR_INVALID, "null key pointer");
  return load_keys_impl(c, KeySource::kDevice, bk, ksk, 0);
}
int rs_load_synthetic_keys(rs_ctx* c, uint64_t seed) { return load_keys_impl(c, KeySource::kSynthetic, nullptr, nullptr, seed); }
int rs_load_compressed_keys(rs_ctx* c, const uint8_t* mask_seed, const int32_t* bk_body, const int32_t* ksk_body) {
  return load_compressed(c, KeySource::kCompressedHost, mask_seed, bk_body, ksk_body);
}
int rs_load_compressed_keys_dev(rs_ctx* c, const uint8_t* mask_seed, const int32_t* bk_body, const int32_t* ksk_body) {
  return load_compressed(c, KeySource::kCompressedDevice, mask_seed, bk_body, ksk_body);
}

int rs_keygen_dev(rs_ctx* c, int32_t* bk, int32_t* ksk, const int32_t* lwe_key, const int32_t* tlwe_key, const uint8_t* seed,
                  double bk_stdev, double ks_stdev) {
  return keygen_impl(c, bk, ksk, lwe_key, tlwe_key, seed, nullptr, bk_stdev, ks_stdev);
}
int rs_keygen_compressed_dev(rs_ctx* c, int32_t* bk_body, int32_t* ksk_body, const int32_t* lwe_key, const int32_t* tlwe_key,
                             const uint8_t* mask_seed, const uint8_t* noise_seed, double bk_stdev, double ks_stdev) {
  if (!noise_seed) return fail(RS_ERR_INVALID, "null pointer");
  return keygen_impl(c, bk_body, ksk_body, lwe_key, tlwe_key, mask_seed, noise_seed, bk_stdev, ks_stdev);
}

int rs_expand_keys_dev(rs_ctx* c, int32_t* bk, int32_t* ksk, const uint8_t* mask_seed, const int32_t* bk_body, const int32_t* ksk_body) {
  int rc = use_device(c);
  if (rc) return rc;
  if (!bk || !ksk || !mask_seed || !bk_body || !ksk_body) return fail(RS_ERR_INVALID, "null pointer");
  if (((uintptr_t)bk & 15u) != 0) return fail(RS_ERR_INVALID, "bk must be 16-byte aligned");
  rs::ExpandArgs e = expand_args(c, mask_seed);
  e.bk = bk; e.ksk = ksk; e.bk_body = bk_body; e.ksk_body = ksk_body;
  RS_HIP(rs::launch_expand_bk(c->logn, e, c->num_cus, nullptr));
  RS_HIP(rs::launch_expand_ksk(e, c->num_cus, nullptr));
  RS_HIP(hipDeviceSynchronize());
  return RS_OK;
}

}  // extern "C"
