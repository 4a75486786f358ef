// tfhe_shim.cpp -- implementation of the TFHE-compatible shim (tfhe/tfhe.h) over libredsec_hip.so.
//
// Host-side pieces restate TFHE v1.1's documented behaviour for the calls REDsec makes:
//   parameters / samples / word-wise LWE ops   lib/Layer.cpp:78-188, lib/BinOps_enc.cpp:37-41,121-143,
//                                              lib/BinFunc.cpp:207-208,251-289, lib/IntFunc.cpp:219-277
//   key generation, encrypt, decrypt           client/gen_secure_keyset.cpp:94-120,
//                                              client/encrypt_image.cpp:77, client/decrypt_image.cpp:52
//   key / ciphertext files                     nets/mnist/sign1024x1/main.cpp:68-78, net.cpp:53-55
// Every bootstrapped operation (tfhe_bootstrap_FFT, boots*) is executed on the GPU through the C ABI;
// nothing here computes a bootstrap on the CPU, and without a GPU those calls abort loudly.
#include "tfhe/tfhe.h"

#include <initializer_list>
#include <sys/stat.h>
#include <map>
#include <chrono>
#include <mutex>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "redsec_hip.h"
#include "rs_keygen.h"   // the mask streams of compressed keys and seeded ciphertexts (csrc/rs_keygen.h): one statement of ChaCha20 for device and host

// seconds spent creating device contexts and uploading / transforming keys since the last call (REDSEC_TRACE reports them apart
// from a layer's own staging: they happen once per process, inside whichever call touches the GPU first)
static double g_setup_seconds = 0.0;
double redsec_take_setup_seconds() { const double v = g_setup_seconds; g_setup_seconds = 0.0; return v; }

namespace {

std::mt19937_64& rng() {
  static std::mt19937_64 g(0x5eed5eedULL);
  return g;
}

[[noreturn]] void die(const char* what) {
  fprintf(stderr, "redsec tfhe shim: %s: %s\n", what, rs_last_error());
  abort();
}

Torus32 gaussian32(Torus32 message, double sigma) {
  std::normal_distribution<double> dist(0.0, sigma);
  return (Torus32)((uint32_t)message + (uint32_t)dtot32(dist(rng())));
}

inline uint32_t uniform32() { return (uint32_t)(rng()() >> 32); }

constexpr uint32_t kMagicSecret = 0x31535352u;  // "RSS1"
constexpr uint32_t kMagicCloud = 0x314b5352u;   // "RSK1"
constexpr uint32_t kMagicCompressed = 0x315a5352u;   // "RSZ1": RSK1's header, the 32-byte mask seed, bk_body, ksk_body
constexpr uint32_t kMagicSeededCt = 0x31435352u;     // "RSC1": RSK1's header, the 32-byte mask seed, uint64 first, int32 bodies

struct ParamHeader {
  uint32_t magic;
  int32_t n, N, k, l, Bgbit, ks_t, ks_basebit;
  double lwe_alpha_min, lwe_alpha_max, tlwe_alpha_min, tlwe_alpha_max;
};

// Parameter objects read from a key file belong to the process, as in TFHE (its readers hand them to the garbage
// collector, delete_gate_bootstrapping_*_keyset leaves them alone): kept reachable here for the process lifetime.
TFheGateBootstrappingParameterSet* params_from_header(const ParamHeader& h) {
  LweParams* lp = new_LweParams(h.n, h.lwe_alpha_min, h.lwe_alpha_max);
  TLweParams* tp = new_TLweParams(h.N, h.k, h.tlwe_alpha_min, h.tlwe_alpha_max);
  TGswParams* gp = new_TGswParams(h.l, h.Bgbit, tp);
  TFheGateBootstrappingParameterSet* p = new TFheGateBootstrappingParameterSet(h.ks_t, h.ks_basebit, lp, gp);
  static std::mutex mu;
  static std::vector<TFheGateBootstrappingParameterSet*>* const owned = new std::vector<TFheGateBootstrappingParameterSet*>();
  std::lock_guard<std::mutex> lock(mu);
  owned->push_back(p);
  return p;
}

ParamHeader header_from_params(uint32_t magic, const TFheGateBootstrappingParameterSet* p) {
  ParamHeader h;
  const TLweParams* tp = p->tgsw_params->tlwe_params;
  h.magic = magic;
  h.n = p->in_out_params->n; h.N = tp->N; h.k = tp->k; h.l = p->tgsw_params->l; h.Bgbit = p->tgsw_params->Bgbit;
  h.ks_t = p->ks_t; h.ks_basebit = p->ks_basebit;
  h.lwe_alpha_min = p->in_out_params->alpha_min; h.lwe_alpha_max = p->in_out_params->alpha_max;
  h.tlwe_alpha_min = tp->alpha_min; h.tlwe_alpha_max = tp->alpha_max;
  return h;
}

size_t bk_words(const TFheGateBootstrappingParameterSet* p) {
  const TLweParams* tp = p->tgsw_params->tlwe_params;
  return (size_t)p->in_out_params->n * p->tgsw_params->kpl * (tp->k + 1) * tp->N;
}
size_t ksk_words(const TFheGateBootstrappingParameterSet* p) {
  const TLweParams* tp = p->tgsw_params->tlwe_params;
  return (size_t)tp->N * tp->k * p->ks_t * ((size_t)1 << p->ks_basebit) * (p->in_out_params->n + 1);
}

void write_exact(FILE* f, const void* src, size_t bytes, const char* what) {
  if (fwrite(src, 1, bytes, f) != bytes) { fprintf(stderr, "redsec tfhe shim: short write (%s)\n", what); abort(); }
}
int32_t* alloc_words(size_t words, const char* what) {
  int32_t* p = (int32_t*)malloc(sizeof(int32_t) * (words ? words : 1));
  if (!p) { fprintf(stderr, "redsec tfhe shim: out of memory (%s, %zu words)\n", what, words); abort(); }
  return p;
}
// a key file's header decides allocation sizes: refuse anything outside what the backend supports
// before allocating (a truncated or foreign file must not turn into a multi-gigabyte malloc)
void check_header(const ParamHeader& h, const char* what) {
  const bool ring = h.N == 1024 || h.N == 2048 || h.N == 4096 || h.N == 8192;   // what rs_create accepts
  const bool ok = ring && h.k == 1 && h.n >= 1 && h.n <= 16384 && h.l >= 1 && h.l <= 16 && h.Bgbit >= 1 &&
                  h.l * h.Bgbit <= 32 && h.ks_t >= 1 && h.ks_basebit >= 1 && h.ks_t * h.ks_basebit <= 31;
  if (!ok) { fprintf(stderr, "redsec tfhe shim: implausible parameters in %s header\n", what); abort(); }
}

LweBootstrappingKey* new_bk(const TFheGateBootstrappingParameterSet* p) {
  LweBootstrappingKey* bk = new LweBootstrappingKey;
  bk->in_out_params = p->in_out_params;
  bk->bk_params = p->tgsw_params;
  bk->bk_words = alloc_words(bk_words(p), "bootstrapping key");
  bk->ksk_words = alloc_words(ksk_words(p), "keyswitch key");
  bk->compressed = 0;
  memset(bk->mask_seed, 0, sizeof bk->mask_seed);
  return bk;
}

// bodies of a compressed key (include/redsec_hip.h): bk_body [n][2l][N] (half the TGSW words), ksk_body [N][t][base]
size_t bk_body_words(const TFheGateBootstrappingParameterSet* p) { return bk_words(p) / 2; }
size_t ksk_body_words(const TFheGateBootstrappingParameterSet* p) { return ksk_words(p) / (size_t)(p->in_out_params->n + 1); }
LweBootstrappingKey* new_body_bk(const TFheGateBootstrappingParameterSet* p) {
  LweBootstrappingKey* bk = new LweBootstrappingKey;
  bk->in_out_params = p->in_out_params;
  bk->bk_params = p->tgsw_params;
  bk->bk_words = alloc_words(bk_body_words(p), "bootstrapping key bodies");
  bk->ksk_words = alloc_words(ksk_body_words(p), "keyswitch key bodies");
  bk->compressed = 2;
  memset(bk->mask_seed, 0, sizeof bk->mask_seed);
  return bk;
}

LweBootstrappingKeyFFT* new_bkfft(const TFheGateBootstrappingParameterSet* p, const LweBootstrappingKey* src) {
  LweBootstrappingKeyFFT* f = new LweBootstrappingKeyFFT;
  f->in_out_params = p->in_out_params;
  f->ctx = nullptr;  // created on first use: client tools never touch the GPU
  f->fleet = nullptr;
  f->fleet_size = 0;
  f->params = p;
  f->src = src;
  return f;
}

// Created on the first bootstrap; the per-ciphertext wrappers are called from OpenMP regions of the caller
// (lib/BinFunc.cpp:217,896,1056), so creation is serialised. One context per device of REDSEC_DEVICES (a device
// may be listed twice: two contexts on one GPU walk the multi-device code path on a one-GPU machine).
rs_ctx* ctx_of_fft(const LweBootstrappingKeyFFT* cf) {
  LweBootstrappingKeyFFT* f = const_cast<LweBootstrappingKeyFFT*>(cf);
  static std::mutex mu;
  std::lock_guard<std::mutex> g(mu);
  if (f->ctx) return f->ctx;
  const TFheGateBootstrappingParameterSet* p = f->params;
  const TLweParams* tp = p->tgsw_params->tlwe_params;
  rs_params rp = {p->in_out_params->n, tp->N, tp->k, p->tgsw_params->l, p->tgsw_params->Bgbit, p->ks_t, p->ks_basebit};
  std::vector<int> devices;
  if (const char* list = getenv("REDSEC_DEVICES")) {
    for (const char* q = list; *q;) {
      char* end = nullptr;
      const long d = strtol(q, &end, 10);
      if (end == q) break;
      devices.push_back((int)d);
      q = *end == ',' ? end + 1 : end;
    }
  }
  if (devices.empty()) { const char* dev = getenv("REDSEC_DEVICE"); devices.push_back(dev ? atoi(dev) : 0); }
  rs_ctx** fleet = (rs_ctx**)calloc(devices.size(), sizeof(rs_ctx*));
  const auto t_setup = std::chrono::steady_clock::now();
  for (size_t i = 0; i < devices.size(); ++i) {
    if (rs_create(&fleet[i], &rp, devices[i]) != 0) die("rs_create");
    if (f->src->compressed == 2) {   // bodies only: every device expands the masks itself
      if (rs_load_compressed_keys(fleet[i], f->src->mask_seed, f->src->bk_words, f->src->ksk_words) != 0) die("rs_load_compressed_keys");
    } else if (rs_load_keys(fleet[i], f->src->bk_words, f->src->ksk_words) != 0) die("rs_load_keys");
  }
  g_setup_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_setup).count();
  f->fleet = fleet;
  f->fleet_size = (int)devices.size();
  f->ctx = fleet[0];
  return f->ctx;
}

void read_exact(FILE* f, void* dst, size_t bytes, const char* what) {
  if (fread(dst, 1, bytes, f) != bytes) { fprintf(stderr, "redsec tfhe shim: short read (%s)\n", what); abort(); }
}
// b += s * a in Z[X]/(X^N+1), s binary
void addmul_binary(int32_t* b, const int32_t* s, const int32_t* a, int32_t N) {
  for (int32_t i = 0; i < N; ++i) {
    if (!s[i]) continue;
    for (int32_t j = 0; j < N - i; ++j) b[i + j] = (int32_t)((uint32_t)b[i + j] + (uint32_t)a[j]);
    for (int32_t j = N - i; j < N; ++j) b[i + j - N] = (int32_t)((uint32_t)b[i + j - N] - (uint32_t)a[j]);
  }
}

void gate(rs_gate_op op, LweSample* result, const LweSample* ca, const LweSample* cb, const TFheGateBootstrappingCloudKeySet* bk) {
  const int32_t n = bk->params->in_out_params->n;
  std::vector<int32_t> x(n + 1), y(n + 1), z(n + 1);
  redsec_pack(x.data(), ca, n);
  redsec_pack(y.data(), cb, n);
  if (rs_gate(redsec_ctx_of(bk), op, z.data(), x.data(), y.data(), 1) != 0) die("rs_gate");
  redsec_unpack(result, z.data(), n);
}

bool key_format_is_rs() { const char* f = getenv("REDSEC_KEY_FORMAT"); return f && strcmp(f, "rs") == 0; }
// REDSEC_KEY_FORMAT=compressed: new keys draw their masks from the ChaCha20 streams of a fresh random mask seed; the cloud key is
// written as RSZ1 (seed + bodies), the secret key as RSS1 (full words, as under REDSEC_KEY_FORMAT=rs)
bool key_format_is_compressed() { const char* f = getenv("REDSEC_KEY_FORMAT"); return f && strcmp(f, "compressed") == 0; }

// words [0, count) of stream (domain, row) of the key words `key` (csrc/rs_keygen.h)
void stream_words(const uint32_t (&key)[8], uint32_t domain, uint64_t row, uint32_t* out, size_t count) {
  for (size_t b = 0; 16 * b < count; ++b) {
    uint32_t w[16];
    rs::kg_chacha_block(key, domain, row, (uint32_t)b, w);
    for (size_t q = 0; q < 16 && 16 * b + q < count; ++q) out[16 * b + q] = w[q];
  }
}

// A compressed key in full words (include/redsec_hip.h, rs_keygen_compressed_dev): bk row p = c l + j of s_i has the domain-3
// mask of the seed and b = a*S + e + s_i g_j X^0 (c = 1) or a*S + e - s_i g_j S (c = 0); ksk sample s the domain-5 mask and
// b = a.s + e + message. The noise comes from the shim's generator (only the masks have to be reproducible).
void compressed_keygen(const TFheGateBootstrappingParameterSet* p, LweBootstrappingKey* bk, const LweKey* lk, const TGswKey* gk) {
  const TGswParams* gp = p->tgsw_params;
  const TLweParams* tp = gp->tlwe_params;
  const int32_t n = p->in_out_params->n, N = tp->N, l = gp->l, kpl = gp->kpl;
  const int32_t t = p->ks_t, basebit = p->ks_basebit, base = 1 << basebit, W = n + 1;
  std::random_device rd;
  for (int k = 0; k < 8; ++k) {
    const uint32_t v = rd();
    memcpy(bk->mask_seed + 4 * k, &v, 4);
  }
  uint32_t key[8];
  rs::kg_seed_words(bk->mask_seed, key);
  for (int32_t i = 0; i < n; ++i)
    for (int32_t row = 0; row < kpl; ++row) {
      const uint64_t r = (uint64_t)i * kpl + row;
      int32_t* apoly = bk->bk_words + r * 2 * (size_t)N;
      int32_t* bpoly = apoly + N;
      for (int32_t j = 0; j < N; ++j) bpoly[j] = gaussian32(0, tp->alpha_min);
      stream_words(key, rs::kKgBkMask, r, reinterpret_cast<uint32_t*>(apoly), (size_t)N);
      addmul_binary(bpoly, gk->key, apoly, N);
      const int32_t comp = row / l, dig = row % l;
      const uint32_t h = (uint32_t)lk->key[i] << (32 - (dig + 1) * gp->Bgbit);
      if (comp == 1) bpoly[0] = (int32_t)((uint32_t)bpoly[0] + h);
      else
        for (int32_t j = 0; j < N; ++j) bpoly[j] = (int32_t)((uint32_t)bpoly[j] - h * (uint32_t)gk->key[j]);
    }
  for (int32_t i = 0; i < N; ++i)
    for (int32_t j = 0; j < t; ++j)
      for (int32_t v = 0; v < base; ++v) {
        const uint64_t s = ((uint64_t)i * t + j) * base + v;
        int32_t* rowp = bk->ksk_words + s * (size_t)W;
        if (v == 0) { memset(rowp, 0, sizeof(int32_t) * (size_t)W); continue; }
        stream_words(key, rs::kKgKsMask, s, reinterpret_cast<uint32_t*>(rowp), (size_t)n);
        uint32_t b = (uint32_t)gaussian32(0, p->in_out_params->alpha_min);
        for (int32_t k = 0; k < n; ++k) b += (uint32_t)rowp[k] * (uint32_t)lk->key[k];
        rowp[n] = (int32_t)(b + (((uint32_t)gk->key[i] * (uint32_t)v) << (32 - (j + 1) * basebit)));
      }
  bk->compressed = 1;
}

// RSZ1: header, mask seed, bk_body, ksk_body (bodies taken out of the full words of a key generated here, or written as read)
void write_compressed(FILE* f, const TFheGateBootstrappingParameterSet* p, const LweBootstrappingKey* bk) {
  const ParamHeader h = header_from_params(kMagicCompressed, p);
  write_exact(f, &h, sizeof h, "compressed cloud key header");
  write_exact(f, bk->mask_seed, sizeof bk->mask_seed, "mask seed");
  if (bk->compressed == 2) {
    write_exact(f, bk->bk_words, sizeof(int32_t) * bk_body_words(p), "bootstrapping key bodies");
    write_exact(f, bk->ksk_words, sizeof(int32_t) * ksk_body_words(p), "keyswitch key bodies");
    return;
  }
  const size_t N = (size_t)p->tgsw_params->tlwe_params->N, W = (size_t)p->in_out_params->n + 1;
  for (size_t r = 0; r < bk_body_words(p) / N; ++r) write_exact(f, bk->bk_words + (2 * r + 1) * N, sizeof(int32_t) * N, "bootstrapping key body");
  std::vector<int32_t> kb(ksk_body_words(p));
  for (size_t s = 0; s < kb.size(); ++s) kb[s] = bk->ksk_words[s * W + W - 1];
  write_exact(f, kb.data(), sizeof(int32_t) * kb.size(), "keyswitch key bodies");
}
}  // namespace

// ---------------------------------------------------------------------------------------------
LweParams* new_LweParams(int32_t n, double alpha_min, double alpha_max) { return new LweParams(n, alpha_min, alpha_max); }
TLweParams* new_TLweParams(int32_t N, int32_t k, double alpha_min, double alpha_max) { return new TLweParams(N, k, alpha_min, alpha_max); }
TGswParams* new_TGswParams(int32_t l, int32_t Bgbit, const TLweParams* tp) { return new TGswParams(l, Bgbit, tp); }

TFheGateBootstrappingParameterSet* new_default_gate_bootstrapping_parameters(int32_t) {
  LweParams* lp = new_LweParams(630, std::pow(2., -15), std::pow(2., -15));  // max noise: TFHE uses 0.012467; unused here
  TLweParams* tp = new_TLweParams(1024, 1, std::pow(2., -25), std::pow(2., -15));
  TGswParams* gp = new_TGswParams(3, 7, tp);
  return new TFheGateBootstrappingParameterSet(8, 2, lp, gp);
}

Torus32 modSwitchToTorus32(int32_t mu, int32_t Msize) {
  const uint64_t interv = ((UINT64_C(1) << 63) / (uint64_t)Msize) * 2;
  return (Torus32)(((uint64_t)(int64_t)mu * interv) >> 32);
}
int32_t modSwitchFromTorus32(Torus32 phase, int32_t Msize) {
  const uint64_t interv = ((UINT64_C(1) << 63) / (uint64_t)Msize) * 2;
  const uint64_t phase64 = ((uint64_t)(uint32_t)phase << 32) + interv / 2;
  return (int32_t)(phase64 / interv);
}
Torus32 dtot32(double d) { return (Torus32)(int64_t)((d - (double)(int64_t)d) * 4294967296.0); }

// ---- samples: one slab of words per array ----
LweSample* new_LweSample_array(int32_t nbelts, const LweParams* params) {
  LweSample* s = new LweSample[nbelts > 0 ? nbelts : 1];
  int32_t* words = (int32_t*)calloc((size_t)(nbelts > 0 ? nbelts : 1) * (size_t)params->n, sizeof(int32_t));
  for (int32_t i = 0; i < nbelts; ++i) { s[i].a = words + (size_t)i * params->n; s[i].b = 0; s[i].current_variance = 0.; }
  if (nbelts <= 0) { s[0].a = words; s[0].b = 0; s[0].current_variance = 0.; }
  return s;
}
LweSample* new_LweSample(const LweParams* params) { return new_LweSample_array(1, params); }
void delete_LweSample_array(int32_t, LweSample* s) {
  if (!s) return;
  free(s[0].a);
  delete[] s;
}
void delete_LweSample(LweSample* s) { delete_LweSample_array(1, s); }
LweSample* new_gate_bootstrapping_ciphertext(const TFheGateBootstrappingParameterSet* p) { return new_LweSample(p->in_out_params); }
LweSample* new_gate_bootstrapping_ciphertext_array(int32_t nbelems, const TFheGateBootstrappingParameterSet* p) {
  return new_LweSample_array(nbelems, p->in_out_params);
}
void delete_gate_bootstrapping_ciphertext(LweSample* s) { delete_LweSample(s); }
void delete_gate_bootstrapping_ciphertext_array(int32_t nbelems, LweSample* s) { delete_LweSample_array(nbelems, s); }

void lweClear(LweSample* r, const LweParams* p) {
  memset(r->a, 0, sizeof(Torus32) * (size_t)p->n);
  r->b = 0; r->current_variance = 0.;
}
void lweCopy(LweSample* r, const LweSample* s, const LweParams* p) {
  memmove(r->a, s->a, sizeof(Torus32) * (size_t)p->n);
  r->b = s->b; r->current_variance = s->current_variance;
}
void lweNegate(LweSample* r, const LweSample* s, const LweParams* p) {
  for (int32_t i = 0; i < p->n; ++i) r->a[i] = (Torus32)(0u - (uint32_t)s->a[i]);
  r->b = (Torus32)(0u - (uint32_t)s->b); r->current_variance = s->current_variance;
}
void lweNoiselessTrivial(LweSample* r, Torus32 mu, const LweParams* p) {
  memset(r->a, 0, sizeof(Torus32) * (size_t)p->n);
  r->b = mu; r->current_variance = 0.;
}
void lweAddTo(LweSample* r, const LweSample* s, const LweParams* p) {
  for (int32_t i = 0; i < p->n; ++i) r->a[i] = (Torus32)((uint32_t)r->a[i] + (uint32_t)s->a[i]);
  r->b = (Torus32)((uint32_t)r->b + (uint32_t)s->b); r->current_variance += s->current_variance;
}
void lweSubTo(LweSample* r, const LweSample* s, const LweParams* p) {
  for (int32_t i = 0; i < p->n; ++i) r->a[i] = (Torus32)((uint32_t)r->a[i] - (uint32_t)s->a[i]);
  r->b = (Torus32)((uint32_t)r->b - (uint32_t)s->b); r->current_variance += s->current_variance;
}
void lweAddMulTo(LweSample* r, int32_t k, const LweSample* s, const LweParams* p) {
  for (int32_t i = 0; i < p->n; ++i) r->a[i] = (Torus32)((uint32_t)r->a[i] + (uint32_t)k * (uint32_t)s->a[i]);
  r->b = (Torus32)((uint32_t)r->b + (uint32_t)k * (uint32_t)s->b); r->current_variance += (double)k * k * s->current_variance;
}
void lweSubMulTo(LweSample* r, int32_t k, const LweSample* s, const LweParams* p) {
  for (int32_t i = 0; i < p->n; ++i) r->a[i] = (Torus32)((uint32_t)r->a[i] - (uint32_t)k * (uint32_t)s->a[i]);
  r->b = (Torus32)((uint32_t)r->b - (uint32_t)k * (uint32_t)s->b); r->current_variance += (double)k * k * s->current_variance;
}

namespace {
// TFHE's lweSymEncrypt: masks from the shim's generator (key generation always takes this path)
void lwe_sym_encrypt_uniform(LweSample* r, Torus32 message, double alpha, const LweKey* key) {
  const int32_t n = key->params->n;
  uint32_t b = (uint32_t)gaussian32(message, alpha);
  for (int32_t i = 0; i < n; ++i) {
    const uint32_t a = uniform32();
    r->a[i] = (Torus32)a;
    b += a * (uint32_t)key->key[i];
  }
  r->b = (Torus32)b;
  r->current_variance = alpha * alpha;
}

// ---- seeded ciphertexts (include/redsec_hip.h rs_encrypt_seeded_dev) ----
// REDSEC_CT_FORMAT=seeded: lweSymEncrypt draws the mask of each new sample from stream (7, row) of a per-process random mask seed,
// rows 0, 1, 2, ... in call order (the noise still comes from the shim's generator: only the masks must be reproducible), and
// export_gate_bootstrapping_ciphertext_toFile writes RSC1 files: the first export to a file writes the header, the seed and the
// sample's row as `first`, every later one just the body. import_gate_bootstrapping_ciphertext_fromFile reads RSC1 in every mode.
bool ct_format_is_seeded() { const char* f = getenv("REDSEC_CT_FORMAT"); return f && strcmp(f, "seeded") == 0; }

struct SeededWriter {
  std::mutex mu;
  bool have_seed = false;
  uint8_t seed[32];
  uint32_t key[8];
  uint64_t next_row = 0;
  std::map<const Torus32*, uint64_t> row_of;   // mask array of a sample -> the row its mask was drawn at
};
SeededWriter& seeded_writer() {
  static SeededWriter* const w = new SeededWriter();
  return *w;
}

// per open file: the position after the last record this shim read or wrote, and the row of the next sample. A state whose file
// (device, inode) or position does not match is stale: the FILE* address was reused for another file.
struct CtFileState {
  dev_t dev = 0;
  ino_t ino = 0;
  long pos = -1;
  uint32_t key[8];
  uint64_t next_row = 0;
};
std::mutex g_ct_files_mu;
std::map<FILE*, CtFileState>& ct_files(bool reading) {
  static std::map<FILE*, CtFileState>* const r = new std::map<FILE*, CtFileState>();
  static std::map<FILE*, CtFileState>* const w = new std::map<FILE*, CtFileState>();
  return reading ? *r : *w;
}
void file_id(FILE* f, dev_t* dev, ino_t* ino) {
  struct stat st;
  if (fstat(fileno(f), &st) == 0) { *dev = st.st_dev; *ino = st.st_ino; }
  else { *dev = 0; *ino = 0; }
}
// the live state of f, or null when f is at its start or its state is stale
CtFileState* ct_file_state(FILE* f, bool reading) {
  auto& m = ct_files(reading);
  const auto it = m.find(f);
  if (it == m.end()) return nullptr;
  dev_t dev; ino_t ino;
  file_id(f, &dev, &ino);
  const long pos = ftell(f);
  if (pos == 0 || it->second.dev != dev || it->second.ino != ino || it->second.pos != pos) { m.erase(it); return nullptr; }
  return &it->second;
}

[[noreturn]] void ct_die(const char* what) {
  fprintf(stderr, "redsec tfhe shim: REDSEC_CT_FORMAT=seeded: %s\n", what);
  abort();
}
}  // namespace

void lweSymEncrypt(LweSample* r, Torus32 message, double alpha, const LweKey* key) {
  if (!ct_format_is_seeded()) { lwe_sym_encrypt_uniform(r, message, alpha, key); return; }
  const int32_t n = key->params->n;
  SeededWriter& w = seeded_writer();
  std::lock_guard<std::mutex> lock(w.mu);
  if (!w.have_seed) {
    std::random_device rd;
    for (int k = 0; k < 8; ++k) {
      const uint32_t v = rd();
      memcpy(w.seed + 4 * k, &v, 4);
    }
    rs::kg_seed_words(w.seed, w.key);
    w.have_seed = true;
  }
  const uint64_t row = w.next_row++;
  uint32_t b = (uint32_t)gaussian32(message, alpha);
  for (int32_t blk = 0; 16 * blk < n; ++blk) {
    uint32_t words[16];
    rs::kg_ct_mask_block(w.key, row, blk, words);
    for (int32_t q = 0; q < 16 && 16 * blk + q < n; ++q) {
      r->a[16 * blk + q] = (Torus32)words[q];
      b += words[q] * (uint32_t)key->key[16 * blk + q];
    }
  }
  r->b = (Torus32)b;
  r->current_variance = alpha * alpha;
  w.row_of[r->a] = row;
}
Torus32 lwePhase(const LweSample* s, const LweKey* key) {
  uint32_t axs = 0;
  for (int32_t i = 0; i < key->params->n; ++i) axs += (uint32_t)s->a[i] * (uint32_t)key->key[i];
  return (Torus32)((uint32_t)s->b - axs);
}
Torus32 lweSymDecrypt(const LweSample* s, const LweKey* key, const int32_t Msize) {
  const uint64_t interv = ((UINT64_C(1) << 63) / (uint64_t)Msize) * 2;
  uint64_t phase64 = ((uint64_t)(uint32_t)lwePhase(s, key) << 32) + interv / 2;
  phase64 -= phase64 % interv;
  return (Torus32)(phase64 >> 32);
}

// ---- keys ----
void tfhe_random_generator_setSeed(uint32_t* values, int32_t size) {
  std::seed_seq seq(values, values + size);
  rng().seed(seq);
}

TFheGateBootstrappingSecretKeySet* new_random_gate_bootstrapping_secret_keyset(const TFheGateBootstrappingParameterSet* p) {
  const TGswParams* gp = p->tgsw_params;
  const TLweParams* tp = gp->tlwe_params;
  const int32_t n = p->in_out_params->n, N = tp->N, k = tp->k, l = gp->l, kpl = gp->kpl;
  const int32_t t = p->ks_t, basebit = p->ks_basebit, base = 1 << basebit, W = n + 1;
  if (k != 1) { fprintf(stderr, "redsec tfhe shim: k = %d unsupported\n", k); abort(); }
  LweKey* lk = new LweKey{p->in_out_params, alloc_words((size_t)n, "lwe key")};
  TGswKey* gk = new TGswKey{gp, alloc_words((size_t)k * N, "tlwe key")};
  for (int32_t i = 0; i < n; ++i) lk->key[i] = (int32_t)(uniform32() & 1u);
  for (int32_t i = 0; i < k * N; ++i) gk->key[i] = (int32_t)(uniform32() & 1u);
  LweBootstrappingKey* bk = new_bk(p);
  if (key_format_is_compressed()) {
    compressed_keygen(p, bk, lk, gk);
    return new TFheGateBootstrappingSecretKeySet(p, bk, new_bkfft(p, bk), lk, gk);
  }
  // TGSW(s_i): row c*l + j = TRLWE encryption of zero + s_i * 2^(32-(j+1)Bgbit) on component c
  for (int32_t i = 0; i < n; ++i)
    for (int32_t row = 0; row < kpl; ++row) {
      int32_t* smp = bk->bk_words + (((size_t)i * kpl + row) * (k + 1)) * (size_t)N;
      int32_t* apoly = smp;
      int32_t* bpoly = smp + (size_t)k * N;
      for (int32_t j = 0; j < N; ++j) bpoly[j] = gaussian32(0, tp->alpha_min);
      for (int32_t j = 0; j < N; ++j) apoly[j] = (int32_t)uniform32();
      addmul_binary(bpoly, gk->key, apoly, N);
      const int32_t comp = row / l, dig = row % l;
      const uint32_t h = (uint32_t)1 << (32 - (dig + 1) * gp->Bgbit);
      smp[(size_t)comp * N] = (int32_t)((uint32_t)smp[(size_t)comp * N] + (uint32_t)lk->key[i] * h);
    }
  // keyswitch key: extracted key (N words) -> LWE key
  LweSample tmp;
  for (int32_t i = 0; i < k * N; ++i)
    for (int32_t j = 0; j < t; ++j)
      for (int32_t v = 0; v < base; ++v) {
        int32_t* rowp = bk->ksk_words + ((((size_t)i * t + j) * base) + v) * (size_t)W;
        tmp.a = rowp;
        if (v == 0) { lweNoiselessTrivial(&tmp, 0, p->in_out_params); rowp[n] = 0; continue; }
        const uint32_t mess = ((uint32_t)gk->key[i] * (uint32_t)v) << (32 - (j + 1) * basebit);
        lwe_sym_encrypt_uniform(&tmp, (Torus32)mess, p->in_out_params->alpha_min, lk);
        rowp[n] = tmp.b;
      }
  return new TFheGateBootstrappingSecretKeySet(p, bk, new_bkfft(p, bk), lk, gk);
}

static void free_cloud_parts(const TFheGateBootstrappingCloudKeySet* c) {
  if (c->bkFFT) {
    for (int i = 0; i < c->bkFFT->fleet_size; ++i) { redsec_pool_release(c->bkFFT->fleet[i]); rs_destroy(c->bkFFT->fleet[i]); }
    free(c->bkFFT->fleet);
    delete c->bkFFT;
  }
  if (c->bk) { free(c->bk->bk_words); free(c->bk->ksk_words); delete c->bk; }
}
void delete_gate_bootstrapping_secret_keyset(TFheGateBootstrappingSecretKeySet* ks) {
  if (!ks) return;
  free_cloud_parts(&ks->cloud);
  free(ks->lwe_key->key); delete ks->lwe_key;
  free(ks->tgsw_key->key); delete ks->tgsw_key;
  delete ks;
}
void delete_gate_bootstrapping_cloud_keyset(TFheGateBootstrappingCloudKeySet* ks) {
  if (!ks) return;
  free_cloud_parts(ks);
  delete ks;
}
void delete_gate_bootstrapping_parameters(TFheGateBootstrappingParameterSet*) {}

// ---- files ----
// KEY FILES. Two formats are read, told apart by the first bytes; REDSEC_KEY_FORMAT=rs selects the private one
// for writing, the default is TFHE's layout -- EXPERIMENTAL until tools/tfhe_crosscheck.md has been run against a real libtfhe:
// files round-trip between this shim and redsec_amd/client.py (two restatements of one recollection), nothing more is claimed,
// and INTEGRATION.md says so. REDSEC_KEY_FORMAT=rs is the verified choice for files that only this backend reads.
//
// (1) TFHE v1.1's own (tfhe_io.cpp write_tfheGateBootstrappingCloudKeySet / ...SecretKeySet) [TFHE-recalled:
//     the library is not in this image, so this is restated from its published source and could not be run
//     against it -- tools/tfhe_crosscheck.md is the recipe for whoever has libtfhe]:
//       text sections "-----BEGIN <TITLE>-----\n" / "name: value\n"... / "-----END <TITLE>-----\n", names sorted:
//         GATEBOOTSPARAMS {ks_basebit, ks_t}; LWEPARAMS {alpha_max, alpha_min, n};
//         TLWEPARAMS {N, alpha_max, alpha_min, k}; TGSWPARAMS {Bgbit, l}
//       then the bootstrapping key: int32 uid; text section LWEKSPARAMS {basebit, n (= k N), t};
//         keyswitch key: int32 uid, double max variance, N t base x (int32 a[n], int32 b);
//         n x TGSW sample: int32 uid, double max variance, (k+1) l x (k+1) x int32[N]
//       secret key files continue with: int32 uid, int32 lwe_key[n]; int32 uid, k x int32 tlwe_key[N].
//     The reader takes the sizes from the text sections and does not insist on the uid VALUES (a mismatch is
//     reported on stderr unless REDSEC_TFHE_QUIET is set), since those constants are the least certain part of
//     the restatement; REDSEC_TFHE_STRICT=1 turns a mismatch into an error.
// (2) this backend's first format: 16-byte-aligned header with magic "RSK1"/"RSS1" + raw arrays.
// (3) the compressed cloud key "RSZ1" (include/redsec_hip.h): RSK1's header, the 32-byte mask seed,
//     bk_body [n][2l][N], ksk_body [N][t][base]. Read as seed + bodies (ctx_of_fft expands them on every device); written for
//     key sets read from RSZ1 or generated under REDSEC_KEY_FORMAT=compressed, whatever REDSEC_KEY_FORMAT says.
namespace {

enum TfheUid : int32_t {   // [TFHE-recalled]
  kUidLweSample = 42, kUidLweKey = 43, kUidTlweKey = 45, kUidTgswSample = 47, kUidLweKeySwitchKey = 200, kUidLweBootstrappingKey = 201,
};


void put_section(FILE* f, const char* title, std::initializer_list<std::pair<const char*, std::string>> props) {
  fprintf(f, "-----BEGIN %s-----\n", title);
  for (const auto& kv : props) fprintf(f, "%s: %s\n", kv.first, kv.second.c_str());
  fprintf(f, "-----END %s-----\n", title);
}
std::string num(long v) { return std::to_string(v); }
std::string num(double v) { char b[64]; snprintf(b, sizeof b, "%.17g", v); return b; }

bool get_line(FILE* f, std::string* line) {
  line->clear();
  int ch;
  while ((ch = fgetc(f)) != EOF) { if (ch == '\n') return true; line->push_back((char)ch); }
  return !line->empty();
}
struct Section { std::string title; std::map<std::string, std::string> kv; };
Section get_section(FILE* f, const char* want) {
  Section s;
  std::string line;
  if (!get_line(f, &line) || line.rfind("-----BEGIN ", 0) != 0 || line.size() < 16) { fprintf(stderr, "redsec tfhe shim: key file: expected section %s\n", want); abort(); }
  s.title = line.substr(11, line.size() - 16);
  if (s.title != want) { fprintf(stderr, "redsec tfhe shim: key file: section %s where %s was expected\n", s.title.c_str(), want); abort(); }
  while (get_line(f, &line)) {
    if (line.rfind("-----END ", 0) == 0) return s;
    const size_t pos = line.find(": ");
    if (pos == std::string::npos) continue;
    s.kv[line.substr(0, pos)] = line.substr(pos + 2);
  }
  fprintf(stderr, "redsec tfhe shim: key file: section %s is not terminated\n", want);
  abort();
}
long prop_long(const Section& s, const char* k) {
  auto it = s.kv.find(k);
  if (it == s.kv.end()) { fprintf(stderr, "redsec tfhe shim: key file: %s lacks %s\n", s.title.c_str(), k); abort(); }
  return strtol(it->second.c_str(), nullptr, 10);
}
double prop_double(const Section& s, const char* k) {
  auto it = s.kv.find(k);
  if (it == s.kv.end()) { fprintf(stderr, "redsec tfhe shim: key file: %s lacks %s\n", s.title.c_str(), k); abort(); }
  return strtod(it->second.c_str(), nullptr);
}
void put_uid(FILE* f, int32_t uid) { write_exact(f, &uid, sizeof uid, "type uid"); }
void get_uid(FILE* f, int32_t want, const char* what) {
  int32_t uid = 0;
  read_exact(f, &uid, sizeof uid, what);
  if (uid == want) return;
  if (getenv("REDSEC_TFHE_STRICT")) { fprintf(stderr, "redsec tfhe shim: %s: type uid %d, expected %d\n", what, uid, want); abort(); }
  if (!getenv("REDSEC_TFHE_QUIET")) fprintf(stderr, "redsec tfhe shim: note: %s carries type uid %d (this reader expected %d; sizes come from the parameter sections)\n", what, uid, want);
}

void tfhe_write_params(FILE* f, const TFheGateBootstrappingParameterSet* p) {
  const TLweParams* tp = p->tgsw_params->tlwe_params;
  put_section(f, "GATEBOOTSPARAMS", {{"ks_basebit", num((long)p->ks_basebit)}, {"ks_t", num((long)p->ks_t)}});
  put_section(f, "LWEPARAMS", {{"alpha_max", num(p->in_out_params->alpha_max)}, {"alpha_min", num(p->in_out_params->alpha_min)}, {"n", num((long)p->in_out_params->n)}});
  put_section(f, "TLWEPARAMS", {{"N", num((long)tp->N)}, {"alpha_max", num(tp->alpha_max)}, {"alpha_min", num(tp->alpha_min)}, {"k", num((long)tp->k)}});
  put_section(f, "TGSWPARAMS", {{"Bgbit", num((long)p->tgsw_params->Bgbit)}, {"l", num((long)p->tgsw_params->l)}});
}
TFheGateBootstrappingParameterSet* tfhe_read_params(FILE* f) {
  const Section g = get_section(f, "GATEBOOTSPARAMS"), lw = get_section(f, "LWEPARAMS"), tl = get_section(f, "TLWEPARAMS"),
                tg = get_section(f, "TGSWPARAMS");
  ParamHeader h{};
  h.n = (int32_t)prop_long(lw, "n"); h.N = (int32_t)prop_long(tl, "N"); h.k = (int32_t)prop_long(tl, "k");
  h.l = (int32_t)prop_long(tg, "l"); h.Bgbit = (int32_t)prop_long(tg, "Bgbit");
  h.ks_t = (int32_t)prop_long(g, "ks_t"); h.ks_basebit = (int32_t)prop_long(g, "ks_basebit");
  h.lwe_alpha_min = prop_double(lw, "alpha_min"); h.lwe_alpha_max = prop_double(lw, "alpha_max");
  h.tlwe_alpha_min = prop_double(tl, "alpha_min"); h.tlwe_alpha_max = prop_double(tl, "alpha_max");
  check_header(h, "TFHE key file");
  return params_from_header(h);
}
void tfhe_write_bk(FILE* f, const TFheGateBootstrappingParameterSet* p, const LweBootstrappingKey* bk) {
  const TLweParams* tp = p->tgsw_params->tlwe_params;
  const int32_t n = p->in_out_params->n, N = tp->N, k = tp->k, kpl = p->tgsw_params->kpl;
  put_uid(f, kUidLweBootstrappingKey);
  put_section(f, "LWEKSPARAMS", {{"basebit", num((long)p->ks_basebit)}, {"n", num((long)(k * N))}, {"t", num((long)p->ks_t)}});
  put_uid(f, kUidLweKeySwitchKey);
  const double ks_var = p->in_out_params->alpha_min * p->in_out_params->alpha_min;
  write_exact(f, &ks_var, sizeof ks_var, "keyswitch variance");
  write_exact(f, bk->ksk_words, sizeof(int32_t) * ksk_words(p), "keyswitch key");      // [kN][t][base] x (a[n], b): TFHE's ks0_raw order
  const double bk_var = tp->alpha_min * tp->alpha_min;
  const size_t sample_words = (size_t)kpl * (k + 1) * N;
  for (int32_t i = 0; i < n; ++i) {
    put_uid(f, kUidTgswSample);
    write_exact(f, &bk_var, sizeof bk_var, "TGSW variance");
    write_exact(f, bk->bk_words + (size_t)i * sample_words, sizeof(int32_t) * sample_words, "TGSW sample");
  }
}
LweBootstrappingKey* tfhe_read_bk(FILE* f, const TFheGateBootstrappingParameterSet* p) {
  const TLweParams* tp = p->tgsw_params->tlwe_params;
  const int32_t n = p->in_out_params->n, N = tp->N, k = tp->k, kpl = p->tgsw_params->kpl;
  get_uid(f, kUidLweBootstrappingKey, "bootstrapping key");
  const Section ks = get_section(f, "LWEKSPARAMS");
  if (prop_long(ks, "n") != (long)k * N || prop_long(ks, "t") != p->ks_t || prop_long(ks, "basebit") != p->ks_basebit) {
    fprintf(stderr, "redsec tfhe shim: key file: LWEKSPARAMS disagree with the parameter sections\n");
    abort();
  }
  LweBootstrappingKey* bk = new_bk(p);
  double var = 0;
  get_uid(f, kUidLweKeySwitchKey, "keyswitch key");
  read_exact(f, &var, sizeof var, "keyswitch variance");
  read_exact(f, bk->ksk_words, sizeof(int32_t) * ksk_words(p), "keyswitch key");
  const size_t sample_words = (size_t)kpl * (k + 1) * N;
  for (int32_t i = 0; i < n; ++i) {
    get_uid(f, kUidTgswSample, "TGSW sample");
    read_exact(f, &var, sizeof var, "TGSW variance");
    read_exact(f, bk->bk_words + (size_t)i * sample_words, sizeof(int32_t) * sample_words, "TGSW sample");
  }
  return bk;
}
// first bytes decide the format: '-' opens a TFHE text section
bool file_is_tfhe(FILE* f) {
  const int ch = fgetc(f);
  if (ch == EOF) { fprintf(stderr, "redsec tfhe shim: empty key file\n"); abort(); }
  ungetc(ch, f);
  return ch == '-';
}

}  // namespace

void export_tfheGateBootstrappingCloudKeySet_toFile(FILE* f, const TFheGateBootstrappingCloudKeySet* key) {
  if (key->bk->compressed) { write_compressed(f, key->params, key->bk); return; }
  if (!key_format_is_rs()) { tfhe_write_params(f, key->params); tfhe_write_bk(f, key->params, key->bk); return; }
  const ParamHeader h = header_from_params(kMagicCloud, key->params);
  write_exact(f, &h, sizeof h, "cloud key header");
  write_exact(f, key->bk->bk_words, sizeof(int32_t) * bk_words(key->params), "bootstrapping key");
  write_exact(f, key->bk->ksk_words, sizeof(int32_t) * ksk_words(key->params), "keyswitch key");
}
void export_tfheGateBootstrappingSecretKeySet_toFile(FILE* f, const TFheGateBootstrappingSecretKeySet* key) {
  const ParamHeader h = header_from_params(kMagicSecret, key->params);
  if (!key_format_is_rs() && !key->cloud.bk->compressed) {   // write_tfheGateBootstrappingSecretKeySet: cloud part, lwe key, tgsw (= tlwe) key
    tfhe_write_params(f, key->params);
    tfhe_write_bk(f, key->params, key->cloud.bk);
    put_uid(f, kUidLweKey);
    write_exact(f, key->lwe_key->key, sizeof(int32_t) * (size_t)h.n, "lwe key");
    put_uid(f, kUidTlweKey);
    write_exact(f, key->tgsw_key->key, sizeof(int32_t) * (size_t)h.k * h.N, "tlwe key");
    return;
  }
  write_exact(f, &h, sizeof h, "secret key header");
  write_exact(f, key->lwe_key->key, sizeof(int32_t) * (size_t)h.n, "lwe key");
  write_exact(f, key->tgsw_key->key, sizeof(int32_t) * (size_t)h.k * h.N, "tlwe key");
  write_exact(f, key->cloud.bk->bk_words, sizeof(int32_t) * bk_words(key->params), "bootstrapping key");
  write_exact(f, key->cloud.bk->ksk_words, sizeof(int32_t) * ksk_words(key->params), "keyswitch key");
}
TFheGateBootstrappingCloudKeySet* new_tfheGateBootstrappingCloudKeySet_fromFile(FILE* f) {
  if (file_is_tfhe(f)) {
    TFheGateBootstrappingParameterSet* p = tfhe_read_params(f);
    LweBootstrappingKey* bk = tfhe_read_bk(f, p);
    return new TFheGateBootstrappingCloudKeySet(p, bk, new_bkfft(p, bk));
  }
  ParamHeader h;
  read_exact(f, &h, sizeof h, "cloud key header");
  if (h.magic == kMagicCompressed) {   // kept as seed + bodies: the devices expand them (ctx_of_fft), the host never does
    check_header(h, "compressed cloud key");
    TFheGateBootstrappingParameterSet* p = params_from_header(h);
    LweBootstrappingKey* bk = new_body_bk(p);
    read_exact(f, bk->mask_seed, sizeof bk->mask_seed, "mask seed");
    read_exact(f, bk->bk_words, sizeof(int32_t) * bk_body_words(p), "bootstrapping key bodies");
    read_exact(f, bk->ksk_words, sizeof(int32_t) * ksk_body_words(p), "keyswitch key bodies");
    return new TFheGateBootstrappingCloudKeySet(p, bk, new_bkfft(p, bk));
  }
  if (h.magic != kMagicCloud) { fprintf(stderr, "redsec tfhe shim: not a cloud key file\n"); abort(); }
  check_header(h, "cloud key");
  TFheGateBootstrappingParameterSet* p = params_from_header(h);
  LweBootstrappingKey* bk = new_bk(p);
  read_exact(f, bk->bk_words, sizeof(int32_t) * bk_words(p), "bootstrapping key");
  read_exact(f, bk->ksk_words, sizeof(int32_t) * ksk_words(p), "keyswitch key");
  return new TFheGateBootstrappingCloudKeySet(p, bk, new_bkfft(p, bk));
}
TFheGateBootstrappingSecretKeySet* new_tfheGateBootstrappingSecretKeySet_fromFile(FILE* f) {
  if (file_is_tfhe(f)) {
    TFheGateBootstrappingParameterSet* p = tfhe_read_params(f);
    LweBootstrappingKey* bk = tfhe_read_bk(f, p);
    const int32_t n = p->in_out_params->n, kN = p->tgsw_params->tlwe_params->k * p->tgsw_params->tlwe_params->N;
    LweKey* lk = new LweKey{p->in_out_params, alloc_words((size_t)n, "lwe key")};
    TGswKey* gk = new TGswKey{p->tgsw_params, alloc_words((size_t)kN, "tlwe key")};
    get_uid(f, kUidLweKey, "lwe key");
    read_exact(f, lk->key, sizeof(int32_t) * (size_t)n, "lwe key");
    get_uid(f, kUidTlweKey, "tlwe key");
    read_exact(f, gk->key, sizeof(int32_t) * (size_t)kN, "tlwe key");
    return new TFheGateBootstrappingSecretKeySet(p, bk, new_bkfft(p, bk), lk, gk);
  }
  ParamHeader h;
  read_exact(f, &h, sizeof h, "secret key header");
  if (h.magic != kMagicSecret) { fprintf(stderr, "redsec tfhe shim: not a secret key file\n"); abort(); }
  check_header(h, "secret key");
  TFheGateBootstrappingParameterSet* p = params_from_header(h);
  LweKey* lk = new LweKey{p->in_out_params, alloc_words((size_t)h.n, "lwe key")};
  TGswKey* gk = new TGswKey{p->tgsw_params, alloc_words((size_t)h.k * h.N, "tlwe key")};
  read_exact(f, lk->key, sizeof(int32_t) * h.n, "lwe key");
  read_exact(f, gk->key, sizeof(int32_t) * (size_t)h.k * h.N, "tlwe key");
  LweBootstrappingKey* bk = new_bk(p);
  read_exact(f, bk->bk_words, sizeof(int32_t) * bk_words(p), "bootstrapping key");
  read_exact(f, bk->ksk_words, sizeof(int32_t) * ksk_words(p), "keyswitch key");
  return new TFheGateBootstrappingSecretKeySet(p, bk, new_bkfft(p, bk), lk, gk);
}
// TFHE v1.1's LweSample record (tfhe_io.cpp write_lweSample): int32 type uid 42, int32 a[n], int32 b,
// double current_variance = 4n + 16 bytes -- image.ctxt / network_output.ctxt
// written here are byte-compatible with a TFHE client's.
static const int32_t kLweSampleTypeUid = kUidLweSample;
// Under REDSEC_CT_FORMAT=seeded the records are RSC1 instead (see lweSymEncrypt): a sample whose mask is no longer its stream's
// words (after lweAddTo, say), that was not encrypted here, or whose row is not the next one of the file, cannot be written so.
static void export_seeded(FILE* f, const LweSample* s, const TFheGateBootstrappingParameterSet* p) {
  const int32_t n = p->in_out_params->n;
  SeededWriter& w = seeded_writer();
  uint64_t row = 0;
  {
    std::lock_guard<std::mutex> lock(w.mu);
    const auto it = w.row_of.find(s->a);
    if (it == w.row_of.end()) ct_die("the sample was not encrypted by lweSymEncrypt in this process; unset it to write TFHE records");
    row = it->second;
    for (int32_t blk = 0; 16 * blk < n; ++blk) {
      uint32_t words[16];
      rs::kg_ct_mask_block(w.key, row, blk, words);
      for (int32_t q = 0; q < 16 && 16 * blk + q < n; ++q)
        if ((uint32_t)s->a[16 * blk + q] != words[q])
          ct_die("the sample's mask is no longer its stream's words (changed after encryption); unset it to write TFHE records");
    }
  }
  std::lock_guard<std::mutex> lock(g_ct_files_mu);
  CtFileState* st = ct_file_state(f, false);
  if (!st) {
    const ParamHeader h = header_from_params(kMagicSeededCt, p);
    write_exact(f, &h, sizeof h, "seeded ciphertext header");
    write_exact(f, w.seed, sizeof w.seed, "mask seed");
    write_exact(f, &row, sizeof row, "first row");
    st = &ct_files(false)[f];
    file_id(f, &st->dev, &st->ino);
    st->next_row = row;
  }
  if (row != st->next_row) ct_die("the samples of one file must be exported in the order they were encrypted, without gaps");
  write_exact(f, &s->b, sizeof(Torus32), "sample body");
  st->next_row = row + 1;
  st->pos = ftell(f);
}
void export_gate_bootstrapping_ciphertext_toFile(FILE* f, const LweSample* s, const TFheGateBootstrappingParameterSet* p) {
  if (ct_format_is_seeded()) { export_seeded(f, s, p); return; }
  write_exact(f, &kLweSampleTypeUid, sizeof(int32_t), "sample type uid");
  write_exact(f, s->a, sizeof(Torus32) * (size_t)p->in_out_params->n, "sample mask");
  write_exact(f, &s->b, sizeof(Torus32), "sample body");
  write_exact(f, &s->current_variance, sizeof(double), "sample variance");
}
// The format is told apart by the first word of the file: 42 (TFHE records) or "RSC1". An RSC1 file's state (mask seed, next row)
// is kept per FILE* and each mask is regenerated here from stream (7, row) of its seed.
void import_gate_bootstrapping_ciphertext_fromFile(FILE* f, LweSample* s, const TFheGateBootstrappingParameterSet* p) {
  const int32_t n = p->in_out_params->n;
  std::lock_guard<std::mutex> lock(g_ct_files_mu);
  CtFileState* st = ct_file_state(f, true);
  if (!st) {
    uint32_t word = 0;
    read_exact(f, &word, sizeof word, "ciphertext type uid");
    if (word == kMagicSeededCt) {
      ParamHeader h;
      h.magic = word;
      read_exact(f, reinterpret_cast<char*>(&h) + sizeof word, sizeof h - sizeof word, "seeded ciphertext header");
      const ParamHeader want = header_from_params(kMagicSeededCt, p);
      if (h.n != want.n || h.N != want.N || h.k != want.k || h.l != want.l || h.Bgbit != want.Bgbit || h.ks_t != want.ks_t ||
          h.ks_basebit != want.ks_basebit) {
        fprintf(stderr, "redsec tfhe shim: seeded ciphertexts of n=%d N=%d l=%d Bgbit=%d t=%d basebit=%d do not fit the key's parameters\n",
                h.n, h.N, h.l, h.Bgbit, h.ks_t, h.ks_basebit);
        abort();
      }
      uint8_t seed[32];
      uint64_t first = 0;
      read_exact(f, seed, sizeof seed, "mask seed");
      read_exact(f, &first, sizeof first, "first row");
      st = &ct_files(true)[f];
      file_id(f, &st->dev, &st->ino);
      rs::kg_seed_words(seed, st->key);
      st->next_row = first;
    } else {
      if ((int32_t)word != kLweSampleTypeUid) {
        fprintf(stderr, "redsec tfhe shim: not an LweSample record (type uid %d, expected 42) nor an RSC1 file\n", (int32_t)word);
        abort();
      }
      read_exact(f, s->a, sizeof(Torus32) * (size_t)n, "ciphertext a");
      read_exact(f, &s->b, sizeof(Torus32), "ciphertext b");
      read_exact(f, &s->current_variance, sizeof(double), "ciphertext variance");
      return;
    }
  }
  read_exact(f, &s->b, sizeof(Torus32), "ciphertext body");
  const uint64_t row = st->next_row;
  for (int32_t blk = 0; 16 * blk < n; ++blk) {
    uint32_t words[16];
    rs::kg_ct_mask_block(st->key, row, blk, words);
    for (int32_t q = 0; q < 16 && 16 * blk + q < n; ++q) s->a[16 * blk + q] = (Torus32)words[q];
  }
  s->current_variance = 0.;
  st->next_row = row + 1;
  st->pos = ftell(f);
}

// ---- GPU ----
rs_ctx* redsec_ctx_of(const TFheGateBootstrappingCloudKeySet* bk) { return ctx_of_fft(bk->bkFFT); }
rs_ctx** redsec_fleet_of(const TFheGateBootstrappingCloudKeySet* bk, int* count) {
  (void)ctx_of_fft(bk->bkFFT);
  *count = bk->bkFFT->fleet_size;
  return bk->bkFFT->fleet;
}
void redsec_pack(int32_t* words, const LweSample* s, int32_t n) {
  memcpy(words, s->a, sizeof(int32_t) * (size_t)n);
  words[n] = s->b;
}
void redsec_unpack(LweSample* s, const int32_t* words, int32_t n) {
  memcpy(s->a, words, sizeof(int32_t) * (size_t)n);
  s->b = words[n];
  s->current_variance = 0.;
}

void tfhe_bootstrap_FFT(LweSample* result, const LweBootstrappingKeyFFT* bkfft, Torus32 mu, const LweSample* x) {
  const int32_t n = bkfft->in_out_params->n;
  std::vector<int32_t> in(n + 1), out(n + 1);
  redsec_pack(in.data(), x, n);
  if (rs_bootstrap(ctx_of_fft(bkfft), out.data(), in.data(), mu, 1) != 0) die("rs_bootstrap");
  redsec_unpack(result, out.data(), n);
}

void bootsSymEncrypt(LweSample* r, int32_t message, const TFheGateBootstrappingSecretKeySet* key) {
  const Torus32 e8 = modSwitchToTorus32(1, 8);
  lweSymEncrypt(r, message ? e8 : -e8, key->params->in_out_params->alpha_min, key->lwe_key);
}
int32_t bootsSymDecrypt(const LweSample* s, const TFheGateBootstrappingSecretKeySet* key) { return lwePhase(s, key->lwe_key) > 0; }
void bootsCONSTANT(LweSample* r, int32_t value, const TFheGateBootstrappingCloudKeySet* bk) {
  const Torus32 e8 = modSwitchToTorus32(1, 8);
  lweNoiselessTrivial(r, value ? e8 : -e8, bk->params->in_out_params);
}
void bootsNOT(LweSample* r, const LweSample* ca, const TFheGateBootstrappingCloudKeySet* bk) { lweNegate(r, ca, bk->params->in_out_params); }
void bootsCOPY(LweSample* r, const LweSample* ca, const TFheGateBootstrappingCloudKeySet* bk) { lweCopy(r, ca, bk->params->in_out_params); }
void bootsNAND(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_NAND, r, a, b, bk); }
void bootsOR(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_OR, r, a, b, bk); }
void bootsAND(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_AND, r, a, b, bk); }
void bootsXOR(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_XOR, r, a, b, bk); }
void bootsXNOR(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_XNOR, r, a, b, bk); }
void bootsNOR(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_NOR, r, a, b, bk); }
void bootsANDNY(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_ANDNY, r, a, b, bk); }
void bootsANDYN(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_ANDYN, r, a, b, bk); }
void bootsORNY(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_ORNY, r, a, b, bk); }
void bootsORYN(LweSample* r, const LweSample* a, const LweSample* b, const TFheGateBootstrappingCloudKeySet* bk) { gate(RS_ORYN, r, a, b, bk); }
void bootsMUX(LweSample* r, const LweSample* a, const LweSample* b, const LweSample* c, const TFheGateBootstrappingCloudKeySet* bk) {
  const int32_t n = bk->params->in_out_params->n;
  std::vector<int32_t> x(n + 1), y(n + 1), z(n + 1), o(n + 1);
  redsec_pack(x.data(), a, n); redsec_pack(y.data(), b, n); redsec_pack(z.data(), c, n);
  if (rs_mux(redsec_ctx_of(bk), o.data(), x.data(), y.data(), z.data(), 1) != 0) die("rs_mux");
  redsec_unpack(r, o.data(), n);
}
