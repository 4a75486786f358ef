/*
 * redsec_hip.h -- C ABI of the MI355X gate-bootstrapping backend (libredsec_hip.so).
 *
 * This is the drop-in boundary for REDsec's encrypted hot path. Each entry point replaces a call
 * that the reference makes into the external TFHE library (paths relative to /root/reference):
 *
 *   rs_bootstrap / rs_bootstrap_dev     tfhe_bootstrap_FFT             lib/BinOps_enc.cpp:185,191
 *                                       (Quantize::execute loops       lib/BinFunc.cpp:1056-1071,
 *                                                                       lib/IntFunc.cpp:871-887)
 *   rs_gate / rs_gate_dev               bootsAND/OR/XOR/...            lib/BinOps_enc.cpp:49-52,104-113,
 *                                                                       153-166,205; lib/IntOps_enc.cpp:63
 *   rs_mux / rs_mux_dev                 bootsMUX                       lib/IntFunc.cpp:962
 *   rs_lincomb_dev, rs_linear_*         lweAddTo/lweSubTo/lweAddMulTo/ lib/BinFunc.cpp:195-320,
 *                                       lweNoiselessTrivial loops      lib/IntFunc.cpp:207-308,643-700
 *   rs_create / rs_load_keys            new_tfheGateBootstrappingCloudKeySet_fromFile + the
 *                                       bkFFT precomputation           nets/mnist/sign1024x1/net.cpp:53-55
 *
 * Plain pointers and sizes only. "_dev" entry points take DEVICE pointers (hipMalloc / torch CUDA
 * tensors) and enqueue on the given hipStream_t (passed as void*; NULL = default stream) without
 * synchronising; the others take HOST pointers and are synchronous.
 *
 * Ciphertext layout: an LWE sample of dimension n is W = n+1 consecutive int32 words
 * (a[0..n-1], b); a batch is int32[B][W], row-major, contiguous. Torus32 arithmetic wraps mod 2^32.
 *
 * Errors: every function returns 0 on success or a negative rs_status; rs_last_error() gives the
 * message for the calling thread. There is NO CPU fallback: without a HIP device every compute
 * entry point fails with RS_ERR_NO_DEVICE.
 */
#ifndef REDSEC_HIP_H
#define REDSEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rs_status {
  RS_OK = 0,
  RS_ERR_INVALID = -1,     /* bad argument / unsupported parameter set */
  RS_ERR_NO_DEVICE = -2,   /* no HIP device or device is not gfx950-compatible */
  RS_ERR_HIP = -3,         /* a HIP runtime call failed */
  RS_ERR_STATE = -4,       /* keys not loaded, etc. */
  RS_ERR_INEXACT = -5      /* RS_MODE_FFT_SPLIT: the enforced rounding certificate failed (see rs_split_bound); sticky until
                              rs_certify(..., reset = 1). The check of call k on a stream is looked at by call k + 1 on that
                              stream, rs_sync, rs_certify, rs_release_stream, rs_destroy and every host-pointer call -- NOT by
                              the *_dev call itself (it is asynchronous): a device-pointer caller must pass one of those
                              before trusting the LAST call's output (rs_destroy returns the error too) */
} rs_status;

/* Mirrors TFheGateBootstrappingParameterSet (ks_t, ks_basebit, in_out_params->n, tgsw_params->l,
 * Bgbit, tlwe_params->N, k) as constructed at client/gen_secure_keyset.cpp:82-90. */
typedef struct rs_params {
  int32_t n;          /* LWE dimension */
  int32_t N;          /* ring degree: 1024, 2048, 4096 or 8192 */
  int32_t k;          /* must be 1 */
  int32_t bk_l;       /* gadget length l and base 2^Bgbit, l * Bgbit <= 32. N = 1024 with 3/7 or 10/3 (the shipped sets) */
  int32_t bk_Bgbit;   /* has all three modes below; every other set runs in RS_MODE_FFT_SPLIT only */
  int32_t ks_t;
  int32_t ks_basebit;
} rs_params;

typedef struct rs_ctx rs_ctx;

typedef enum rs_gate_op {
  RS_NAND = 0, RS_OR = 1, RS_AND = 2, RS_NOR = 3, RS_XOR = 4, RS_XNOR = 5,
  RS_ANDNY = 6, RS_ANDYN = 7, RS_ORNY = 8, RS_ORYN = 9
} rs_gate_op;

const char* rs_last_error(void);
const char* rs_version(void);

/* Parameter sets shipped with the reference / TFHE. */
int rs_params_default128(rs_params* p);        /* TFHE default 128-bit set (NAND microbench) */
int rs_params_redsec_small_v2(rs_params* p);   /* client/gen_secure_keyset.cpp:70-91 (the set the client ships with) */
int rs_params_redsec_small(rs_params* p);      /* client/gen_secure_keyset.cpp:47-68:  n=500  N=1024 l=3 Bgbit=10 */
int rs_params_redsec_medium(rs_params* p);     /* client/gen_secure_keyset.cpp:28-45:  n=3072 N=4096 l=3 Bgbit=10 */
int rs_params_redsec_large(rs_params* p);      /* client/gen_secure_keyset.cpp:9-26:   n=6144 N=8192 l=3 Bgbit=10 */

/* Context bound to one HIP device (device index as in hipSetDevice). */
int rs_create(rs_ctx** out, const rs_params* p, int device);
int rs_destroy(rs_ctx* ctx);

/* Upload the evaluation key (HOST pointers):
 *   bk  int32[n][(k+1)*l][k+1][N]   TGSW rows, row p = c*l + j (bk->bk[i].all_sample[p].a[col])
 *   ksk int32[k*N][t][1<<basebit][n+1]   bk->ks->ks[i][j][v] as (a[0..n-1], b)
 * Transforms bk to the transform domain on the device (the bkFFT analogue). */
int rs_load_keys(rs_ctx* ctx, const int32_t* bk, const int32_t* ksk);
/* The same with a SYNTHETIC key generated on the device: bk word k = high half of splitmix64(seed + k) (csrc/rs_ntt.h,
 * synthetic_key_word; redsec_amd/client.py restates it in numpy), ksk word k likewise from seed ^ 0x6b73. Not an encryption of
 * anything: for benchmarks and parity tests of the large rings, whose real keys are gigabytes on the host (redsec_params_large:
 * 2.4 GB of bk + 7.2 GB of ksk) -- every kernel does exactly the work it does on a real key, and the oracle is fed the same words. */
int rs_load_synthetic_keys(rs_ctx* ctx, uint64_t seed);

/* Evaluation key of this context's parameter set, generated on the device (CLIENT-side operation; INTEGRATION.md, "Key generation").
 * lwe_key int32[n], tlwe_key int32[N]: HOST, values 0/1. bk, ksk: DEVICE, layouts of rs_load_keys (bk 16-byte aligned).
 * seed: 32 bytes (ChaCha20 key). bk_stdev / ks_stdev: TFHE alpha in torus units (0 = noiseless, tests only).
 * Synchronous. The secret key is copied to a private device buffer that is zeroed and freed before the call returns; the
 * context's loaded key is not touched. RS_ERR_INVALID for null pointers, key words outside {0, 1}, negative or non-finite
 * deviations; RS_ERR_INEXACT if a rounding distance of the a*S products reaches 1/4 (never expected).
 *
 * Every key word is a function of (seed, lwe_key, tlwe_key, deviations), regenerated by redsec_amd/keygen.py:
 * Stream (domain, row): word w is word w & 15 of the ChaCha20 block (RFC 8439 section 2.3) with key = the seed as 8
 * little-endian words, word 12 = block counter w >> 4, words 13, 14, 15 = domain, row & 0xffffffff, row >> 32.
 *   domain 1 LWE secret    row 0                          s_i = word i & 1 (i < n)        [redsec_amd/keygen.py secret_keys]
 *   domain 2 TRLWE secret  row 0                          S_j = word j & 1 (j < N)
 *   domain 3 bk mask       row i 2l + p                   the N mask coefficients of TGSW row p = c l + j of s_i
 *   domain 4 bk noise      row i 2l + p                   the N Gaussians of that row
 *   domain 5 ksk mask      row (i t + j) 2^basebit + v    the n mask words of that sample
 *   domain 6 ksk noise     same row                       1 Gaussian
 * Gaussian g of a row uses words 4g .. 4g+3: u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) 2^-53 in (0, 1], u2 = ((w2 >> 5) 2^26 + (w3 >> 6))
 * 2^-53 in [0, 1), z = sqrt(-2 ln u1) cos(2 pi u2); the noise word is TFHE's dtot32(stdev z): the fractional part (truncated) times
 * 2^32, converted to int64, wrapped to 32 bits.
 * bk row p = c l + j of key bit s_i is (a, b) with a the domain-3 mask and b = a*S + e (mod 2^32, negacyclic); then coefficient 0 of
 * component c gains s_i 2^(32 - (j+1) Bgbit) (for c = 0: a[0] changes after b was formed).
 * ksk samples with v = 0 are all zero; v >= 1: a = the domain-5 words, b = sum_k a_k s_k + e + ((S_i v) << (32 - (j+1) basebit)). */
int rs_keygen_dev(rs_ctx* ctx, int32_t* bk, int32_t* ksk, const int32_t* lwe_key, const int32_t* tlwe_key,
                  const uint8_t* seed, double bk_stdev, double ks_stdev);
/* rs_load_keys with DEVICE pointers (no host round trip; the inputs are not modified). */
int rs_load_keys_dev(rs_ctx* ctx, const int32_t* bk, const int32_t* ksk);

/* Compressed evaluation key: a public 32-byte MASK SEED plus the bodies, 1/8 to 1/6 of the bytes of the
 * full key. It is another encryption of the same key, with the gadget term of c = 0 rows moved out of the public mask:
 *   bk row p = c l + j of key bit s_i (row i 2l + p):  a = the domain-3 stream of the mask seed (stored unchanged),
 *     b = a*S + e + s_i g_j X^0 (c = 1),  b = a*S + e - s_i g_j S (c = 0),  g_j = 2^(32 - (j+1) Bgbit),  e = domain 4 of the noise seed.
 *     Its phase is that of the rs_keygen_dev row; their difference is -s_i g_j (1, S) for c = 0, an exact encryption of zero.
 *   ksk sample s = (i t + j) 2^basebit + v:  a = the domain-5 stream of the mask seed, b as in rs_keygen_dev with e = domain 6 of
 *     the noise seed; samples with v = 0 are all zero (their body word is 0 and is ignored).
 * The NOISE SEED (domains 1, 2, 4, 6) stays private; equal seeds would publish the noise, hence the secret, and are refused.
 * Layouts: bk_body int32[n][2l][N], ksk_body int32[N][t][2^basebit], mask_seed 32 bytes.
 *
 * rs_keygen_compressed_dev: the bodies, generated on the device under rs_keygen_dev's contract (CLIENT side): lwe_key / tlwe_key
 * HOST, bk_body / ksk_body DEVICE (bk_body 16-byte aligned); RS_ERR_INVALID as rs_keygen_dev and for equal seeds; RS_ERR_INEXACT
 * as rs_keygen_dev. The secret's device copy is zeroed and freed on every path. Needs the split-key product.
 * rs_expand_keys_dev: the full key (layouts of rs_load_keys) from the mask seed and the bodies; every pointer DEVICE, bk 16-byte
 * aligned. Needs no product: works on every context. Synchronous.
 * rs_load_compressed_keys (HOST bodies) / rs_load_compressed_keys_dev (DEVICE bodies): rs_load_keys of the expanded key (SERVER
 * side); the expansion happens on the device, the full key never exists on the host. A failed load, invalid arguments included,
 * leaves the context with no key. */
int rs_keygen_compressed_dev(rs_ctx* ctx, int32_t* bk_body, int32_t* ksk_body, const int32_t* lwe_key, const int32_t* tlwe_key,
                             const uint8_t* mask_seed, const uint8_t* noise_seed, double bk_stdev, double ks_stdev);
int rs_expand_keys_dev(rs_ctx* ctx, int32_t* bk, int32_t* ksk, const uint8_t* mask_seed, const int32_t* bk_body, const int32_t* ksk_body);
int rs_load_compressed_keys(rs_ctx* ctx, const uint8_t* mask_seed, const int32_t* bk_body, const int32_t* ksk_body);
int rs_load_compressed_keys_dev(rs_ctx* ctx, const uint8_t* mask_seed, const int32_t* bk_body, const int32_t* ksk_body);

/* Seeded LWE ciphertexts: a batch travels as a public 32-byte MASK SEED, a uint64 `first` and one body
 * word per sample, 4 bytes instead of 4 (n + 1). Streams as for rs_keygen_dev, two more domains:
 *   domain 7 ciphertext mask   row first + i   the n mask words of ciphertext i of the call (mask seed)
 *   domain 8 ciphertext noise  same row        1 Gaussian, words 0-3 (noise seed)
 * Ciphertext i: a_k = word k of stream (7, first + i) of the mask seed; e = dtot32(stdev z) of Gaussian 0 of stream (8, first + i)
 * of the noise seed, as in rs_keygen_dev; body = sum_k a_k s_k + e + mu_i (mod 2^32). The expanded sample is the usual
 * int32[B][n+1], the body at word n. Domains 7 and 8 are disjoint from 1-6: one seed may serve a compressed key and ciphertexts.
 * Rules:
 *   - the NOISE SEED is private; equal mask and noise seeds would publish the noise and are refused;
 *   - first + B must not pass 2^64 (the last row is at most 2^64 - 1);
 *   - a (mask seed, row) pair must never encrypt two messages: equal masks publish the difference of the messages up to noise.
 *     redsec_amd's default is a fresh random mask seed per call.
 * Both return RS_ERR_INVALID for null pointers, key words outside {0, 1}, a negative or non-finite stdev, equal seeds and first + B
 * passing 2^64; B = 0 is a no-op that returns RS_OK. There is no CPU fallback: without a device they fail with RS_ERR_NO_DEVICE.
 *
 * CLIENT side. Synchronous. lwe_key HOST int32[n], 0/1. mu DEVICE int32[B] (torus words). body DEVICE int32[B].
 * ct DEVICE int32[B][n+1], or NULL for bodies only. The secret's private device copy is zeroed and freed on every path. */
int rs_encrypt_seeded_dev(rs_ctx* ctx, int32_t* body, int32_t* ct, const int32_t* mu, size_t B, const int32_t* lwe_key,
                          const uint8_t* mask_seed, const uint8_t* noise_seed, uint64_t first, double stdev);
/* SERVER side. Ordered on `stream`, like the other *_dev calls; needs no loaded key. ct, body DEVICE. */
int rs_expand_ciphertexts_dev(rs_ctx* ctx, int32_t* ct, const uint8_t* mask_seed, uint64_t first, const int32_t* body,
                              size_t B, void* stream);

/* Public-key encryption (no reference counterpart: TFHE has no public key). A party WITHOUT the secret
 * encrypts under a Regev public key: m encryptions of zero, canonically rs_expand_ciphertexts_dev of an rs_encrypt_seeded_dev(mu = 0,
 * B = m) batch, so a public key travels as a seeded-ciphertext batch (32-byte mask seed + m body words). Each output is the sum of a
 * secret random subset of the rows; with `base` the same call re-randomises ciphertexts. One more stream, disjoint from domains 1-8:
 *   domain 9   selection bits   row first + i   bit j of ciphertext i = (word (j >> 5) of the stream >> (j & 31)) & 1,  j < m
 *   ct[i] = (base ? base[i] : 0) + (0, mu ? mu[i] : 0) + sum over j with bit j set of pk[j]      (word-wise mod 2^32)
 * pk DEVICE int32[m][n+1]; mu DEVICE int32[B] or NULL; base DEVICE int32[B][n+1] or NULL; ct DEVICE int32[B][n+1]. ct may equal base
 * (re-randomisation in place); any other overlap is the caller's error. rand_seed: HOST, 32 bytes, the encryptor's PRIVATE randomness
 * (the ChaCha key of domain 9), read before the call returns; it reaches the device as a kernel argument, the selection bits exist
 * only in registers and LDS, and nothing secret outlives the call. Needs no loaded key. Asynchronous and ordered on `stream`, like
 * rs_expand_ciphertexts_dev. B = 0 is a no-op that returns RS_OK.
 * Rule: a (rand seed, row) pair must never be used twice -- two outputs with the same selection differ by exactly their messages (and
 * bases). redsec_amd's default is a fresh random rand seed per call.
 * Noise of an output: about alpha sqrt(m / 2) for rows of deviation alpha (m / 2 rows are added on average). Security rests on LWE at
 * the rows' alpha and on the leftover hash lemma over m (redsec_amd's default m = 32 (n + 1) + 256 = n log q + 2 lambda); nothing more
 * is claimed.
 * RS_ERR_INVALID: a null ct, pk or rand_seed; m outside 1 .. 2^31 - 1; first + B passing 2^64; B or m whose row arithmetic would
 * overflow. Without a device or context it fails as rs_expand_ciphertexts_dev does. */
int rs_pk_encrypt_dev(rs_ctx* ctx, int32_t* ct, const int32_t* pk, size_t m, const int32_t* mu, const int32_t* base,
                      size_t B, const uint8_t* rand_seed, uint64_t first, void* stream);

/* Compact RLWE public keys (no reference counterpart). The Regev key above costs 32 (n + 1) + 256 rows and
 * gives outputs of noise alpha sqrt(m / 2), too much for the 1/4096-scale inputs of the networks. An RLWE public key is ONE ring sample
 * (a, b = a*S + e) under the ring secret S, negacyclic mod 2^32: a 32-byte mask seed plus the N body words (4 KB at N = 1024). A party
 * WITHOUT the secret encrypts N messages per ciphertext, (a*u + e1, b*u + e2 + m) with u uniform binary, of phase error e*u + e2 - e1*S:
 * deviation alpha sqrt(N + 1). The server extracts one LWE sample per coefficient and keyswitches it with the key it has loaded.
 * Four more streams, disjoint from domains 1-9 (Gaussians as everywhere: Gaussian g from words 4g .. 4g+3, kg_noise32):
 *   domain 10  public-key mask    row 0          mask seed (public)          a_k = word k, k < N
 *   domain 11  public-key noise   row 0          owner's noise seed (private) e_k = Gaussian k, k < N
 *   domain 12  selector u         row first + r  rand seed (private)         u_k = (word (k >> 5) >> (k & 31)) & 1, k < N
 *   domain 13  encryption noise   row first + r  rand seed                   Gaussians 0 .. N-1 are e1, N .. 2N-1 are e2
 * Key generation (domains 10, 11) is the owner's and has no device code (redsec_amd/keygen.py rlwe_public_key).
 *
 * rs_rlwe_pk_encrypt_dev: R = ceil(count / N) ciphertexts, N the context's ring; ciphertext r has row first + r and carries messages
 * mu[rN] .. mu[rN + N - 1] in its coefficients, slots at or past count carry 0:
 *   rlwe[r][0] = a*u_r + e1,   rlwe[r][1] = b*u_r + e2 + m_r      (negacyclic, word-wise mod 2^32)
 * rlwe DEVICE int32[R][2][N]; pk DEVICE int32[2][N] (a, then b); mu DEVICE int32[count] torus words. rand_seed: HOST, 32 bytes, the
 * encryptor's PRIVATE randomness, read before the call returns (its host copy is cleared); u exists only in registers and LDS.
 * stdev: deviation of e1 and e2, any finite value >= 0 (0 is for word-identity tests; policy lives in redsec_amd). Needs no loaded
 * key. Asynchronous and ordered on `stream`. count = 0 is a no-op that returns RS_OK.
 * Rule: a (rand seed, row) pair must never be used twice. Security rests on RLWE at the key's alpha with a binary ephemeral secret;
 * nothing more is claimed (no circuit privacy, no CCA security).
 * RS_ERR_INVALID: a null rlwe, pk, mu or rand_seed; a negative or non-finite stdev; first + R passing 2^64; a count whose row
 * arithmetic would overflow. Without a device or context it fails as rs_pk_encrypt_dev does. */
int rs_rlwe_pk_encrypt_dev(rs_ctx* ctx, int32_t* rlwe, const int32_t* pk, const int32_t* mu, size_t count, const uint8_t* rand_seed,
                           uint64_t first, double stdev, void* stream);

/* rs_rlwe_extract_dev: sample i = rN + c of u is the extraction of coefficient c of ciphertext r, in the convention of
 * rs_bootstrap_wo_ks_dev's output, so that rs_keyswitch_dev and rs_phase_dev(dim = N) apply unchanged:
 *   word j = rlwe[r][0][c - j] for j <= c,   word j = -rlwe[r][0][N + c - j] for c < j < N,   word N = rlwe[r][1][c]
 * u DEVICE int32[count][N+1]; rlwe DEVICE int32[ceil(count / N)][2][N]; u must not overlap rlwe. Needs no key. Asynchronous and
 * ordered on `stream`. count = 0 is a no-op. RS_ERR_INVALID: a null u or rlwe; a count whose row arithmetic would overflow. */
int rs_rlwe_extract_dev(rs_ctx* ctx, int32_t* u, const int32_t* rlwe, size_t count, void* stream);

/* Packed results (TFHE's TLWE keyswitch with the identity function): a public keyswitch from the LWE key s
 * to the ring key S that puts up to N LWE samples into the coefficients of ONE RLWE ciphertext of section 17's format, 8N bytes
 * instead of N 4 (n + 1). The packing key holds, per key bit s_i and digit j, a ring sample under S whose message is s_i times the
 * digit's weight; two more streams, disjoint from domains 1-13 (owner's side only: redsec_amd/keygen.py pack_key, rs_pack_keygen_dev):
 *   domain 14  packing-key mask    row i t + j   mask seed (public)             a_ij[k] = word k, k < N
 *   domain 15  packing-key noise   row i t + j   owner's noise seed (private)   e_ij[k] = Gaussian k (words 4k .. 4k+3, kg_noise32)
 *
 * rs_pack_dev: R = ceil(count / N) ciphertexts, N and n the context's; ciphertext r packs samples rN .. rN + count_r - 1 into
 * coefficients 0 .. count_r - 1, count_r = min(N, count - rN). Word-wise mod 2^32, negacyclic products, the digit convention of
 * lweKeySwitch / rs_keyswitch_dev:
 *   K[i][j]   = (a_ij, b_ij = a_ij*S + e_ij + s_i 2^(32-(j+1) basebit) X^0)        i < n, j < t
 *   abar      = a + off,  off = 2^(31 - t basebit)  (0 when t basebit = 32)
 *   D_ij(X)   = sum over c < count_r of ((abar_i of sample rN+c) >> (32-(j+1) basebit) & (2^basebit - 1)) X^c
 *   rlwe[r]   = (0, sum_c b_(rN+c) X^c) - sum_{i,j} D_ij(X) K[i][j]
 * Under S, coefficient c of the result has phase (b - a*S) equal to the phase of sample rN + c plus the packing error, of variance
 *   sigma^2 = n t count_r (2^basebit - 1)(2^(basebit+1) - 1)/6 sigma_k^2  +  (n/2) 2^(-2 t basebit)/12
 * (sigma_k the key's deviation; the first term is the key noise under the digits, the second the digits' rounding). Slots at or
 * past count hold noise around 0. rs_rlwe_extract_dev + rs_keyswitch_dev turn a packed ciphertext back into LWE inputs, and
 * rs_rlwe_extract_dev + rs_phase_dev(dim = N) decrypt it on the device.
 * ct DEVICE int32[count][n+1]; rlwe DEVICE int32[R][2][N]; pack_key DEVICE int32[n][t][2][N]. The kernels add into rlwe with
 * atomics after an init kernel has set it: an rlwe that overlaps ct or pack_key is refused (the inputs may overlap each other). Integer
 * arithmetic only, exact: the words do not depend on how the work is tiled. Needs no loaded key. Asynchronous and ordered on
 * `stream`; no allocation. count = 0 is a no-op that returns RS_OK.
 * RS_ERR_INVALID: a null rlwe, ct or pack_key; basebit outside 1 .. 8; t < 1; t basebit > 32; a count whose row arithmetic would
 * overflow; an rlwe that shares a byte with ct or pack_key ("rlwe overlaps ct"). Without a device or context it fails as
 * rs_rlwe_extract_dev does. */
int rs_pack_dev(rs_ctx* ctx, int32_t* rlwe, const int32_t* ct, size_t count,
                const int32_t* pack_key, int32_t basebit, int32_t t, void* stream);

/* Re-keying: a public LWE-to-LWE keyswitch under a caller-supplied key, from any source dimension to
 * any destination dimension. Results encrypted under a key s leave the server decryptable under another key s': delegation to a
 * third party, key rotation, or crossing from one parameter set to another (n = 350 to n = 630 and back). rs_keyswitch_dev reads
 * only the context's loaded key in TFHE's table layout; this call reads the key it is given, in the digit-times-row form of
 * rs_pack_dev. Word-wise mod 2^32, the digit convention of lweKeySwitch / rs_keyswitch_dev / rs_pack_dev:
 *   K[i][j]  = row i t + j of rekey_key = (a_ij, b_ij),  b_ij = <a_ij, s'> + e_ij + s_i 2^(32-(j+1) basebit)     i < n_src, j < t
 *   abar     = a + off,  off = 2^(31 - t basebit)  (0 when t basebit = 32)
 *   d_ij(r)  = (abar_i of sample r >> (32-(j+1) basebit)) & (2^basebit - 1)
 *   out[r]   = (0, b_r) - sum_{i,j} d_ij(r) K[i][j]
 * Under s', out[r] has the phase of ct[r] under s plus the re-keying error, of variance
 *   sigma^2 = n_src t (2^basebit - 1)(2^(basebit+1) - 1)/6 sigma_row^2  +  (n_src/2) 2^(-2 t basebit)/12
 * (sigma_row the deviation of one key row's phase; the first term is the key noise under the digits, the second the digits'
 * rounding). The key needs no call of its own: it is n_src t seeded encryptions of the words s_i 2^(32-(j+1) basebit) under the
 * recipient's LWE key (rs_encrypt_seeded_dev, expanded by rs_expand_ciphertexts_dev on a context with n = n_dst), or, without the
 * recipient's secret, ceil(n_src t / N) ciphertexts of those words under the recipient's compact RLWE public key
 * (rs_rlwe_pk_encrypt_dev) turned into rows by rs_rlwe_extract_dev: then n_dst = N and the destination is the recipient's ring
 * key read as an LWE key, under which rs_phase_dev(dim = N) decrypts. The rows of one such ciphertext share its selector and
 * noise polynomials, so their noise has a common part that the unsigned digits would add up; redsec_amd encrypts every odd row
 * negated and negates it back after the extraction (keygen.py rekey_alternate), and the formula above then holds for this form.
 * ct DEVICE int32[B][n_src+1]; rekey_key DEVICE int32[n_src][t][n_dst+1]; out DEVICE int32[B][n_dst+1]; an out that overlaps
 * ct or rekey_key is refused (the kernels add into out with atomics; the inputs may overlap each other). Both dimensions are arguments, not the context's: a server context of any set re-keys to any recipient. Integer arithmetic
 * only, exact: the words do not depend on how the work is tiled. Needs no loaded key. Asynchronous and ordered on `stream`; no
 * allocation. B = 0 is a no-op that returns RS_OK. A second call into the same buffer gives the same words.
 * RS_ERR_INVALID: a null out, ct or rekey_key; n_src or n_dst outside 1 .. 65536; basebit outside 1 .. 8; t < 1; t basebit > 32; a
 * B whose row arithmetic would overflow or whose grid passes one launch; an out that shares a byte with ct or rekey_key ("out
 * overlaps ct"). Without a device or context it fails as rs_pack_dev does. */
int rs_rekey_dev(rs_ctx* ctx, int32_t* out, const int32_t* ct, size_t B, int32_t n_src,
                 const int32_t* rekey_key, int32_t n_dst, int32_t basebit, int32_t t, void* stream);

/* Ring re-keying: a public RLWE-to-RLWE keyswitch under a caller-supplied key of t + 1 ring samples.
 * Packed ciphertexts (rs_pack_dev, rs_rlwe_pk_encrypt_dev) under a ring key S leave the server decryptable under another ring key
 * S' of the same degree: packed replies for a third party, or key rotation of packed ciphertexts that lie in storage, with one
 * keyswitch error and no detour through LWE samples. Word-wise mod 2^32 with negacyclic products:
 *   K[j]     = row j of ring_key = (a_j, b_j),  b_j - a_j*S' = e_j + h_j S,  h_j = 2^(31-(j+1) basebit)                j < t
 *   K[t]     = (a_t, b_t),  b_t - a_t*S' = e_t + c0 (1 + X + ... + X^(N-1)) S,  c0 = (2^basebit - 1) sum_j h_j
 *   abar_k   = a_k + off,  off = 2^(31 - t basebit)
 *   d_j(k)   = 2 ((abar_k >> (32-(j+1) basebit)) & (2^basebit - 1)) - (2^basebit - 1)        odd, symmetric about zero
 *   D_j(X)   = sum_k d_j(k) X^k
 *   out[r]   = (0, b_r) - K[t] - sum_{j<t} D_j(X) K[j]
 * Under S', out[r] has the phase of rlwe[r] under S plus the re-keying error, per coefficient of variance
 *   sigma^2 = (t N (4^basebit - 1)/3 + 1) sigma_row^2  +  (N/2) 2^(-2 t basebit)/12
 * (sigma_row the deviation of one key row's phase per coefficient; an odd digit has mean square (4^basebit - 1)/3; the second
 * term is the rounding of abar to t basebit bits). The digits are centred, not the unsigned ones of rs_pack_dev / rs_rekey_dev,
 * and the constant row K[t] carries what the centring took away: rows made from one RLWE public key share that key's noise, and
 * a digit polynomial with a mean would add the common part up along the coefficients (16 .. 22 times the formula with unsigned
 * digits; section 22 has the comparison). The key needs no call of its own: t + 1 seeded ring samples under S', or, without the
 * recipient's secret, the t + 1 ciphertexts of rs_rlwe_pk_encrypt_dev over the message rows under the recipient's RLWE public key.
 * rlwe, out DEVICE int32[R][2][N]; ring_key DEVICE int32[t+1][2][N]; an out that overlaps rlwe or ring_key is refused (the
 * kernels add into out with atomics: re-keying in place is not offered; the inputs may overlap each other). N is the context's ring; source
 * and destination share it (crossing between rings of different degree is out of scope). Integer arithmetic only, exact: the
 * words do not depend on how the work is tiled. Needs no loaded key. Asynchronous and ordered on `stream`; no allocation. R = 0 is
 * a no-op that returns RS_OK. A second call into the same buffer gives the same words.
 * RS_ERR_INVALID: a null out, rlwe or ring_key; basebit outside 1 .. 8; t < 1; t basebit > 31 (h_j is an integer); an R whose row
 * arithmetic would overflow or whose grid passes one launch; an out that shares a byte with rlwe or ring_key ("out overlaps
 * rlwe"). Without a device or context it fails as rs_pack_dev does. */
int rs_ring_rekey_dev(rs_ctx* ctx, int32_t* out, const int32_t* rlwe, size_t R,
                      const int32_t* ring_key, int32_t basebit, int32_t t, void* stream);

/* Encrypted selection: the levelled mode on packed ciphertexts. rs_ring_cmux_dev is the CMUX built on
 * the external product RLWE x RGSW: out[r] takes the phase of d1[r] where the selector encrypts 1 and of d0[r] where it encrypts 0,
 * and the server learns nothing of the bit. rs_ring_lookup_dev is the CMUX tree: out = table[index] for an index whose bits arrive
 * as `depth` selectors and which the server never sees. Ciphertexts are int32[2][N] = (a, b) with phase b - a*S, as rs_pack_dev and
 * rs_rlwe_pk_encrypt_dev make them and rs_ring_rekey_dev takes them; a plaintext row p is the trivial ciphertext (0, p).
 * sel DEVICE int32[2l][2][N]: one RGSW sample of a bit m under the context ring's key S. Rows j < l are ring samples of zero with
 * m h_j added to a, rows l + j have m h_j added to b, h_j = 2^(32-(j+1) basebit): the samples a bootstrapping key consists of, made
 * by the client (client.SecretKeySet.ring_selector). Word-wise mod 2^32 with negacyclic products and the signed digits of TFHE's
 * tGswTorus32PolynomialDecompH:
 *   B = 2^basebit,  off = sum_j (B/2) h_j + 2^(31 - l basebit)
 *   x = d1[r] - d0[r]                      (x = -d0[r] when d1 == NULL: an all-zero d1)
 *   u_j(w)   = ((w + off) >> (32 - (j+1) basebit)) & (B - 1),   dig_j(w) = u_j(w) - B/2
 *   Da_j(X)  = sum_k dig_j(x.a_k) X^k,   Db_j(X) = sum_k dig_j(x.b_k) X^k
 *   out[r]   = d0[r] + sum_{j<l} Da_j(X) sel[j] + sum_{j<l} Db_j(X) sel[l+j]
 * phase(out) = phase(d0) + m (phase(d1) - phase(d0)) + noise, per coefficient and CMUX of variance
 *   sigma^2 = 2 l N (B^2 + 2)/12 sigma_row^2  +  (1 + N/2) 2^(-2 l basebit)/12
 * (sigma_row the deviation of one selector row's phase per coefficient; a signed digit has mean square (B^2 + 2)/12; the second
 * term is the rounding of x to l basebit bits, present where m = 1). A lookup adds `depth` of them.
 * d0[r] and d1[r] are read at row r stride (int32[2][N] each; stride >= 1, 2 for the even and odd entries of a table); out DEVICE
 * int32[R][2][N], contiguous. The first kernel sets out = d0 and the second adds into it with atomics, so a second call into the
 * same buffer gives the same words and an out that overlaps an input is refused: the ((R - 1) stride + 1) ciphertexts that d0 and
 * d1 are read from, or sel (out = d0 is not offered; d0, d1 and sel may overlap each other, as table[1:] / table do at stride 2). N is the context's ring. Integer arithmetic only, exact: the words do not depend on how the work is tiled. Needs no
 * loaded key. Asynchronous and ordered on `stream`; no allocation. R = 0 is a no-op that returns RS_OK.
 * RS_ERR_INVALID: a null out, d0 or sel; basebit outside 1 .. 8; l < 1; l basebit > 31; stride = 0; an R and stride whose row
 * arithmetic would overflow or whose grid passes one launch; an out that shares a byte with d0, d1 or sel ("out overlaps d0").
 * Without a device or context it fails as rs_ring_rekey_dev does. */
int rs_ring_cmux_dev(rs_ctx* ctx, int32_t* out, const int32_t* d1, const int32_t* d0, size_t R, size_t stride,
                     const int32_t* sel, int32_t basebit, int32_t l, void* stream);
/* out DEVICE int32[2][N] = table[index] for table DEVICE int32[entries][2][N], 1 <= entries <= 2^depth, 1 <= depth <= 30, and sel
 * DEVICE int32[depth][2l][2][N]: sample k selects on bit k of the index, least significant bit first. Entries at or past `entries`
 * count as the all-zero ciphertext, so an index past `entries` yields an encryption of zero. Level k is one rs_ring_cmux_dev-shaped
 * launch over the pairs (2r, 2r + 1) of the previous level with stride 2; an unpaired last row runs as a second launch with d1 =
 * NULL, also where it is the only row of its level. scratch DEVICE int32[ceil(E/2) + ceil(E/4)][2][N], E = entries, used as two
 * ping-pong halves; it may be NULL when depth = 1. The last level writes out. An out that overlaps table, sel or scratch, and a
 * scratch that overlaps table or sel, are refused. Otherwise as rs_ring_cmux_dev, and RS_ERR_INVALID also for a null table, depth
 * or entries out of range, a null scratch with depth > 1, and those overlaps ("out overlaps scratch"). */
int rs_ring_lookup_dev(rs_ctx* ctx, int32_t* out, const int32_t* table, size_t entries,
                       const int32_t* sel, int32_t depth, int32_t basebit, int32_t l, int32_t* scratch, void* stream);
/* The alternating form of the two calls above, for selectors made by circuit bootstrapping. Everything
 * is as in rs_ring_cmux_dev but the digit: the sign of every other source coefficient is flipped before and after the
 * decomposition,
 *   eps_k = +1 for even k, -1 for odd k                      (k = 0 .. N-1, the index of the source coefficient)
 *   dig'_j(x_k) = eps_k dig_j(eps_k x_k)                     (dig_j, off, h_j those of rs_ring_cmux_dev; dig'_j in -B/2 .. B/2)
 *   Da_j(X) = sum_k dig'_j(x.a_k) X^k,   Db_j(X) = sum_k dig'_j(x.b_k) X^k
 * sum_j dig'_j(w) h_j is still w rounded to l basebit bits within the same half step, so the SAME selectors select and phase(out)
 * = phase(d0) + m (phase(d1) - phase(d0)) + noise. The digit at position k has mean -eps_k / 2 instead of -1/2 and the same mean
 * square (B^2 + 2)/12: under a client's selector (independent row noise) the variance above holds unchanged. Under a produced
 * selector (rs_ring_selector_dev, rs_circuit_bootstrap_dev), whose level error is one scalar on the whole digit polynomial, the
 * means no longer add up along S(X): the ramp ((1 - t_c)^2 + N/4)/4 of section 24 becomes (N/4 + [c odd])/4 on every coefficient.
 * The same arguments, checks, overlap refusals, error codes, level and scratch plan as rs_ring_cmux_dev / rs_ring_lookup_dev;
 * asynchronous, no allocation, no loaded key. The words differ from the signed form's; both decrypt to the same selection. */
int rs_ring_cmux_alt_dev(rs_ctx* ctx, int32_t* out, const int32_t* d1, const int32_t* d0, size_t R, size_t stride,
                         const int32_t* sel, int32_t basebit, int32_t l, void* stream);
int rs_ring_lookup_alt_dev(rs_ctx* ctx, int32_t* out, const int32_t* table, size_t entries,
                           const int32_t* sel, int32_t depth, int32_t basebit, int32_t l, int32_t* scratch, void* stream);

/* Encrypted rotation: out[r] = X^(step index_r) in[r stride] for an index the server does not see, the
 * horizontal half of TFHE's levelled mode beside the vertical lookup above. A chain of `depth` CMUXes whose second input is never
 * stored: level k selects between acc and X^(e_k) acc under selector sample k. Word-wise mod 2^32 with negacyclic products; the
 * digits, off and h_j are those of rs_ring_cmux_dev (rs_ring_rotate_alt_dev: those of rs_ring_cmux_alt_dev):
 *   acc_0[r]     = in[r stride]                        (stride = 0 is allowed: every row starts from in[0])
 *   e_k          = (step 2^k) mod 2N                   (64-bit product, k < depth; step any int32)
 *   x_k[r]       = X^(e_k) acc_k[r] - acc_k[r]
 *   acc_(k+1)[r] = acc_k[r] + sum_{j<l} Da_j(X) S_k[j] + sum_{j<l} Db_j(X) S_k[l+j]         over the digits of x_k[r]
 *   out[r]       = acc_depth[r]
 * (X^e v)_c with e = q N + s, 0 <= s < N, is (-1)^q ext_v[c - s + N] for ext_v = (-v, v). S_k is selector sample k of the row's set:
 * sel DEVICE int32[depth][2l][2][N] with per_row = 0 (one hidden index for all rows), int32[R][depth][2l][2][N] with per_row = 1
 * (one index per row); the bits least significant first, the samples rs_ring_lookup_dev takes and rs_circuit_bootstrap_dev makes.
 * phase(out[r]) = X^(step index_r) phase(in[r stride]) + noise: step = -1 brings slot `index` to coefficient 0, step = -w brings
 * slots w index .. w index + w - 1 to coefficients 0 .. w - 1. The noise is that of `depth` CMUXes (the variance of
 * rs_ring_cmux_dev times depth; later levels move a level's error to other coefficients and flip signs, they do not grow it).
 * A level with e_k = 0 leaves the words unchanged (every digit of 0 is 0 in both forms).
 * scratch DEVICE int32[R][2][N], needed for depth >= 2 (NULL is accepted at depth 1): the levels alternate between scratch and out
 * so that the last one writes out, and every level sets its target before it adds into it, so a second call into the same buffers
 * gives the same words. 1 <= depth <= 30. Asynchronous and ordered on `stream`; no allocation; needs no loaded key. R = 0 is a
 * no-op that returns RS_OK.
 * RS_ERR_INVALID, before anything is launched: the refusals of rs_ring_cmux_dev with their texts (a null out, in or sel; basebit
 * outside 1 .. 8; l < 1; l basebit > 31; row arithmetic that overflows; a grid that passes one launch); depth out of range; a null
 * scratch with depth >= 2; an out that overlaps the rows `in` is read from, sel or scratch ("out overlaps in"); a scratch that
 * overlaps in or sel. */
int rs_ring_rotate_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, size_t R, size_t stride,
                       const int32_t* sel, int32_t depth, int32_t per_row, int32_t step, int32_t basebit, int32_t l,
                       int32_t* scratch, void* stream);
int rs_ring_rotate_alt_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, size_t R, size_t stride,
                           const int32_t* sel, int32_t depth, int32_t per_row, int32_t step, int32_t basebit, int32_t l,
                           int32_t* scratch, void* stream);
/* u DEVICE int32[R width][N+1]: sample r width + c is the extraction of coefficient c < width of ciphertext r of rlwe DEVICE
 * int32[R][2][N], in the convention of rs_rlwe_extract_dev (that call's word formula with the slot index replaced): the step
 * between a rotated ciphertext and rs_keyswitch_dev. 1 <= width <= N; u must not overlap rlwe ("u overlaps rlwe"). Asynchronous, no
 * allocation, no loaded key; R = 0 is a no-op. */
int rs_ring_heads_dev(rs_ctx* ctx, int32_t* u, const int32_t* rlwe, size_t R, size_t width, void* stream);

/* Batched encrypted lookup: out DEVICE int32[R][2][N], out[q] = table_q[index_q], R of the trees of
 * rs_ring_lookup_dev side by side with ONE init and ONE sweep launch per level for all rows. Entry e < entries of row q's table is
 * the ciphertext at table + (q row_stride + e entry_stride) 2N words:
 *   row_stride = 0                              every row reads one shared table
 *   row_stride = entries, entry_stride = 1      R tables stored one after another
 *   row_stride = 1, entry_stride = R            the layout [entries][R][2][N] of entries that are R ciphertexts wide
 * and any row_stride >= 0, entry_stride >= 1 is accepted; the tables are only read and may overlap each other. sel DEVICE
 * int32[depth][2l][2][N] with per_row = 0 (one hidden index for all rows), int32[R][depth][2l][2][N] with per_row = 1: the layouts
 * rs_ring_rotate_dev takes and rs_circuit_bootstrap_batch_dev writes. The arithmetic is that of rs_ring_lookup_dev
 * (rs_ring_lookup_rows_alt_dev: of rs_ring_lookup_alt_dev) row by row: level k pairs rows (2i, 2i + 1) of row q's previous level
 * under sample k of row q's set, an unpaired last row meets the all-zero ciphertext (inside the same launch), entries at or past
 * `entries` count as zero, and every word of out[q] equals what the single call gives for row q's table and selectors. Integer
 * arithmetic mod 2^32, exact in any order; the noise is that of rs_ring_lookup_dev.
 * scratch DEVICE int32[R (ceil(E/2) + ceil(E/4))][2][N], E = entries: two ping-pong halves of R ceil(E/2) and R ceil(E/4)
 * ciphertexts. Level k writes [R][P_k][2][N] contiguously from the start of half k & 1, P_k the rows its trees leave; the next
 * level reads that with row stride P_k and entry stride 1; the last level writes out. NULL is accepted at depth 1. Every level
 * sets its target before it adds into it, so a second call into the same buffers gives the same words. 1 <= depth <= 30.
 * Asynchronous and ordered on `stream`; no allocation; needs no loaded key. R = 0 is a no-op that returns RS_OK.
 * RS_ERR_INVALID, before anything is launched: a null out, table or sel; the digit-shape and ring refusals of rs_ring_cmux_dev;
 * depth outside 1 .. 30; entries outside 1 .. 2^depth; entry_stride = 0; a null scratch with depth > 1; row arithmetic that
 * overflows (the read extent of (R - 1) row_stride + (entries - 1) entry_stride + 1 ciphertexts, the selector sets, the scratch);
 * a level whose workgroups pass one launch; an out that overlaps the table extent, sel or scratch ("out overlaps table"); a
 * scratch that overlaps table or sel. Without a device or context it fails as rs_ring_cmux_dev does. */
int rs_ring_lookup_rows_dev(rs_ctx* ctx, int32_t* out, const int32_t* table, size_t entries,
                            size_t row_stride, size_t entry_stride, size_t R,
                            const int32_t* sel, int32_t depth, int32_t per_row,
                            int32_t basebit, int32_t l, int32_t* scratch, void* stream);
int rs_ring_lookup_rows_alt_dev(rs_ctx* ctx, int32_t* out, const int32_t* table, size_t entries,
                                size_t row_stride, size_t entry_stride, size_t R,
                                const int32_t* sel, int32_t depth, int32_t per_row,
                                int32_t basebit, int32_t l, int32_t* scratch, void* stream);

/* Circuit bootstrapping (CGGI17 section 4): the selectors of rs_ring_cmux_dev / rs_ring_lookup_dev made
 * on the server from LWE bits it computed itself. rs_ring_selector_dev is the step in the middle, a keyswitch from LWE samples to
 * ring samples under two key families, one of them private (the message multiplied by -S(X)). Word-wise mod 2^32 with the
 * unsigned rounding digits of rs_pack_dev / rs_rekey_dev:
 *   h_j  = 2^(32-(j+1) basebit)                      l basebit <= 31, so h_j/2 is an integer
 *   ct[k l + j] = (a, b), n_src-dimensional: the bootstrap of bit k at level j, phase +-h_j/2
 *   x    = (a_0 .. a_{n_src-1}, b + h_j/2)           n_src + 1 coordinates, phase = -sum_i x_i sg_i, sg = (s, -1)
 *   K[f][i][q]  = ring sample under S of  M_f sg_i 2^(32-(q+1) ks_basebit),   M_1 = 1 (X^0),  M_0 = -S(X)
 *   d_iq = ((x_i + off) >> (32-(q+1) ks_basebit)) & (2^ks_basebit - 1),   off = 2^(31 - ks_t ks_basebit)  (0 at 32 bits)
 *   sel[k][f l + j] = - sum_{i <= n_src, q < ks_t} d_iq K[f][i][q]                    f = 0, 1
 * sel DEVICE int32[depth][2l][2][N], the format rs_ring_cmux_dev / rs_ring_lookup_dev read: rows j < l have phase -m h_j S + noise,
 * rows l + j have phase m h_j at coefficient 0 and noise elsewhere (m the bit, 1 for a phase of +h_j/2). ct DEVICE
 * int32[depth l][n_src+1]; sel_key DEVICE int32[2][n_src+1][ks_t][2][N], 16-byte aligned (client.SecretKeySet.selector_key);
 * a sel that overlaps ct or sel_key is refused (the kernels add into sel with atomics). n_src is an argument, as in rs_rekey_dev: the context's n (after rs_bootstrap_lut_dev) or N (extracted
 * samples before the LWE keyswitch); N is the context's ring, 1024 .. 8192. Per coefficient the keyswitch adds an error of variance
 *   (n_src + 1) ks_t (2^ks_basebit - 1)(2^(ks_basebit+1) - 1)/6 sigma_k^2  +  rho (1 + n_src/2) 2^(-2 ks_t ks_basebit)/12
 * (sigma_k the deviation of a key row; rho = 1 where the message sits: coefficient 0 of rows l + j and the coefficients of rows
 * j < l at which S has a bit, 0 elsewhere), beside the bootstrap's own noise, which reaches the same coefficients.
 * Integer arithmetic only, exact: the words do not depend on how the work is tiled. Needs no loaded key. Asynchronous and ordered
 * on `stream`; no allocation. depth = 0 is a no-op that returns RS_OK. A second call into the same buffer gives the same words.
 * RS_ERR_INVALID: a null sel, ct or sel_key; basebit or ks_basebit outside 1 .. 8; l < 1; l basebit > 31; ks_t < 1; ks_t ks_basebit >
 * 32; depth outside 0 .. 30; n_src outside 1 .. 65536; a misaligned sel_key; row arithmetic that overflows or a grid past one
 * launch; a sel that shares a byte with ct or sel_key ("sel overlaps ct"). Without a device or context it fails as rs_pack_dev does. */
int rs_ring_selector_dev(rs_ctx* ctx, int32_t* sel, const int32_t* ct, int32_t depth, int32_t basebit, int32_t l,
                         int32_t n_src, const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, void* stream);
/* The composed call: bits DEVICE int32[depth][n+1] at +-1/8 under the context's loaded key (m = 1 is a phase of +1/8) become sel
 * DEVICE int32[depth][2l][2][N]. On the stream: each bit is replicated l times (rs_gather_rows_dev), ONE rs_bootstrap_lut_dev launch
 * takes the depth l rows, row k l + j against the constant test polynomial h_j/2, and rs_ring_selector_dev switches the results
 * from n_src = n. scratch DEVICE int32[l N + depth l (2 (n + 1) + 1)]: the l test polynomials, the row index of the gather, the
 * replicated bits and their bootstraps; a sel that overlaps bits, sel_key or scratch, and a scratch that overlaps bits or sel_key,
 * are refused. Needs a loaded evaluation key (RS_ERR_STATE without
 * one); all three arithmetic modes, with the certificate and mode rules of the other bootstrapped calls. Otherwise as
 * rs_ring_selector_dev, and RS_ERR_INVALID also for a null bits or scratch and for those overlaps ("sel overlaps scratch"). */
int rs_circuit_bootstrap_dev(rs_ctx* ctx, int32_t* sel, const int32_t* bits, int32_t depth, int32_t basebit, int32_t l,
                             const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, int32_t* scratch, void* stream);
/* The batch forms: any number of bits in one call. `count` replaces depth and is bounded only by what
 * one launch can index; the arithmetic, the key format, the digit rules, the checks and the refusals are those of the two calls
 * above with the extents computed from count: ct DEVICE int32[count l][n_src+1], bits DEVICE int32[count][n+1], sel DEVICE
 * int32[count][2l][2][N], scratch DEVICE int32[l N + count l (2 (n + 1) + 1)] in the same layout. Every word of sel equals what the
 * calls above give for the same bits taken 30 at a time, in all three arithmetic modes. rs_circuit_bootstrap_batch_dev runs the
 * same steps with ONE rs_bootstrap_lut_dev launch over the count l rows. The keyswitch runs in one of two forms, chosen from the row
 * count and the context's compute units: the chunked kernel of rs_ring_selector_dev (atomic adds), or, as soon as count l rows
 * give every compute unit a workgroup of it, a wide kernel that sums all n_src + 1 coordinates in registers and stores each word
 * once. RS_SEL_FORM=wide|chunked, read once in rs_create, forces a form at any size (diagnostics and tests); rs_ring_selector_dev
 * always takes the chunked kernel. sel must be 16-byte aligned ("sel must be 16-byte aligned"). A count whose rows pass one launch
 * is refused with RS_ERR_INVALID ("count l = ... rows are too many for one launch") before anything is launched; count = 0 is a
 * no-op that returns RS_OK. Asynchronous and ordered on `stream`; no allocation; a second call into the same buffers gives the
 * same words. */
int rs_ring_selector_batch_dev(rs_ctx* ctx, int32_t* sel, const int32_t* ct, size_t count, int32_t basebit, int32_t l,
                               int32_t n_src, const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, void* stream);
int rs_circuit_bootstrap_batch_dev(rs_ctx* ctx, int32_t* sel, const int32_t* bits, size_t count, int32_t basebit, int32_t l,
                                   const int32_t* sel_key, int32_t ks_basebit, int32_t ks_t, int32_t* scratch, void* stream);
/* Form (0 chunked, 1 wide) and workgroups of the context's last selector keyswitch, batch or not; RS_ERR_STATE before the first. */
int rs_last_selector(rs_ctx* ctx, int32_t* form, int64_t* workgroups);

/* The packing key on the device: generation, expansion on load and (below, rs_audit_pack_key_dev) the
 * exact noise audit, the three steps the evaluation key has. n and N are the context's; row i t + j of the key is K[i][j]. All three
 * need no loaded key and work on every context, N = 1024 .. 8192: 32-bit integer adds, no product, no transform, no mode dependence.
 *
 * rs_pack_keygen_dev (CLIENT): body[i t + j] = a*S + e + s_i 2^(32-(j+1) basebit) X^0, negacyclic mod 2^32, a = words 0 .. N-1 of
 * stream (14, i t + j) of the mask seed, e_k = Gaussian k of stream (15, i t + j) of the noise seed through kg_noise32: word for
 * word redsec_amd/keygen.py pack_key (up to its note on the last bit of numpy's log / cos). body DEVICE int32[n][t][N]. lwe_key,
 * tlwe_key HOST int32[n], int32[N] with words in {0, 1}; their private device copy (packed bits) is zeroed and freed on every path.
 * The mask never reaches global memory. stdev: any finite value >= 0 (0 for word-identity tests; what deviation a key may have is the
 * caller's policy, redsec_amd/client.py). Synchronous, like rs_keygen_dev.
 * RS_ERR_INVALID: null pointer; key word outside {0, 1}; equal seeds; basebit outside 1 .. 8; t < 1; t basebit > 32; negative or
 * non-finite stdev; n t whose row arithmetic would overflow.
 *
 * rs_pack_expand_dev (SERVER): pack_key[i][j] = (the domain-14 stream of row i t + j of the mask seed, body[i][j]): the key
 * rs_pack_dev takes, from the seed and the bodies that travel. pack_key DEVICE int32[n][t][2][N], must not overlap body; body DEVICE
 * int32[n][t][N]. Asynchronous and ordered on `stream`; no allocation. RS_ERR_INVALID: null pointer; t < 1; overflow as above.
 * Without a device or context both fail as rs_pack_dev does. */
int rs_pack_keygen_dev(rs_ctx* ctx, int32_t* body, const int32_t* lwe_key, const int32_t* tlwe_key,
                       const uint8_t* mask_seed, const uint8_t* noise_seed, int32_t basebit, int32_t t, double stdev);
int rs_pack_expand_dev(rs_ctx* ctx, int32_t* pack_key, const uint8_t* mask_seed, const int32_t* body, int32_t t, void* stream);

/* Device decryption and the exact noise audit of evaluation keys. CLIENT side: a server holds no secret.
 * All three are synchronous like rs_keygen_dev and additionally wait for ALL work queued on the context's device, on every stream,
 * before they read their inputs. Secret keys are HOST pointers with words in {0, 1}; their private device copy (packed bits) is
 * zeroed and freed on every path. The context's loaded key is not touched and none is needed. The arithmetic is 32-bit integer
 * only (a'*S is a signed sum of rotated copies of a' over the set bits of S): no floating-point product, so they work on every
 * context and share nothing with the split-key product that generated the key. No CPU fallback: RS_ERR_NO_DEVICE without a device.
 *
 * rs_phase_dev: phase[i] = b_i - sum_k a_ik key_k (mod 2^32) of ct int32[B][dim+1]. dim = n with the LWE key, or dim = k N with the
 * TRLWE key read as an LWE key (the extracted key of rs_bootstrap_wo_ks_dev's output). phase, ct DEVICE; key HOST int32[dim].
 * B = 0 is a no-op. RS_ERR_INVALID: null pointer, dim not n or k N, key word outside {0, 1}. */
int rs_phase_dev(rs_ctx* ctx, int32_t* phase, const int32_t* ct, size_t B, const int32_t* key, int32_t dim);

typedef struct rs_key_audit {
  uint32_t bk_max_abs, ksk_max_abs;   /* largest |noise word| read as signed 32-bit (|INT32_MIN| = 2^31) */
  uint64_t bk_over, ksk_over;         /* noise words with |e| > bk_limit / ksk_limit */
  uint64_t ksk_zero_bad;              /* full key only: v = 0 samples with any non-zero word */
  uint64_t bk_words, ksk_words;       /* noise words looked at: n 2l N and N t (2^basebit - 1); 0 for a skipped half */
} rs_key_audit;

/* "Is this key, as it lies in device memory, an encryption of my secret with the noise I asked for?" -- every word of it.
 * Noise words, all arithmetic mod 2^32, products negacyclic, g_j = 2^(32 - (j+1) Bgbit), row p = c l + j of key bit s_i:
 *   bk, full key, stored row (a', b):  e = b - a'*S - s_i g_j X^0 for c = 1;  e = b - a'*S + s_i g_j S for c = 0
 *     (for c = 0 the stored mask carries the gadget term, a' = a + s_i g_j X^0, so b - a'*S = e - s_i g_j S);
 *   bk, compressed: the same two formulas with a' = the domain-3 stream of the mask seed and b = the body row;
 *   ksk sample (i, j, v), v >= 1:  e = b - sum_k a_k s_k - ((S_i v) << (32 - (j+1) basebit)); compressed: a = domain 5, b = the body word;
 *   ksk, v = 0: the noise word is 0. Full key: the sample counts in ksk_zero_bad if any of its n + 1 words is non-zero.
 *     Compressed: the body word is ignored, as rs_expand_keys_dev ignores it.
 * A correctly generated key returns exactly the generator's noise words (the domain-4 and domain-6 Gaussians of rs_keygen_dev); a
 * noiseless key returns zeros. redsec_amd/keygen.py restates it (bk_noise, ksk_noise, audit; noise_limits gives default limits).
 *
 * rs_audit_keys_dev: the full key, layouts of rs_load_keys (no alignment needed). bk or ksk may be NULL (that half is skipped; both
 * NULL is RS_ERR_INVALID). bk_noise int32[n][2l][N] and ksk_noise int32[N][t][2^basebit] are optional DEVICE outputs (NULL: report
 * only). report is HOST. RS_ERR_INVALID also for a null report or key and key words outside {0, 1}.
 * rs_audit_compressed_keys_dev: the same on a compressed key WITHOUT expanding it: masks regenerated from the public mask seed. */
int rs_audit_keys_dev(rs_ctx* ctx, rs_key_audit* report, int32_t* bk_noise, int32_t* ksk_noise,
                      const int32_t* bk, const int32_t* ksk, const int32_t* lwe_key, const int32_t* tlwe_key,
                      uint32_t bk_limit, uint32_t ksk_limit);
int rs_audit_compressed_keys_dev(rs_ctx* ctx, rs_key_audit* report, int32_t* bk_noise, int32_t* ksk_noise,
                                 const uint8_t* mask_seed, const int32_t* bk_body, const int32_t* ksk_body,
                                 const int32_t* lwe_key, const int32_t* tlwe_key, uint32_t bk_limit, uint32_t ksk_limit);

/* rs_audit_pack_key_dev (CLIENT): the same question for a packing key, the only other key material a
 * server holds; a bad row publishes a bit of the LWE secret. Noise word of row i t + j: e = b - a*S - s_i 2^(32-(j+1) basebit) X^0.
 * mask_seed NULL: key is the full key DEVICE int32[n][t][2][N] (what rs_pack_dev reads). With a mask seed: key is the bodies DEVICE
 * int32[n][t][N] and a is regenerated from the seed, without expanding. noise: optional DEVICE int32[n][t][N]. report is HOST.
 * A correctly generated key returns exactly the generator's domain-15 words; a noiseless key returns zeros. Integer arithmetic only,
 * a signed sum of rotations over the set bits of S: another loop than the generator's. Synchronous; waits for ALL work queued on the
 * device before it reads, as the audits above; secrets are HOST pointers handled as there. redsec_amd/keygen.py restates it
 * (pack_key_noise; pack_noise_limit gives a default limit).
 * RS_ERR_INVALID: a null report, key or secret; key words outside {0, 1}; basebit, t as for rs_pack_keygen_dev. */
typedef struct rs_pack_key_audit {
  uint32_t max_abs;   /* largest |noise word| read as signed 32-bit (|INT32_MIN| = 2^31) */
  uint64_t over;      /* noise words with |e| > limit */
  uint64_t words;     /* noise words looked at: n t N */
} rs_pack_key_audit;
int rs_audit_pack_key_dev(rs_ctx* ctx, rs_pack_key_audit* report, int32_t* noise, const int32_t* key, const uint8_t* mask_seed,
                          const int32_t* lwe_key, const int32_t* tlwe_key, int32_t basebit, int32_t t, uint32_t limit);

/* Arithmetic of the external product (both keys are resident after rs_load_keys; switching is free):
 *   RS_MODE_FFT        folded 512-point complex FP64 FFT -- the arithmetic class of TFHE's own
 *                      tGswFFTExternMulToTLwe -- rounded to the nearest integer. The true product is an
 *                      integer and the FFT error is two orders of magnitude below 1/2, so rounding returns
 *                      exactly the integer result. Every bootstrapped call records the largest distance to an
 *                      integer it rounded (its "certificate") and is followed, on the same stream, by the
 *                      exact-NTT kernels GATED on that certificate: they return at once while it is below the
 *                      limit and otherwise overwrite the call's result with the exact one before anything
 *                      downstream reads it. No host round trip; holds for the *_dev calls and the host calls alike.
 *   RS_MODE_EXACT_NTT  exact negacyclic NTT over a 51-bit prime carried in FP64: exact by construction,
 *                      2.3x the FP64 operations.
 *   RS_MODE_FFT_SPLIT  the same FP64 FFT with the key split into two signed 16-bit halves (twice the pointwise
 *                      products and inverse transforms). Every half product stays below 2^40, where the FFT's
 *                      WORST-CASE error is below 1/2 for every parameter set the reference defines (a-priori bound
 *                      derived in csrc/rs_general.h, rs_split_bound: 3e-4 ... 0.011 for N = 1024, 0.10 for N = 4096,
 *                      0.30 for N = 8192): rounding is exact for EVERY input. The general kernels (N >= 2048, or any
 *                      gadget outside the shipped ones) also ENFORCE a rounding certificate: a call that rounds a value
 *                      1/4 or more away from an integer makes the next call on its stream, rs_sync, rs_certify and the
 *                      host-pointer calls fail with RS_ERR_INEXACT (never observed: measured distances are 4e-6).
 *                      General kernels: any N in {1024 ... 8192}, any gadget; the only mode of the sets outside the
 *                      specialised N = 1024 kernels.
 * Results are identical word for word in all modes (= the CPU oracle).
 * Default RS_MODE_FFT where available (environment REDSEC_MODE=exact | split selects another at context creation;
 * the environment is read ONCE, in rs_create). rs_set_mode must not race with launches of the same context. */
enum { RS_MODE_EXACT_NTT = 0, RS_MODE_FFT = 1, RS_MODE_FFT_SPLIT = 2 };
int rs_set_mode(rs_ctx* ctx, int mode);
int rs_get_mode(rs_ctx* ctx, int* mode);
/* The a-priori bound on |computed - true coefficient| of a split-key product for this context's parameters (derived in
 * csrc/rs_general.h from the rounding model of the FP64 butterflies actually used; nothing quoted). The mode is offered
 * when it is below 1/2, i.e. when rounding to the nearest integer is exact for every input. */
int rs_split_bound(rs_ctx* ctx, double* bound);
/* A call whose certificate reaches this limit is recomputed exactly on the device (default 0.25: an error
 * of +-1 needs a distance > 0.5). limit = 0 forces the recomputation of every call (tests). */
#define RS_CERTIFICATE_LIMIT 0.25
int rs_set_certificate_limit(rs_ctx* ctx, double limit);
/* Synchronises `stream` and reports what its calls did since the last reset: the largest rounding distance
 * and how many calls were recomputed exactly (expected: 0). Either pointer may be NULL. */
int rs_certify(rs_ctx* ctx, void* stream, double* max_distance, int64_t* recomputed_calls, int reset);
/* The same over ALL streams of the context (device-wide synchronisation). */
int rs_rounding_certificate(rs_ctx* ctx, double* max_distance, int reset);
int rs_fft_fallbacks(rs_ctx* ctx, int64_t* count);

/* Streams. A context keeps one private slice of mutable state per stream it has seen (extracted-sample
 * workspace, work counter, certificate slots, convolution scratch, timing events), so *_dev calls on
 * DIFFERENT streams of one context may be issued concurrently, also from different host threads; calls on
 * one stream are ordered by the stream. The synchronous host-pointer calls are serialised per context.
 * Workspace is grown on demand (a device-wide wait); rs_reserve pre-sizes the default stream's,
 * rs_reserve_stream a given stream's, for batches of up to max_batch ciphertexts. */
int rs_reserve(rs_ctx* ctx, size_t max_batch);
int rs_reserve_stream(rs_ctx* ctx, size_t max_batch, void* stream);

/* out[b] = tfhe_bootstrap_FFT(mu, in[b]) for b < B. */
int rs_bootstrap_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, int32_t mu, size_t B, void* stream);
int rs_bootstrap(rs_ctx* ctx, int32_t* out, const int32_t* in, int32_t mu, size_t B);

/* Sparse bootstraps: rs_bootstrap_dev for a batch of which the caller KNOWS most rows to be trivial
 * samples (0, ..., 0, b), e.g. the output channels of a convolution whose ternary weights are all zero. in, out DEVICE
 * int32[B][n+1] (out == in is allowed; any other overlap is the caller's error); live DEVICE int32[n_live]: the rows that are
 * really bootstrapped; n_live a HOST value: the launch form is planned from it exactly as rs_bootstrap_dev plans from B.
 *   A row named in live gets the words of rs_bootstrap_dev(in[r], mu).
 *   AN UNLISTED ROW IS READ AT WORD n ONLY: it is the caller's promise of a trivial sample and gets (0, ..., 0, b'), b' =
 *   coefficient 0 of the test vector rotated by the mod-switched in[r][n] (+-mu) -- the words the dense call produces for
 *   (0, ..., 0, in[r][n]), where no CMUX runs and the keyswitch of a zero mask subtracts nothing.
 * Entries of live outside [0, B) are ignored on the device; a repeated entry is harmless (the same words are written twice).
 * Nothing else is validated on the device, and it never reads or writes outside in, out, live and the context's own buffers.
 * n_live = 0 launches no rotation and no keyswitch (rs_last_launch and rs_last_kernel_ms then answer RS_ERR_STATE: nothing was
 * launched); n_live = B with the identity list gives the dense call's words; B = 0 is a no-op that returns RS_OK.
 * RS_ERR_INVALID: a null in or out, a null live with n_live > 0, n_live > B, row arithmetic that overflows.
 * On the stream: in[live[i]] is gathered into the per-stream staging buffer of rs_gate_rows_dev (grown on demand to 2 n_live
 * rows: a device-wide wait), all B rows of out are filled with the trivial result (each row reads its own word n before it is
 * overwritten), the unchanged blind rotation and keyswitch take the n_live staged rows into the second half of the staging
 * buffer, and that half is scattered into out[live[i]]. Asynchronous and stream-ordered; all three arithmetic modes and every
 * parameter set, with the certificate rules of the other bootstrapped calls (the gated exact recomputation re-reads the staged
 * rows, never in). rs_last_launch and rs_last_kernel_ms describe the compact launch of n_live rows; the gather and the fill run
 * in front of the two timed intervals, the scatter behind them. */
int rs_bootstrap_sparse_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, int32_t mu, size_t B, const int32_t* live, size_t n_live,
                            void* stream);

/* Programmable bootstrap: tfhe_blindRotateAndExtract_FFT with the test polynomial lut[(lut_first + b) % lut_count]
 * (DEVICE int32[lut_count][N]; lut_first lets a caller that shards a batch keep the batch-wide assignment)
 * followed by lweKeySwitch. With pbar = the phase of in[b] mod-switched to
 * [0, 2N): out[b] encrypts lut[pbar] for pbar < N and -lut[pbar - N] beyond. Serves the corrected
 * Quantize::relu_shift (lib/IntFunc.cpp:934-973, lib/BinFunc.cpp:1120-1162): one bootstrap per neuron
 * evaluates clamp((slope x + bias) >> slope_bits, 0, 2^shift_bits - 1), see DESIGN.md "ReLU semantics". */
int rs_bootstrap_lut_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, const int32_t* lut, size_t lut_count, size_t lut_first,
                         size_t B, void* stream);

/* out[b] = boots<OP>(a[b], b[b]) (mu = 1/8 encoding). */
int rs_gate_dev(rs_ctx* ctx, rs_gate_op op, int32_t* out, const int32_t* a, const int32_t* b, size_t B, void* stream);
int rs_gate(rs_ctx* ctx, rs_gate_op op, int32_t* out, const int32_t* a, const int32_t* b, size_t B);

/* Same gate, but the output encodes the result as +-mu instead of +-1/8 (the test-vector value is a
 * free parameter of the bootstrap). Used by the max-pool OR chain, whose last OR must hand +-1/4096
 * to the next linear stage (lib/BinFunc.cpp:880-925 feeds +-1/4096 sign outputs to bootsOR, which
 * assumes +-1/8: see DESIGN.md "max-pool semantics"). */
int rs_gate_mu_dev(rs_ctx* ctx, rs_gate_op op, int32_t* out, const int32_t* a, const int32_t* b, int32_t mu, size_t B, void* stream);

/* Three-input gates and indexed gate batches (no reference counterpart: the reference composes
 * two-input gates, five per full-adder bit). One bootstrap of a linear combination of THREE +-1/8 inputs gives a majority or a parity:
 * a full adder is XOR3 + MAJ3, a subtractor XOR3 + MAJ3N. With e8 = 2^29 (1/8) and e4 = 2^30 (1/4), row op -> x = c0 a + c1 b + c2 c
 * + (0, bconst), word-wise mod 2^32, and the result is bootstrap_mu(x):
 *   0 NAND  (-1, -1, 0) +e8     1 OR    ( 1,  1, 0) +e8     2 AND   ( 1,  1, 0) -e8     3 NOR   (-1, -1, 0) -e8
 *   4 XOR   ( 2,  2, 0) +e4     5 XNOR  (-2, -2, 0) -e4     6 ANDNY (-1,  1, 0) -e8     7 ANDYN ( 1, -1, 0) -e8
 *   8 ORNY  (-1,  1, 0) +e8     9 ORYN  ( 1, -1, 0) +e8     (rs_gate_op's constants: the third input is ignored and never read)
 *   10 MAJ3 ( 1,  1, 1)  0      11 XOR3 (-2, -2, -2)  0     12 MAJ3N (-1, 1, 1)  0
 * The phase of x lies 1/8 (MAJ3, MAJ3N) or 1/4 (XOR3) from both 0 and 1/2 before noise. */
typedef enum rs_row_op {            /* 0..9 = rs_gate_op with the same values (third input ignored) */
  RS_ROW_MAJ3  = 10,                /* majority(a, b, c):      x =  a + b + c          */
  RS_ROW_XOR3  = 11,                /* a ^ b ^ c:              x = -2a - 2b - 2c       */
  RS_ROW_MAJ3N = 12                 /* majority(!a, b, c):     x = -a + b + c   (borrow of a - b) */
} rs_row_op;
typedef struct rs_row_group { int32_t op; int32_t reserved; uint64_t count; } rs_row_group;

/* out[i] = op(a[i], b[i], c[i]) for op = 10..12 (mu = 1/8 encoding): rs_gate_rows_dev with one group, three base pointers and the
 * identity index. RS_ERR_INVALID for another op or a null pointer; B = 0 is a no-op. */
int rs_gate3_dev(rs_ctx* ctx, int op, int32_t* out, const int32_t* a, const int32_t* b, const int32_t* c, size_t B, void* stream);

/* One bootstrap batch of B rows with MIXED ops over rows picked by index. in int32[in_rows][n+1], idx DEVICE int32[B][3],
 * groups HOST (read before the call returns), out int32[B][n+1]. The rows are cut into n_groups consecutive runs: the first
 * groups[0].count rows run groups[0].op, and so on. Row r of group g:
 *   out[r] = bootstrap_mu(sum_j c_j(op_g) s(idx[r][j]) + (0, bconst(op_g))),  s(i) = in[i] for 0 <= i < in_rows,
 *   s(-2) = the trivial TRUE sample (0, +2^29); s(i) = the trivial FALSE sample (0, -2^29) for every other negative i and every
 *   i >= in_rows. Nothing validates idx on the device and nothing needs to: the kernel never reads outside `in`.
 * A constant carry-in is index -1: XOR3(a, b, FALSE) = -2(a + b) + 1/4 decrypts as a ^ b (its words are NOT bootsXOR's: mask and
 * phase are the negation of 2(a + b) + 1/4); MAJ3(a, b, FALSE) = a + b - 1/8 is exactly bootsAND's combination.
 * RS_ERR_INVALID: a null pointer, n_groups outside 1..16, an op outside 0..12, reserved != 0, sum of the counts != B. A group
 * with count 0 is allowed; B = 0 is a no-op that returns RS_OK.
 * `out` may alias rows of `in`, also rows the same call reads: the combinations are materialised in a per-stream staging buffer
 * [B][n+1] (grown on demand like the workspace: a device-wide wait; rs_reserve* do not size it) before any output is written,
 * and the gated exact recomputation of RS_MODE_FFT re-reads that buffer, never `in`.
 * Asynchronous and stream-ordered like every *_dev call; all three arithmetic modes and every parameter set, with the certificate
 * rules of the other bootstrapped calls. The pre-pass (4 B (n+1) 4 bytes of traffic) runs in front of the two intervals
 * rs_last_kernel_ms reports and is in neither. */
int rs_gate_rows_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, size_t in_rows, const int32_t* idx, const rs_row_group* groups,
                     int n_groups, int32_t mu, size_t B, void* stream);

/* Compiled Boolean circuits (no reference counterpart: the reference calls one gate at a time). A
 * circuit is a table of CELLS sorted by level; rs_circuit_run_dev runs it level by level on `lanes` independent data sets, one
 * bootstrap batch per level, without synchronising.
 *   Wires: 0 .. n_inputs-1 are the inputs, cell i defines wire n_inputs + i. Level v is cells [level_end[v-1], level_end[v]).
 *   Sources: src[j] is a wire, -1 (the trivial FALSE sample (0, -2^29)) or -2 (the trivial TRUE sample (0, +2^29)). Bit j of `neg`
 *     negates source j: its coefficient is -c_j (a NOT for free; a negated constant is the other constant). A bit on a source whose
 *     coefficient is 0 is ignored.
 *   Ops 0..12 are the row ops above with their coefficient table: the cell's value is bootstrap_{1/8}(sum_j +-c_j(op) s(src[j]) +
 *     (0, bconst(op))); without neg bits its words are those of rs_gate_rows_dev on the same rows.
 *   Op 13, MUX(a, b, c) = a ? b : c, is bootsMUX as rs_mux_dev computes it: u1 = woKS(a + b - 1/8), u2 = woKS(-a + c - 1/8), value =
 *     KS(u1 + u2 + (0, 1/8)): two blind rotations, one keyswitch; neg bits flip the sign of their source in both combinations.
 *   Arena: DEVICE int32[n_inputs + n_cells][lanes][n+1]; wire w of lane l is row w * lanes + l. The caller fills the input rows, the
 *     call fills every other row (+-1/8 encoding). A circuit does not depend on `lanes`.
 * rs_circuit_create (HOST pointers, read before it returns) validates everything and copies the table to the device once.
 * RS_ERR_INVALID: a null pointer; n_levels = 0; an empty level, level_end not increasing, or its last entry != n_cells; an op outside
 * 0..13; reserved != 0; a src below -2; a src (any of the three, read or not) that is no input, constant or cell of an EARLIER level;
 * a MUX cell followed in its level by another op (the MUX cells of a level come last); more than 2^31 - 1 wires. The device
 * therefore validates nothing and never reads outside the table and the arena. A circuit belongs to its context: rs_destroy frees
 * those still alive, rs_circuit_destroy one (RS_ERR_INVALID for a handle that is not alive: destroyed before, or another context's).
 * rs_circuit_run_dev: asynchronous and stream-ordered; all three arithmetic modes and every parameter set, with the certificate
 * rules of the other bootstrapped calls. lanes = 0 is a no-op; RS_ERR_INVALID for a null arena, a handle that is not alive, or
 * sizes whose row arithmetic would overflow. Per level of C cells, the last M of them MUX: the pre-pass stages (C + M) lanes
 * combinations in the per-stream staging buffer of rs_gate_rows_dev (grown ahead of the first level, like the workspace), the
 * unchanged blind rotation runs over them, a fold adds the MUX rows' second samples, and ONE keyswitch of the first C lanes samples
 * writes the level's arena rows. rs_last_kernel_ms reports the last level. */
typedef enum rs_cell_op { RS_CELL_MUX = 13 } rs_cell_op;   /* 0..12 = rs_gate_op / rs_row_op values */
typedef struct rs_cell { int32_t src[3]; uint8_t op; uint8_t neg; uint16_t reserved; } rs_cell;   /* 16 bytes */
typedef struct rs_circuit rs_circuit;
int rs_circuit_create(rs_ctx* ctx, rs_circuit** out, const rs_cell* cells, size_t n_cells, const uint32_t* level_end, size_t n_levels,
                      size_t n_inputs);
int rs_circuit_destroy(rs_ctx* ctx, rs_circuit* circuit);
int rs_circuit_run_dev(rs_ctx* ctx, const rs_circuit* circuit, int32_t* arena, size_t lanes, void* stream);

/* out[i] = bootsMUX(a[i], b[i], c[i]) = a ? b : c. */
int rs_mux_dev(rs_ctx* ctx, int32_t* out, const int32_t* a, const int32_t* b, const int32_t* c, size_t B, void* stream);
int rs_mux(rs_ctx* ctx, int32_t* out, const int32_t* a, const int32_t* b, const int32_t* c, size_t B);

/* Pieces of the bootstrap, exposed for parity tests and for callers that fuse differently:
 *   blind rotate + sample extract (tfhe_bootstrap_woKS_FFT): in int32[B][n+1] -> u int32[B][k*N+1]
 *   keyswitch (lweKeySwitch):                                 u int32[B][k*N+1] -> out int32[B][n+1] */
int rs_bootstrap_wo_ks_dev(rs_ctx* ctx, int32_t* u, const int32_t* in, int32_t mu, size_t B, void* stream);
int rs_keyswitch_dev(rs_ctx* ctx, int32_t* out, const int32_t* u, size_t B, void* stream);

/* Debug/parity tap: negacyclic product of a small-coefficient polynomial with a torus polynomial
 * through exactly the device transform path used by the external product (HOST pointers). */
int rs_debug_polymul(rs_ctx* ctx, int32_t* out, const int32_t* a_small, const int32_t* b_torus, size_t count);
/* Debug tap of the XCD cohort protocol of the lock-step kernels (no reference counterpart: the reference has no batch kernel):
 * copies the progress table of `stream`'s last cohort launch to out[8 * 64] (HOST) after synchronising the stream. Entry
 * [xcd * 64 + slot] of workgroup (blockIdx & 7, blockIdx >> 3) reads 0x40000000 + the CMUX steps that workgroup walked once it
 * has left; entries no workgroup owned read 0x7f7f7f7f. RS_ERR_STATE before the first such launch. */
int rs_debug_cohort_table(rs_ctx* ctx, void* stream, int32_t* out);
/* Box calibration (no reference counterpart): the FP64 fused-multiply-add lane-operations per second the device sustains right
 * now at the occupancy of the blind-rotation kernels (8 waves per CU, 16 independent chains per lane; best of three 10-ms
 * launches on the default stream). bench.py reports it beside roofline_valu: boxes of one pool differ by several per cent. */
int rs_debug_fp64_rate(rs_ctx* ctx, double* lane_ops_per_s);

/* ---- linear stage on LWE words (no bootstrap), DEVICE pointers ---------------------------------
 * out[m] = bias_b[m % bias_depth] (on the b word, optional) + zero_tap_b * (#zero taps of m)
 *          + sum_k s(k,m) * in[k]
 * with s = +1 where sign[k*M+m] == 1, -1 where 0, and the tap replaced by the constant where
 * zero[k*M+m] == 1 (zero may be NULL). Fully-connected form of Convolution::execute
 * (lib/BinFunc.cpp:217-320: zero_tap_b = 0; lib/IntFunc.cpp:227-308: zero_tap_b = -1/4096). */
int rs_linear_fc_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, const uint8_t* sign, const uint8_t* zero,
                     int32_t K, int32_t M, int32_t zero_tap_b, const int32_t* bias_b, int32_t bias_depth,
                     void* stream);

/* General 2-D convolution over ciphertext feature maps (NHWC), same semantics as above per tap;
 * out-of-bounds taps under same-padding contribute pad_tap_b on the b word.
 * in  int32[H][Wd][Cin][W], out int32[Ho][Wo][Cout][W], sign/zero uint8[fh][fw][Cin][Cout]
 * (get_filter_i, lib/BinFunc.cpp:388). */
typedef struct rs_conv_shape {
  int32_t H, Wd, Cin, Cout, fh, fw, stride_h, stride_w, off_h, off_w, Ho, Wo;
} rs_conv_shape;
int rs_conv_ternary_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, const uint8_t* sign, const uint8_t* zero,
                        const rs_conv_shape* shape, int32_t zero_tap_b, int32_t pad_tap_b,
                        const int32_t* bias_b, int32_t bias_depth, void* stream);

/* Windowed LWE sum (SumPooling::execute, lib/BinFunc.cpp:677-732, lib/IntFunc.cpp:643-700):
 * in int32[H][Wd][C][W] -> out int32[Ho][Wo][C][W]; taps outside the image are skipped. */
typedef struct rs_pool_shape {
  int32_t H, Wd, C, win_h, win_w, stride_h, stride_w, off_h, off_w, Ho, Wo;
} rs_pool_shape;
int rs_sumpool_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, const rs_pool_shape* shape,
                   const int32_t* bias_b, int32_t bias_depth, void* stream);

/* out[i] = ca * a[i] + cb * b[i] word-wise, plus bconst on the b word (b may be NULL).
 * lweAddTo / lweSubTo / lweAddMulTo / lweNoiselessTrivial compositions (lib/BinOps_enc.cpp:37-41,
 * 121-143; lib/IntOps_enc.cpp:35-56). */
int rs_lincomb_dev(rs_ctx* ctx, int32_t* out, const int32_t* a, int32_t ca, const int32_t* b, int32_t cb,
                   int32_t bconst, size_t B, void* stream);

/* out[i] = in[row_index[i]] for i < B (row_index on the device; a negative index gives the trivial
 * zero sample). Gathers the window taps of MaxPooling::execute (lib/BinFunc.cpp:896-921). */
int rs_gather_rows_dev(rs_ctx* ctx, int32_t* out, const int32_t* in, const int32_t* row_index, size_t B, void* stream);

/* Device memory helpers for hosts that do not link HIP themselves (the C++ layer mirror). */
int rs_dev_alloc(rs_ctx* ctx, void** ptr, size_t bytes);
int rs_dev_free(rs_ctx* ctx, void* ptr);
int rs_copy_to_dev(rs_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int rs_copy_to_host(rs_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* Device-to-device copy between the devices of two contexts (the same device is fine): the slice exchange of a
 * stage sharded over several GPUs of one process. Synchronous. */
int rs_copy_dev_to_dev(rs_ctx* dst_ctx, void* dst_dev, rs_ctx* src_ctx, const void* src_dev, size_t bytes);
/* The slice exchange of a stage sharded over the n contexts of one process (the reference's shape: one host process driving
 * NUM_GPUS devices, lib/GPU/Layer.cuh:15,22-37, which has no merge step at all). bufs[d] is context d's full replica
 * int32[rows][row_words]; context d has just computed rows shard(d) = the d-th of n balanced contiguous slices (sizes differ
 * by at most one, lower ranks first) into it, on ITS default stream. Afterwards every replica holds every slice.
 * Entirely asynchronous and event-ordered: each context records an event on its default stream at the start of the call
 * (behind the kernels that wrote its slice AND behind whatever it queued earlier that still reads bufs[d]'s previous
 * contents); every destination first waits for its own event, then pulls slice e on a private copy stream as soon as e's
 * event has fired, so slice e moves while e+1 is still being computed; finally every context's default stream waits for
 * all copies, so later launches (and buffer reuse) on any of them are ordered behind the exchange. Nothing blocks the host.
 * Path per device pair: contexts on one device copy device-to-device; different devices use hipMemcpyPeerAsync over xGMI
 * when hipDeviceCanAccessPeer + hipDeviceEnablePeerAccess succeed (asked once per pair), and otherwise the library stages the
 * slice through pinned host memory itself (source D2H once, each such destination H2D) -- slower, same result
 * (RS_FORCE_HOST_STAGED=1 at rs_create forces that path everywhere: how a one-GPU box tests it). The operation list is
 * host logic (csrc/rs_host.h exchange_plan), checked on the CPU. */
int rs_allgather_rows(rs_ctx* const* ctxs, int n_ctx, int32_t* const* bufs, size_t rows, size_t row_words);
int rs_sync(rs_ctx* ctx);
/* Drops the private state a context keeps for `stream` (workspace, certificate slots, events; see "Streams" above) after
 * synchronising it. For callers that create and destroy many streams: a later stream with the same handle value would
 * otherwise inherit the old one's workspace size and running certificate. The default stream's state cannot be released. */
int rs_release_stream(rs_ctx* ctx, void* stream);

/* Time (ms) of the kernels enqueued by the last *_dev / host call, by HIP events on the stream the
 * kernels ran on; -1 if not available. Index: 0 blind-rotate, 1 keyswitch. */
int rs_set_timing(rs_ctx* ctx, int enable);
int rs_last_kernel_ms(rs_ctx* ctx, float* blind_rotate_ms, float* keyswitch_ms);               /* default stream */
int rs_last_kernel_ms_stream(rs_ctx* ctx, void* stream, float* blind_rotate_ms, float* keyswitch_ms);

/* Facts used by bench.py's roofline accounting. rs_last_launch: what the last blind rotation on `stream`
 * actually ran -- form 0 per-wave, 1 lock-step workgroups, 2 duo, 3 / 4 cooperative (2 / 4 waves per
 * ciphertext), 5 general (one workgroup of N/16 threads per ciphertext), 6 lock-step workgroups on the split key (8 or 4 waves),
 * 7 cooperative on the split key (2 / 4 waves per ciphertext), 8 duo on the split key, 9 cooperative with 8 waves per ciphertext,
 * 10 the same with the listed step (gadgets with l < 4) -- its waves per workgroup, and `resident` = ciphertexts sharing one sweep of the key (R of the
 * algorithmic-bytes formula). rs_info's waves_per_block is that of the default stream's last launch. */
int rs_last_launch(rs_ctx* ctx, void* stream, int32_t* form, int32_t* waves_per_block, int64_t* resident);
/* What the last keyswitch on `stream` ran: form 0 generic gather (one workgroup per ciphertext), 1 tiled (256 ciphertexts x 32
 * words per workgroup), 2 tiled over `slices` cuts of the input coefficients (small batches), 3 wide (1,024 ciphertexts x 32
 * words per workgroup, one workgroup per CU: large un-sliced batches); `slices` is 1 except in form 2. The environment variable
 * RS_KS_FORM=wide|tiled, read once in rs_create, forces or forbids the wide form (diagnostics and tests). */
int rs_last_keyswitch(rs_ctx* ctx, void* stream, int32_t* form, int32_t* slices);
int rs_info(rs_ctx* ctx, int64_t* bk_device_bytes, int64_t* ksk_device_bytes, int32_t* waves_per_block,
            int32_t* num_cus);

#ifdef __cplusplus
}
#endif
#endif
