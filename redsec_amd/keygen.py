"""Evaluation-key generation on the device (rs_keygen_dev) and its numpy restatement.

Every word of a generated key is a function of a 32-byte seed, the secret keys and the two noise deviations. The streams
(specified in include/redsec_hip.h beside rs_keygen_dev and in csrc/rs_keygen.h):

  Stream (domain, row): word w is word w & 15 of the ChaCha20 block of RFC 8439 section 2.3 whose key is the seed as 8
  little-endian words, word 12 the block counter w >> 4, words 13, 14, 15 = domain, row & 0xffffffff, row >> 32.

  domain 1 LWE secret    row 0                          s_i = word i & 1 (i < n)
  domain 2 TRLWE secret  row 0                          S_j = word j & 1 (j < N)
  domain 3 bk mask       row i 2l + p                   the N mask coefficients of TGSW row p = c l + j of s_i
  domain 4 bk noise      row i 2l + p                   the N Gaussians of that row
  domain 5 ksk mask      row (i t + j) 2^basebit + v    the n mask words of that sample
  domain 6 ksk noise     same row                       1 Gaussian

  Gaussian g of a row uses words 4g .. 4g+3: u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) 2^-53 in (0, 1],
  u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53 in [0, 1), z = sqrt(-2 ln u1) cos(2 pi u2); the noise word is TFHE's
  dtot32(sigma z) (client._gaussian32: fractional part truncated, times 2^32, to int64, wrapped to 32 bits).

  bk row p = c l + j of key bit s_i is (a, b): a = the domain-3 mask, b = a*S + e (mod 2^32, negacyclic); then coefficient 0
  of component c gains s_i 2^(32 - (j+1) Bgbit) (for c = 0, a[0] changes after b was formed).
  ksk samples with v = 0 are all zero; v >= 1: a = the domain-5 words, b = sum_k a_k s_k + e + ((S_i v) << (32 - (j+1) basebit)).

Compressed key (rs_keygen_compressed_dev, rs_expand_keys_dev; include/redsec_hip.h): a public 32-byte MASK SEED and the bodies,
another encryption of the same key with the gadget term of c = 0 rows moved out of the mask:

  bk row p = c l + j of s_i: a = domain 3 of the mask seed (stored unchanged); b = a*S + e + s_i g_j X^0 for c = 1 and
  b = a*S + e - s_i g_j S for c = 0, g_j = 2^(32 - (j+1) Bgbit), e = domain 4 of the noise seed. Same phase as the row above;
  the difference is -s_i g_j (1, S) for c = 0, an exact encryption of zero.
  ksk sample s: a = domain 5 of the mask seed; b as above with e = domain 6 of the noise seed; v = 0 samples are all zero.
  The NOISE SEED (domains 1, 2, 4, 6: the secret keys and the noise) stays private and must differ from the mask seed.
  Layouts: bk_body int32 [n][2l][N], ksk_body int32 [N][t][2^basebit].

Seeded LWE ciphertexts (rs_encrypt_seeded_dev, rs_expand_ciphertexts_dev; include/redsec_hip.h): ciphertext i of a call has
row first + i (a uint64):

  domain 7 ciphertext mask   row first + i   the n mask words a_k (mask seed, public)
  domain 8 ciphertext noise  same row        1 Gaussian, words 0-3 (noise seed, private)

  body = sum_k a_k s_k + e + mu_i (mod 2^32); expanded, the sample is the usual int32 [B][n+1] with the body at word n. Equal seeds
  are refused; first + B must not pass 2^64; a (mask seed, row) pair must never encrypt two messages.

Public-key encryption (rs_pk_encrypt_dev; include/redsec_hip.h): a public key is m encryptions of zero
(a seeded batch with mu = 0); ciphertext i of a call has row first + i (a uint64) of the encryptor's PRIVATE rand seed:

  domain 9   selection bits   row first + i   bit j of ciphertext i = (word (j >> 5) of the stream >> (j & 31)) & 1,  j < m
  ct[i] = (base ? base[i] : 0) + (0, mu ? mu[i] : 0) + sum over j with bit j set of pk[j]      (word-wise mod 2^32)

  Domain 9 is disjoint from domains 1-8. A (rand seed, row) pair must never be used twice; first + B must not pass 2^64.
  pk_selection / pk_encrypt restate it; pk_rows(n) = 32 (n + 1) + 256 is the default m (n log q + 2 lambda).

Compact RLWE public keys (rs_rlwe_pk_encrypt_dev, rs_rlwe_extract_dev; include/redsec_hip.h): the key
is one ring sample (a, b = a*S + e) under the ring secret S, negacyclic mod 2^32; ciphertext r of a call has row first + r of the
encryptor's PRIVATE rand seed and carries N messages:

  domain 10  public-key mask    row 0          mask seed (public)             a_k = word k, k < N
  domain 11  public-key noise   row 0          owner's noise seed (private)   e_k = Gaussian k (words 4k .. 4k+3), k < N
  domain 12  selector u         row first + r  rand seed (private)            u_k = (word (k >> 5) >> (k & 31)) & 1, k < N
  domain 13  encryption noise   row first + r  rand seed                      Gaussians 0 .. N-1 are e1, N .. 2N-1 are e2
  rlwe[r] = (a*u_r + e1, b*u_r + e2 + m_r), m_r = mu[rN .. rN + N - 1] padded with zeros; extraction of coefficient c: word j =
  a'[c - j] (j <= c), -a'[N + c - j] (j > c), word N = b'[c].

  Domains 10-13 are disjoint from domains 1-9. Equal mask and noise seeds are refused; a (rand seed, row) pair must never be used
  twice. rlwe_pk_mask / rlwe_public_key / rlwe_pk_selector / rlwe_pk_encrypt / rlwe_extract / rlwe_phase restate it.

Packed results (rs_pack_dev; include/redsec_hip.h): a public keyswitch from the LWE key s to the ring
key S puts up to N LWE samples into the coefficients of one RLWE ciphertext of the format above. The packing key has, per key bit
s_i and digit j < t, the ring sample K[i][j] = (a_ij, b_ij = a_ij*S + e_ij + s_i 2^(32-(j+1) basebit) X^0):

  domain 14  packing-key mask    row i t + j   mask seed (public)             a_ij[k] = word k, k < N
  domain 15  packing-key noise   row i t + j   owner's noise seed (private)   e_ij[k] = Gaussian k (words 4k .. 4k+3, kg_noise32)
  rlwe[r] = (0, sum_c b_(rN+c) X^c) - sum_{i,j} D_ij(X) K[i][j], D_ij(X) = sum_c ((a_i + off of sample rN+c) >> (32-(j+1) basebit)
  & (2^basebit - 1)) X^c, off = 2^(31 - t basebit) (0 at 32 bits): the digits of lweKeySwitch.

  Domains 14 and 15 are disjoint from domains 1-13. Equal mask and noise seeds are refused. pack_key_mask / pack_key / pack /
  pack_sigma / pack_default restate it.

The packing key on the device (rs_pack_keygen_dev, rs_pack_expand_dev, rs_audit_pack_key_dev; include/redsec_hip.h; INTEGRATION.md
section 19): the bodies above generated by the device word for word, the full key [n][t][2][N] expanded from the seed and the
bodies, and the noise words e_ij = b_ij - a_ij*S - s_i 2^(32-(j+1) basebit) X^0 of a key under its secret. pack_key_noise restates
the audit (through _times_binary, a third arithmetic beside the device's two loops); pack_noise_limit gives the default limit.

Re-keying (rs_rekey_dev; include/redsec_hip.h): a public keyswitch from an LWE key s of dimension n_src
to an LWE key s' of dimension n_dst under a caller-supplied key [n_src][t][n_dst+1] whose row i t + j encrypts s_i 2^(32-(j+1)
basebit) under s'. The key uses no stream of its own: its rows are seeded ciphertexts of rows 0 .. n_src t - 1 (domains 7 / 8) under
the recipient's LWE key, or the rows extracted from RLWE public-key ciphertexts (domains 12 / 13) under the recipient's ring key.
  out[r] = (0, b_r) - sum_{i,j} d_ij(r) K[i][j], d_ij(r) = ((a_i + off of sample r) >> (32-(j+1) basebit)) & (2^basebit - 1).
  rekey_messages / rekey / rekey_sigma / rekey_default restate it.

Ring re-keying (rs_ring_rekey_dev; include/redsec_hip.h): a public keyswitch from a
ring key S to a ring key S' of the same N under a caller-supplied key [t+1][2][N]: row j < t encrypts h_j S, h_j = 2^(31-(j+1)
basebit), row t the constant row c0 (1 + X + ... + X^(N-1)) S, c0 = (2^basebit - 1) sum_j h_j, under S'. The seeded form:

  domain 16  ring re-keying mask    row j   mask seed (public)             a_j[k] = word k, k < N
  domain 17  ring re-keying noise   row j   owner's noise seed (private)   e_j[k] = Gaussian k (words 4k .. 4k+3)
  out[r] = (0, b_r) - K[t] - sum_j D_j(X) K[j], D_j(X) = sum_k (2 (((a_k + off) >> (32-(j+1) basebit)) & (2^basebit - 1)) -
  (2^basebit - 1)) X^k, off = 2^(31 - t basebit): odd digits, symmetric about zero.

  Domains 16 and 17 are disjoint from domains 1-15. Equal mask and noise seeds are refused. The other form is t + 1 ciphertexts of
  rlwe_pk_encrypt (domains 12 / 13) over the same message rows. ring_rekey_messages / ring_rekey_key / ring_rekey_expand /
  ring_rekey / ring_rekey_sigma / ring_rekey_default restate it.

Encrypted selection (rs_ring_cmux_dev, rs_ring_lookup_dev; include/redsec_hip.h): the CMUX of two ring
ciphertexts under an RGSW sample [2l][2][N] of a bit m under the ring key S, and the CMUX tree over a table under `depth` of them.
Row j < l of a sample is a ring sample of zero with m h_j added to a, row l + j has m h_j added to b, h_j = 2^(32-(j+1) basebit).
The seeded form, row = k 2l + j for sample k (bit k of the index, least significant first):

  domain 18  selector mask    row   mask seed (public)              a[i] = word i, i < N (the a the server uses)
  domain 19  selector noise   row   client's noise seed (private)   e[i] = Gaussian i (words 4i .. 4i+3)
  body of row j < l: a*S + e - m h_j S (so that (a - m h_j, body) is a sample of zero); of row l + j: a*S + e + m h_j.
  out = d0 + sum_j Da_j(X) sel[j] + sum_j Db_j(X) sel[l+j], the digits dig_j(w) = (((w + off) >> (32-(j+1) basebit)) & (B - 1)) -
  B/2 of x = d1 - d0, B = 2^basebit, off = sum_j (B/2) h_j + 2^(31 - l basebit): signed, TFHE's tGswTorus32PolynomialDecompH.

  Domains 18 and 19 are disjoint from domains 1-17. Equal mask and noise seeds are refused. ring_cmux_digits / ring_cmux /
  ring_lookup / ring_selector_rows / ring_selector_expand / ring_trivial / ring_cmux_sigma / ring_cmux_default restate it.
  digits="alternating" in ring_cmux_digits / ring_cmux / ring_lookup / circuit_bootstrap_sigma / circuit_bootstrap_default is the
  second digit form (rs_ring_cmux_alt_dev, rs_ring_lookup_alt_dev): eps_k dig_j(eps_k x_k), eps_k = (-1)^k.

Circuit bootstrapping (rs_ring_selector_dev, rs_circuit_bootstrap_dev; include/redsec_hip.h): the
selectors of the section above made by the server from LWE bits. Bit k is bootstrapped at the l levels to phase +-h_j/2, and a
keyswitch from the n_src + 1 coordinates x = (a, b + h_j/2) to the ring key, under two key families, gives the rows of the RGSW
sample. The selector key, row = (f (n_src+1) + i) ks_t + q with sg = (s, -1), g_q = 2^(32-(q+1) ks_basebit):

  domain 20  selector-key mask    row   mask seed (public)             a[c] = word c, c < N
  domain 21  selector-key noise   row   owner's noise seed (private)   e[c] = Gaussian c (words 4c .. 4c+3)
  body of family 1: a*S + e + sg_i g_q (coefficient 0); of family 0: a*S + e - sg_i g_q S, a sample of zero with the message
  folded into the mask side, as selector rows are.
  sel[k][f l + j] = - sum_{i, q} d_iq K[f][i][q],  d_iq = ((x_i + off) >> (32-(q+1) ks_basebit)) & (2^ks_basebit - 1), the unsigned
  rounding digits of pack / rekey, off = 2^(31 - ks_t ks_basebit).

  Domains 20 and 21 are disjoint from domains 1-19. Equal mask and noise seeds are refused. selector_key / selector_key_expand /
  ring_selector_switch / bootstrap_sigma / circuit_bootstrap_sigma / circuit_bootstrap_default restate it.

Noise audit (rs_audit_keys_dev, rs_audit_compressed_keys_dev; include/redsec_hip.h): the noise words of a key under its secret,
all arithmetic mod 2^32, g_j = 2^(32 - (j+1) Bgbit):

  bk row p = c l + j of s_i, stored (a', b): e = b - a'*S - s_i g_j X^0 (c = 1), e = b - a'*S + s_i g_j S (c = 0); compressed: a' = the
  domain-3 stream of the mask seed, b = the body row. ksk sample (i, j, v >= 1): e = b - sum_k a_k s_k - ((S_i v) << (32 - (j+1) basebit));
  v = 0: the noise word is 0 and, in a full key, every word of the sample must be 0. bk_noise / ksk_noise / audit restate it.

The noise words are restated with numpy's log / cos, which may differ from the device's in the last bit of z: a restated
noise word can then differ by one from the device's in the rare case where sigma z 2^32 lies that close to an integer. Mask
words, secret keys and noiseless keys are restated exactly.
"""
import os

import numpy as np

from . import client

DOMAIN_LWE_SECRET, DOMAIN_TLWE_SECRET, DOMAIN_BK_MASK, DOMAIN_BK_NOISE, DOMAIN_KS_MASK, DOMAIN_KS_NOISE = 1, 2, 3, 4, 5, 6
DOMAIN_CT_MASK, DOMAIN_CT_NOISE = 7, 8
DOMAIN_PK_SELECT = 9
DOMAIN_RLWE_MASK, DOMAIN_RLWE_NOISE, DOMAIN_RLWE_SELECT, DOMAIN_RLWE_ENC_NOISE = 10, 11, 12, 13
DOMAIN_PACK_MASK, DOMAIN_PACK_NOISE = 14, 15
DOMAIN_RING_REKEY_MASK, DOMAIN_RING_REKEY_NOISE = 16, 17
DOMAIN_RING_SELECTOR_MASK, DOMAIN_RING_SELECTOR_NOISE = 18, 19
DOMAIN_SELECTOR_KEY_MASK, DOMAIN_SELECTOR_KEY_NOISE = 20, 21
_SIGMA = b"expand 32-byte k"


def _seed_words(seed):
    seed = bytes(seed)
    assert len(seed) == 32, "seed must be 32 bytes"
    return np.frombuffer(seed, dtype="<u4").astype(np.uint32)


def _rotl(v, c):
    return (v << np.uint32(c)) | (v >> np.uint32(32 - c))


def _chacha_blocks(key, domain, rows, blocks):
    """ChaCha20 blocks for every (row, block) pair of the broadcast arrays `rows` (uint64) and `blocks` (uint32) -> [..., 16]."""
    rows, blocks = np.broadcast_arrays(np.asarray(rows, np.uint64), np.asarray(blocks, np.uint32))
    shape = rows.shape
    const = np.frombuffer(_SIGMA, dtype="<u4").astype(np.uint32)
    init = [np.full(shape, const[k], np.uint32) for k in range(4)] + [np.full(shape, key[k], np.uint32) for k in range(8)]
    init += [blocks.astype(np.uint32), np.full(shape, np.uint32(domain & 0xFFFFFFFF), np.uint32),
             (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32)]
    x = [v.copy() for v in init]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 16)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 12)
        x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 8)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 7)
    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        return np.stack([x[k] + init[k] for k in range(16)], axis=-1)


def chacha20_words(seed, domain, row, count):
    """Words [0, count) of stream (domain, row) -> uint32 [count], or [len(row)][count] for an array of rows."""
    key = _seed_words(seed)
    nblk = (int(count) + 15) // 16
    rows = np.asarray(row, np.uint64)
    out = _chacha_blocks(key, domain, rows[..., None], np.arange(nblk, dtype=np.uint32))
    return out.reshape(rows.shape + (nblk * 16,))[..., :int(count)]


def uniforms(w):
    """(u1, u2) of the Gaussians whose words are w[..., 4g:4g+4] (uint32) -> two float64 arrays [..., G]."""
    w = np.asarray(w, np.uint32).reshape(np.shape(w)[:-1] + (-1, 4)).astype(np.uint64)
    u1 = (((w[..., 0] >> np.uint64(5)) << np.uint64(26)) + (w[..., 1] >> np.uint64(6)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (((w[..., 2] >> np.uint64(5)) << np.uint64(26)) + (w[..., 3] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
    return u1, u2


def noise32(w, sigma):
    """dtot32(sigma z) of the Gaussians made from the words w[..., 4g:4g+4] -> int32 [..., G]."""
    u1, u2 = uniforms(w)
    if sigma == 0:
        return np.zeros(u1.shape, np.int32)
    e = float(sigma) * (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2))
    frac = e - np.trunc(e)
    return (frac * 4294967296.0).astype(np.int64).astype(np.uint64).astype(np.uint32).view(np.int32)


def _shape(name, n=None):
    (n0, N, k, l, Bgbit, t, basebit, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    return dict(n=int(n) if n is not None else n0, N=N, l=l, Bgbit=Bgbit, t=t, basebit=basebit, ks_stdev=ks_stdev, bk_stdev=bk_stdev)


def set_name(p):
    """The client.PARAM_SETS name of a parameter set (rs_params; n may be reduced): its ring, gadget and keyswitch shape."""
    for name, (n0, N, k, l, Bgbit, t, basebit, _, _) in client.PARAM_SETS.items():
        if (p.N, p.k, p.bk_l, p.bk_Bgbit, p.ks_t, p.ks_basebit) == (N, k, l, Bgbit, t, basebit):
            return name
    raise KeyError("no parameter set with N=%d l=%d Bgbit=%d t=%d basebit=%d" % (p.N, p.bk_l, p.bk_Bgbit, p.ks_t, p.ks_basebit))


def secret_keys(name, seed, n=None):
    """(lwe_key int32[n], tlwe_key int32[N]) of domains 1 and 2."""
    s = _shape(name, n)
    lwe = (chacha20_words(seed, DOMAIN_LWE_SECRET, 0, s["n"]) & 1).astype(np.int32)
    tlwe = (chacha20_words(seed, DOMAIN_TLWE_SECRET, 0, s["N"]) & 1).astype(np.int32)
    return lwe, tlwe


def _times_binary(A, tlwe_key):
    """Rows of A (uint32 [R][N]) times the binary polynomial S, negacyclic mod 2^32 -> uint32 [R][N]."""
    N = A.shape[-1]
    if N <= 1024:   # the exact float64 matrix product of client.py (an N x N matrix of 8 MB)
        return client._mul_by_binary_poly(A.view(np.int32), client._negacyclic_matrix(np.asarray(tlwe_key))).view(np.uint32)
    out = np.zeros_like(A)
    with np.errstate(over="ignore"):
        for m in np.flatnonzero(np.asarray(tlwe_key)):   # X^m a: a shifted up by m, the wrapped part negated
            out[:, m:] += A[:, :N - m]
            out[:, :m] -= A[:, N - m:]
    return out


def _bk_rows(name, mask_seed, noise_seed, lwe_key, tlwe_key, bk_stdev, rows, n, chunk, compressed):
    s = _shape(name, n if n is not None else len(lwe_key))
    l, Bgbit, N = s["l"], s["Bgbit"], s["N"]
    rows = np.arange(s["n"] * 2 * l) if rows is None else np.asarray(rows, np.int64).ravel()
    lwe = np.asarray(lwe_key).astype(np.uint32)
    tlwe = np.asarray(tlwe_key).astype(np.uint32)
    out = np.empty((len(rows), N) if compressed else (len(rows), 2, N), np.int32)
    with np.errstate(over="ignore"):
        for lo in range(0, len(rows), chunk):
            r = rows[lo:lo + chunk]
            A = chacha20_words(mask_seed, DOMAIN_BK_MASK, r, N)
            B = _times_binary(A, tlwe_key)
            if bk_stdev:
                B += noise32(chacha20_words(noise_seed, DOMAIN_BK_NOISE, r, 4 * N), bk_stdev).view(np.uint32)
            p = r % (2 * l)
            c, j = p // l, p % l
            gadget = lwe[r // (2 * l)] * (np.uint32(1) << (32 - (j + 1) * Bgbit).astype(np.uint32))
            B[c == 1, 0] += gadget[c == 1]
            if compressed:
                B[c == 0] -= gadget[c == 0, None] * tlwe[None, :]
                out[lo:lo + chunk] = B.view(np.int32)
                continue
            A[c == 0, 0] += gadget[c == 0]
            out[lo:lo + chunk, 0] = A.view(np.int32)
            out[lo:lo + chunk, 1] = B.view(np.int32)
    return out


def restate_bk(name, seed, lwe_key, tlwe_key, bk_stdev, rows=None, n=None, chunk=256):
    """bk rows i 2l + p (all n 2l rows if rows is None) -> int32 [R][2][N]."""
    return _bk_rows(name, seed, seed, lwe_key, tlwe_key, bk_stdev, rows, n, chunk, False)


def _ksk_rows(name, mask_seed, noise_seed, lwe_key, tlwe_key, ks_stdev, rows, n, chunk, compressed):
    s = _shape(name, n if n is not None else len(lwe_key))
    n, N, t, basebit = s["n"], s["N"], s["t"], s["basebit"]
    base = 1 << basebit
    rows = np.arange(N * t * base) if rows is None else np.asarray(rows, np.int64).ravel()
    lwe = np.asarray(lwe_key).astype(np.uint64)
    tlwe = np.asarray(tlwe_key).astype(np.uint64)
    out = np.zeros(len(rows) if compressed else (len(rows), n + 1), np.int32)
    for lo in range(0, len(rows), chunk):
        r = rows[lo:lo + chunk]
        v = r % base
        live = np.flatnonzero(v != 0)
        if len(live) == 0:
            continue
        rl = r[live]
        A = chacha20_words(mask_seed, DOMAIN_KS_MASK, rl, n)
        dot = (A.astype(np.uint64) * lwe).sum(axis=-1)
        e = noise32(chacha20_words(noise_seed, DOMAIN_KS_NOISE, rl, 4), ks_stdev)[:, 0] if ks_stdev else np.zeros(len(rl), np.int32)
        ij = rl >> basebit
        i, j = ij // t, ij % t
        mess = (tlwe[i] * (rl % base).astype(np.uint64)) << (32 - (j + 1) * basebit).astype(np.uint64)
        b = (dot + e.view(np.uint32).astype(np.uint64) + mess) & np.uint64(0xFFFFFFFF)
        if compressed:
            out[lo + live] = b.astype(np.uint32).view(np.int32)
            continue
        out[lo + live, :n] = A.view(np.int32)
        out[lo + live, n] = b.astype(np.uint32).view(np.int32)
    return out


def restate_ksk(name, seed, lwe_key, tlwe_key, ks_stdev, rows=None, n=None, chunk=4096):
    """ksk samples s = (i t + j) 2^basebit + v (all of them if rows is None) -> int32 [R][n+1]."""
    return _ksk_rows(name, seed, seed, lwe_key, tlwe_key, ks_stdev, rows, n, chunk, False)


def restate(name, seed, lwe_key, tlwe_key, bk_stdev, ks_stdev, rows=None):
    """The key rs_keygen_dev writes, regenerated on the host. rows=None: the whole (bk [n][2l][2][N], ksk [N][t][2^basebit][n+1]);
    rows=(bk_rows, ksk_rows): only those bk rows ([R][2][N]) and ksk samples ([R'][n+1]); either entry may be None (skipped).
    The LWE dimension is len(lwe_key)."""
    s = _shape(name, len(lwe_key))
    if rows is None:
        bk = restate_bk(name, seed, lwe_key, tlwe_key, bk_stdev).reshape(s["n"], 2 * s["l"], 2, s["N"])
        ksk = restate_ksk(name, seed, lwe_key, tlwe_key, ks_stdev).reshape(s["N"], s["t"], 1 << s["basebit"], s["n"] + 1)
        return bk, ksk
    bk_rows, ksk_rows = rows
    bk = None if bk_rows is None else restate_bk(name, seed, lwe_key, tlwe_key, bk_stdev, bk_rows)
    ksk = None if ksk_rows is None else restate_ksk(name, seed, lwe_key, tlwe_key, ks_stdev, ksk_rows)
    return bk, ksk


def generate(backend, seed=None, bk_stdev=None, ks_stdev=None, load=True):
    """Secret keys of domains 1 / 2 of `seed` (default os.urandom(32)) and the evaluation key generated on the backend's device
    -> (client.SecretKeySet without an evaluation key, bk, ksk as int32 CUDA tensors). Deviations default to the set's
    (client.PARAM_SETS). load=True also makes it the backend's key (rs_load_keys_dev). Client-side operation: see INTEGRATION.md."""
    p = backend.p
    name = set_name(p)
    s = _shape(name, p.n)
    seed = os.urandom(32) if seed is None else bytes(seed)
    bk_stdev = s["bk_stdev"] if bk_stdev is None else bk_stdev
    ks_stdev = s["ks_stdev"] if ks_stdev is None else ks_stdev
    lwe, tlwe = secret_keys(name, seed, p.n)
    bk, ksk = backend.keygen(lwe, tlwe, seed, bk_stdev, ks_stdev)
    if load:
        backend.load_keys_dev(bk, ksk)
    return client.SecretKeySet.from_secret(name, lwe, tlwe), bk, ksk


# ---- compressed keys ----

class CompressedKey:
    """A compressed evaluation key: the set name, the LWE dimension n, the public 32-byte mask seed and the bodies bk_body
    [n][2l][N], ksk_body [N][t][2^basebit] (int32 numpy arrays or CUDA tensors). nbytes: what travels (seed + bodies)."""

    def __init__(self, name, n, mask_seed, bk_body, ksk_body):
        self.name, self.n, self.mask_seed = name, int(n), bytes(mask_seed)
        assert len(self.mask_seed) == 32, "mask seed must be 32 bytes"
        self.bk_body, self.ksk_body = bk_body, ksk_body

    @property
    def nbytes(self):
        s = _shape(self.name, self.n)
        return 32 + 4 * (self.n * 2 * s["l"] * s["N"] + s["N"] * s["t"] * (1 << s["basebit"]))

    def numpy(self):
        """The same key with host bodies."""
        host = lambda x: x if isinstance(x, np.ndarray) else x.cpu().numpy()
        return CompressedKey(self.name, self.n, self.mask_seed, host(self.bk_body), host(self.ksk_body))


def full_nbytes(name, n=None):
    """Bytes of the full evaluation key (bk + ksk) of a set."""
    s = _shape(name, n)
    return 4 * (s["n"] * 2 * s["l"] * 2 * s["N"] + s["N"] * s["t"] * (1 << s["basebit"]) * (s["n"] + 1))


def restate_compressed(name, mask_seed, noise_seed, lwe_key, tlwe_key, bk_stdev, ks_stdev, rows=None):
    """The bodies rs_keygen_compressed_dev writes, regenerated on the host. rows=None: the whole (bk_body [n][2l][N],
    ksk_body [N][t][2^basebit]); rows=(bk_rows, ksk_rows): only those bk rows ([R][N]) and ksk samples ([R']); either may be None.
    The LWE dimension is len(lwe_key). The numpy level does not refuse equal seeds (the tests relate it to restate that way)."""
    s = _shape(name, len(lwe_key))
    bk_rows, ksk_rows = (None, None) if rows is None else rows
    bk = None if rows is not None and bk_rows is None else _bk_rows(name, mask_seed, noise_seed, lwe_key, tlwe_key, bk_stdev, bk_rows, None, 256, True)
    ksk = None if rows is not None and ksk_rows is None else _ksk_rows(name, mask_seed, noise_seed, lwe_key, tlwe_key, ks_stdev, ksk_rows, None, 4096, True)
    if rows is None:
        bk = bk.reshape(s["n"], 2 * s["l"], s["N"])
        ksk = ksk.reshape(s["N"], s["t"], 1 << s["basebit"])
    return bk, ksk


def expand_bk(name, mask_seed, body_rows, rows, chunk=256):
    """Expanded bk rows (rs_expand_keys_dev): the domain-3 masks of `rows` beside their bodies body_rows [R][N] -> int32 [R][2][N]."""
    rows = np.asarray(rows, np.int64).ravel()
    body_rows = np.asarray(body_rows, np.int32).reshape(len(rows), -1)
    out = np.empty((len(rows), 2, body_rows.shape[1]), np.int32)
    for lo in range(0, len(rows), chunk):
        out[lo:lo + chunk, 0] = chacha20_words(mask_seed, DOMAIN_BK_MASK, rows[lo:lo + chunk], body_rows.shape[1]).view(np.int32)
    out[:, 1] = body_rows
    return out


def expand_ksk(name, mask_seed, body_words, rows, n, chunk=4096):
    """Expanded ksk samples (rs_expand_keys_dev): the domain-5 masks of samples `rows` and their body words -> int32 [R][n+1];
    samples with v = 0 are all zero."""
    base = 1 << _shape(name)["basebit"]
    rows = np.asarray(rows, np.int64).ravel()
    body_words = np.asarray(body_words, np.int32).ravel()
    out = np.zeros((len(rows), int(n) + 1), np.int32)
    for lo in range(0, len(rows), chunk):
        r = rows[lo:lo + chunk]
        live = np.flatnonzero(r % base != 0)
        if len(live):
            out[lo + live, :n] = chacha20_words(mask_seed, DOMAIN_KS_MASK, r[live], n).view(np.int32)
            out[lo + live, n] = body_words[lo + live]
    return out


def expand(name, mask_seed, bk_body, ksk_body, n=None, rows=None):
    """The full key of a compressed one, expanded on the host. rows=None: bk_body / ksk_body are whole and the result is the whole
    (bk [n][2l][2][N], ksk [N][t][2^basebit][n+1]); rows=(bk_rows, ksk_rows): bk_body / ksk_body hold the bodies of exactly those
    rows and the result those rows ([R][2][N], [R'][n+1]); either entry may be None (skipped). n defaults to the set's."""
    s = _shape(name, n if n is not None else (np.shape(bk_body)[0] if rows is None else None))
    if rows is None:
        N, l, t, base = s["N"], s["l"], s["t"], 1 << s["basebit"]
        bk = expand_bk(name, mask_seed, np.reshape(bk_body, (-1, N)), np.arange(s["n"] * 2 * l)).reshape(s["n"], 2 * l, 2, N)
        ksk = expand_ksk(name, mask_seed, ksk_body, np.arange(N * t * base), s["n"]).reshape(N, t, base, s["n"] + 1)
        return bk, ksk
    bk_rows, ksk_rows = rows
    bk = None if bk_rows is None else expand_bk(name, mask_seed, bk_body, bk_rows)
    ksk = None if ksk_rows is None else expand_ksk(name, mask_seed, ksk_body, ksk_rows, s["n"])
    return bk, ksk


def generate_compressed(backend, noise_seed=None, mask_seed=None, bk_stdev=None, ks_stdev=None, load=True):
    """Secret keys of domains 1 / 2 of the private noise_seed (default os.urandom(32)) and the bodies of a compressed evaluation key
    generated on the backend's device under the public mask_seed (default os.urandom(32); must differ from noise_seed)
    -> (client.SecretKeySet without an evaluation key, CompressedKey with CUDA-tensor bodies). load=True also makes it the
    backend's key (rs_load_compressed_keys_dev). Client-side operation: see INTEGRATION.md section 11."""
    p = backend.p
    name = set_name(p)
    s = _shape(name, p.n)
    noise_seed = os.urandom(32) if noise_seed is None else bytes(noise_seed)
    mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
    bk_stdev = s["bk_stdev"] if bk_stdev is None else bk_stdev
    ks_stdev = s["ks_stdev"] if ks_stdev is None else ks_stdev
    lwe, tlwe = secret_keys(name, noise_seed, p.n)
    bk_body, ksk_body = backend.keygen_compressed(lwe, tlwe, mask_seed, noise_seed, bk_stdev, ks_stdev)
    if load:
        backend.load_compressed_keys(mask_seed, bk_body, ksk_body)
    return client.SecretKeySet.from_secret(name, lwe, tlwe), CompressedKey(name, p.n, mask_seed, bk_body, ksk_body)


# ---- seeded LWE ciphertexts ----

def _ct_rows(first, B):
    """Rows first .. first + B - 1 as uint64 (first + B must not pass 2^64)."""
    first, B = int(first), int(B)
    if first < 0 or B < 0 or first + B > 1 << 64:
        raise ValueError("first + B = %d + %d passes 2^64" % (first, B))
    return np.uint64(first) + np.arange(B, dtype=np.uint64) if B else np.zeros(0, np.uint64)


def ct_masks(mask_seed, n, first, B, chunk=None):
    """Mask words of ciphertexts first .. first + B - 1: the domain-7 words of the mask seed -> uint32 [B][n]."""
    n = int(n)
    rows = _ct_rows(first, B)
    chunk = chunk or max(1, (1 << 18) // ((n + 15) // 16))
    key = _seed_words(mask_seed)
    blocks = np.arange((n + 15) // 16, dtype=np.uint32)
    out = np.empty((len(rows), n), np.uint32)
    for lo in range(0, len(rows), chunk):
        r = rows[lo:lo + chunk]
        out[lo:lo + chunk] = _chacha_blocks(key, DOMAIN_CT_MASK, r[:, None], blocks[None, :]).reshape(len(r), -1)[:, :n]
    return out


def ct_noise(noise_seed, first, B, stdev):
    """Noise words of ciphertexts first .. first + B - 1: Gaussian 0 of the domain-8 stream of the noise seed -> int32 [B]."""
    rows = _ct_rows(first, B)
    if stdev == 0 or len(rows) == 0:
        return np.zeros(len(rows), np.int32)
    w = _chacha_blocks(_seed_words(noise_seed), DOMAIN_CT_NOISE, rows, np.uint32(0))[:, :4]
    return noise32(w, stdev)[:, 0]


def _check_seeds(mask_seed, noise_seed):
    if bytes(mask_seed) == bytes(noise_seed):
        raise ValueError("mask seed and noise seed are equal: the public mask seed would reveal the noise")


def encrypt_seeded(lwe_key, mu, mask_seed, noise_seed, first=0, stdev=client.SECALPHA):
    """Bodies of seeded ciphertexts of the torus words mu [B] under lwe_key (rs_encrypt_seeded_dev restated) -> int32 [B]."""
    _check_seeds(mask_seed, noise_seed)
    lwe = np.asarray(lwe_key, np.int64).ravel()
    mu = np.asarray(mu).astype(np.int64).ravel()
    a = ct_masks(mask_seed, lwe.size, first, mu.size).astype(np.uint64)
    dot = (a * lwe.astype(np.uint64)).sum(axis=-1) if mu.size else np.zeros(0, np.uint64)
    e = ct_noise(noise_seed, first, mu.size, stdev).view(np.uint32).astype(np.uint64)
    return ((dot + e + (mu & 0xFFFFFFFF).astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def expand_ciphertexts(mask_seed, body, n, first=0):
    """The full samples of seeded ciphertexts (rs_expand_ciphertexts_dev restated): the domain-7 masks beside the bodies
    -> int32 [B][n+1]."""
    body = np.asarray(body, np.int32).ravel()
    out = np.empty((body.size, int(n) + 1), np.int32)
    out[:, :int(n)] = ct_masks(mask_seed, n, first, body.size).view(np.int32)
    out[:, int(n)] = body
    return out


# ---- public-key encryption (rs_pk_encrypt_dev restated) ----

def pk_rows(n):
    """Default number m of rows of a public key for LWE dimension n: n log q + 2 lambda with q = 2^32 and lambda = 128 (the textbook
    leftover-hash-lemma size), counting the body word: 32 (n + 1) + 256."""
    return 32 * (int(n) + 1) + 256


def pk_selection(rand_seed, m, first, B):
    """Selection bits of ciphertexts first .. first + B - 1 over m public-key rows: the domain-9 stream of the rand seed, bit j =
    bit j & 31 of word j >> 5 -> uint8 [B][m] of 0 / 1."""
    m = int(m)
    if not 1 <= m <= (1 << 31) - 1:
        raise ValueError("m = %d is outside 1 .. 2^31 - 1" % m)
    rows = _ct_rows(first, B)
    words = chacha20_words(rand_seed, DOMAIN_PK_SELECT, rows, (m + 31) // 32).reshape(len(rows), -1)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return bits.reshape(len(rows), -1)[:, :m].astype(np.uint8)


def pk_encrypt(pk, mu, rand_seed, first=0, base=None, B=None):
    """rs_pk_encrypt_dev restated: ct[i] = base[i] + (0, mu[i]) + the rows of pk (int32 [m][n+1], encryptions of zero) whose selection
    bit is set for ciphertext i -> int32 [B][n+1]. mu [B] and base [B][n+1] may each be None; B is taken from mu, else base, else B.
    The subset sums are taken as exact float64 products of the 0 / 1 matrix with the 16-bit halves of the rows (every partial sum stays
    below m 2^16 < 2^53), nothing like the device's integer adds."""
    pk = np.ascontiguousarray(pk, np.int32)
    assert pk.ndim == 2 and pk.shape[0] >= 1, "pk must hold [m][n+1] words"
    m, W = pk.shape
    if mu is not None:
        mu = np.asarray(mu).astype(np.int64).ravel()
        B = mu.size
    if base is not None:
        base = np.asarray(base, np.int32).reshape(-1, W)
        B = base.shape[0] if mu is None else B
        assert base.shape[0] == B, "base must hold [B][n+1] words"
    B = int(B or 0)
    u = pk.view(np.uint32)
    lo, hi = (u & np.uint32(0xFFFF)).astype(np.float64), (u >> np.uint32(16)).astype(np.float64)
    out = np.empty((B, W), np.uint64)
    for i0 in range(0, B, 256):
        sel = pk_selection(rand_seed, m, int(first) + i0, min(256, B - i0)).astype(np.float64)
        out[i0:i0 + 256] = (sel @ lo).astype(np.uint64) + ((sel @ hi).astype(np.uint64) << np.uint64(16))
    if base is not None:
        out += base.view(np.uint32)
    if mu is not None:
        out[:, W - 1] += (mu & 0xFFFFFFFF).astype(np.uint64)
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


# ---- compact RLWE public keys (rs_rlwe_pk_encrypt_dev / rs_rlwe_extract_dev restated) ----

MIN_STDEV = 2.0 ** -31   # below this dtot32 truncates most noise words to zero: a noise-free (a, a*S) publishes S by linear algebra


def rlwe_default_stdev(name):
    """The default deviation of an RLWE public key and of its ciphertexts: the set's bk_stdev (the ring's alpha). ValueError on the
    sets whose bk_stdev truncates to zero in a 32-bit torus (redsec_medium, redsec_large): they need an explicit stdev."""
    stdev = _shape(name)["bk_stdev"]
    if stdev < MIN_STDEV:
        raise ValueError("the bk_stdev of %s (%.3g) truncates to zero in a 32-bit torus and a noise-free key publishes the secret: "
                         "pass an explicit stdev >= 2^-31" % (name, stdev))
    return stdev


def rlwe_pk_mask(mask_seed, N):
    """The mask polynomial a of an RLWE public key: words 0 .. N-1 of stream (10, 0) of the mask seed -> int32 [N]."""
    return chacha20_words(mask_seed, DOMAIN_RLWE_MASK, 0, int(N)).view(np.int32)


def rlwe_public_key(name, tlwe_key, mask_seed, noise_seed, stdev=None):
    """The body b = a*S + e (negacyclic, mod 2^32) of the RLWE public key of the ring secret tlwe_key: a = rlwe_pk_mask(mask_seed, N),
    e = the N Gaussians of stream (11, 0) of the private noise seed -> int32 [N]. stdev defaults to rlwe_default_stdev(name)."""
    _check_seeds(mask_seed, noise_seed)
    stdev = rlwe_default_stdev(name) if stdev is None else float(stdev)
    N = _shape(name)["N"]
    S = np.asarray(tlwe_key).ravel()
    assert S.size == N, "tlwe_key must have N = %d words" % N
    a = rlwe_pk_mask(mask_seed, N).view(np.uint32)
    b = _times_binary(a[None, :], S)[0]
    with np.errstate(over="ignore"):
        b = b + noise32(chacha20_words(noise_seed, DOMAIN_RLWE_NOISE, 0, 4 * N), stdev).view(np.uint32)
    return b.view(np.int32)


def _rlwe_rows(first, count, N):
    count = int(count)
    if count < 0:
        raise ValueError("count = %d is negative" % count)
    return _ct_rows(first, -(-count // int(N)))


def rlwe_pk_selector(rand_seed, N, first, R):
    """The binary polynomials u of ciphertexts first .. first + R - 1: the domain-12 stream of the rand seed, u_k = bit k & 31 of word
    k >> 5 -> uint8 [R][N] of 0 / 1."""
    rows = _ct_rows(first, R)
    words = chacha20_words(rand_seed, DOMAIN_RLWE_SELECT, rows, int(N) // 32).reshape(len(rows), -1)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return bits.reshape(len(rows), -1).astype(np.uint8)


def rlwe_pk_noise(rand_seed, N, first, R, stdev):
    """(e1, e2) of ciphertexts first .. first + R - 1: Gaussians 0 .. N-1 and N .. 2N-1 of stream (13, row) -> int32 [R][2][N]."""
    rows = _ct_rows(first, R)
    if stdev == 0 or len(rows) == 0:
        return np.zeros((len(rows), 2, int(N)), np.int32)
    return noise32(chacha20_words(rand_seed, DOMAIN_RLWE_ENC_NOISE, rows, 8 * int(N)), stdev).reshape(len(rows), 2, int(N))


def rlwe_pk_encrypt(pk, mu, rand_seed, first=0, *, stdev):
    """rs_rlwe_pk_encrypt_dev restated: ciphertext r = (a*u_r + e1, b*u_r + e2 + m_r) for pk = (a, b) int32 [2][N] and the torus words
    mu [count], N per ciphertext, the last one padded with zeros -> int32 [ceil(count / N)][2][N]. The products are _times_binary's
    (float64 matrix products on 16-bit halves for N <= 1024, shifted slices above): nothing like the device's tiled integer adds."""
    pk = np.ascontiguousarray(pk, np.int32)
    assert pk.ndim == 2 and pk.shape[0] == 2, "pk must hold [2][N] words"
    N = pk.shape[1]
    mu = np.asarray(mu).astype(np.int64).ravel()
    rows = _rlwe_rows(first, mu.size, N)
    R = len(rows)
    m = np.zeros(R * N, np.uint32)
    m[:mu.size] = (mu & 0xFFFFFFFF).astype(np.uint32)
    out = np.empty((R, 2, N), np.uint32)
    for r in range(R):
        u = rlwe_pk_selector(rand_seed, N, int(rows[r]), 1)[0]
        out[r] = _times_binary(pk.view(np.uint32), u)
    with np.errstate(over="ignore"):
        out += rlwe_pk_noise(rand_seed, N, first, R, stdev).view(np.uint32)
        out[:, 1, :] += m.reshape(R, N)
    return out.view(np.int32)


def rlwe_extract(rlwe, count):
    """rs_rlwe_extract_dev restated: sample i = rN + c is the LWE sample of coefficient c of ciphertext r under the ring key read as
    an LWE key -> int32 [count][N+1]."""
    rlwe = np.ascontiguousarray(rlwe, np.int32)
    N = rlwe.shape[-1]
    rlwe = rlwe.reshape(-1, 2, N)
    count = int(count)
    assert 0 <= count <= rlwe.shape[0] * N, "count exceeds the slots of the ciphertexts"
    out = np.empty((count, N + 1), np.int32)
    j = np.arange(N)[None, :]
    with np.errstate(over="ignore"):
        for r in range(-(-count // N)):
            c = np.arange(min(N, count - r * N))[:, None]
            words = rlwe[r, 0].view(np.uint32)[(c - j) % N]
            out[r * N:r * N + len(c), :N] = np.where(j > c, np.uint32(0) - words, words).view(np.int32)
            out[r * N:r * N + len(c), N] = rlwe[r, 1, :len(c)]
    return out


def rlwe_phase(rlwe, tlwe_key):
    """Phases b' - a'*S of RLWE ciphertexts [R][2][N] under the ring secret -> int32 [R][N]."""
    rlwe = np.ascontiguousarray(rlwe, np.int32)
    N = rlwe.shape[-1]
    rlwe = rlwe.reshape(-1, 2, N).view(np.uint32)
    with np.errstate(over="ignore"):
        return (rlwe[:, 1] - _times_binary(np.ascontiguousarray(rlwe[:, 0]), np.asarray(tlwe_key).ravel())).view(np.int32)


# ---- packed results (rs_pack_dev restated) ----

def pack_default(name):
    """(basebit, t) of a set's packing key: basebit 4; t = 4 (16 bits) where results are +-1/8 bits (default-128), t = 5 (20 bits) on
    the REDsec sets, whose 1/4096-scale values need the digits' rounding sqrt(n / 24) 2^(-t basebit) well under the half step 1.2e-4
    (16 bits: 7e-5; 20 bits: 4e-6)."""
    _shape(name)
    return (4, 4) if name == "default128" else (4, 5)


def _check_digits(basebit, t):
    basebit, t = int(basebit), int(t)
    if not (1 <= basebit <= 8 and t >= 1 and t * basebit <= 32):
        raise ValueError("basebit = %d, t = %d: basebit must lie in 1 .. 8, t >= 1 and t basebit <= 32" % (basebit, t))
    return basebit, t


def pack_key_mask(mask_seed, N, rows):
    """The mask polynomials a_ij of packing-key rows i t + j: words 0 .. N-1 of stream (14, row) of the mask seed -> int32 [R][N]."""
    rows = np.asarray(rows, np.int64).ravel()
    return chacha20_words(mask_seed, DOMAIN_PACK_MASK, rows.astype(np.uint64), int(N)).reshape(len(rows), int(N)).view(np.int32)


def pack_key(name, lwe_key, tlwe_key, mask_seed, noise_seed, basebit, t, stdev=None, rows=None, chunk=256):
    """The bodies b_ij = a_ij*S + e_ij + s_i 2^(32-(j+1) basebit) X^0 of the packing key from lwe_key to tlwe_key: a_ij =
    pack_key_mask(mask_seed, N, i t + j), e_ij the N Gaussians of stream (15, i t + j) of the private noise seed -> int32 [n][t][N]
    (rows=None), or [len(rows)][N] for the rows i t + j listed. The LWE dimension is len(lwe_key). stdev defaults to
    rlwe_default_stdev(name): the ring's alpha, refused where it truncates to zero."""
    _check_seeds(mask_seed, noise_seed)
    basebit, t = _check_digits(basebit, t)
    stdev = rlwe_default_stdev(name) if stdev is None else float(stdev)
    N = _shape(name)["N"]
    lwe = np.asarray(lwe_key).ravel().astype(np.uint32)
    S = np.asarray(tlwe_key).ravel()
    assert S.size == N, "tlwe_key must have N = %d words" % N
    whole = rows is None
    rows = np.arange(lwe.size * t) if whole else np.asarray(rows, np.int64).ravel()
    out = np.empty((len(rows), N), np.int32)
    with np.errstate(over="ignore"):
        for lo in range(0, len(rows), chunk):
            r = rows[lo:lo + chunk]
            B = _times_binary(np.ascontiguousarray(pack_key_mask(mask_seed, N, r)).view(np.uint32), S)
            if stdev:
                B += noise32(chacha20_words(noise_seed, DOMAIN_PACK_NOISE, r.astype(np.uint64), 4 * N), stdev).reshape(len(r), N).view(np.uint32)
            B[:, 0] += lwe[r // t] * (np.uint32(1) << (32 - (r % t + 1) * basebit).astype(np.uint32))
            out[lo:lo + chunk] = B.view(np.int32)
    return out.reshape(lwe.size, t, N) if whole else out


def pack_key_noise(name, lwe_key, tlwe_key, key, basebit, t, mask_seed=None, rows=None, chunk=256):
    """rs_audit_pack_key_dev restated: the noise words e = b - a*S - s_i 2^(32-(j+1) basebit) X^0 of packing-key rows i t + j (all n t
    rows if rows is None) -> int32 [R][N]. Full key (mask_seed None): key holds the rows [R][2][N]; with a mask seed key holds the
    body rows [R][N] and the masks are pack_key_mask's. The LWE dimension is len(lwe_key). A key of pack_key returns exactly its
    domain-15 noise32 words."""
    basebit, t = _check_digits(basebit, t)
    N = _shape(name)["N"]
    lwe = np.asarray(lwe_key).ravel().astype(np.uint32)
    S = np.asarray(tlwe_key).ravel()
    assert S.size == N, "tlwe_key must have N = %d words" % N
    rows = np.arange(lwe.size * t) if rows is None else np.asarray(rows, np.int64).ravel()
    stored = np.asarray(key, np.int32).reshape(len(rows), -1, N)
    assert stored.shape[1] == (2 if mask_seed is None else 1), "stored rows have the wrong shape"
    out = np.empty((len(rows), N), np.int32)
    with np.errstate(over="ignore"):
        for lo in range(0, len(rows), chunk):
            r = rows[lo:lo + chunk]
            A = stored[lo:lo + chunk, 0] if mask_seed is None else pack_key_mask(mask_seed, N, r)
            E = np.ascontiguousarray(stored[lo:lo + chunk, -1]).view(np.uint32) - _times_binary(np.ascontiguousarray(A).view(np.uint32), S)
            E[:, 0] -= lwe[r // t] * (np.uint32(1) << (32 - (r % t + 1) * basebit).astype(np.uint32))
            out[lo:lo + chunk] = E.view(np.int32)
    return out


def pack_noise_limit(stdev):
    """Default limit of the packing-key audit = floor(8.58 stdev 2^32) + 1: the bound of noise_limits (|z| <= 8.572), not a statistic."""
    return int(np.floor(GAUSS_BOUND * float(stdev) * 2.0 ** 32)) + 1


def pack_digits(a, basebit, t):
    """The t digits of the mask words a (any shape, int32 / uint32) in lweKeySwitch's convention: abar = a + 2^(31 - t basebit) (no
    offset at 32 bits), digit j = (abar >> (32 - (j+1) basebit)) & (2^basebit - 1) -> uint32 [..., t]."""
    basebit, t = _check_digits(basebit, t)
    a = np.asarray(a).astype(np.int64) & 0xFFFFFFFF
    off = (1 << (31 - t * basebit)) if t * basebit < 32 else 0
    abar = (a + off) & 0xFFFFFFFF
    return np.stack([(abar >> (32 - (j + 1) * basebit)) & ((1 << basebit) - 1) for j in range(t)], axis=-1).astype(np.uint32)


def pack(ct, key, basebit, t):
    """rs_pack_dev restated: ct int32 [count][n+1], key int32 [n][t][2][N] -> int32 [ceil(count / N)][2][N], ciphertext r =
    (0, sum_c b_(rN+c) X^c) - sum_{i,j} D_ij(X) K[i][j]. Per polynomial the sum over the n t rows is ONE float64 matrix product per
    16-bit half of the key words, G[c][x] = sum_rows digit[row][c] ext[row][x] over ext = (-p, p) (every entry below 2^8 2^16 n t
    < 2^53: exact), and coefficient k is the sum over c of G[c][k - c + N], taken in 64-bit integers: nothing like the device's tiled
    32-bit multiply-adds."""
    basebit, t = _check_digits(basebit, t)
    key = np.ascontiguousarray(key, np.int32)
    assert key.ndim == 4 and key.shape[1] == t and key.shape[2] == 2, "key must hold [n][t][2][N] words"
    n, N = key.shape[0], key.shape[3]
    assert n * t < 1 << 28, "n t is too large for the exact float64 sums"
    ct = np.ascontiguousarray(ct, np.int32).reshape(-1, n + 1)
    count = ct.shape[0]
    R = -(-count // N)
    out = np.zeros((R, 2, N), np.uint32)
    if count == 0:
        return out.view(np.int32)
    ku = key.view(np.uint32).reshape(n * t, 2, N)
    halves = []
    for poly in range(2):
        ext = np.concatenate([np.uint32(0) - ku[:, poly], ku[:, poly]], axis=1)                   # [n t][2N]
        halves.append(((ext & np.uint32(0xFFFF)).astype(np.float64), (ext >> np.uint32(16)).astype(np.float64)))
    step = max(4, (1 << 22) // (2 * N))                                                        # slots per product: G of 32 MB
    for r in range(R):
        rows = ct[r * N:(r + 1) * N]
        cr = rows.shape[0]
        out[r, 1, :cr] = rows[:, n].view(np.uint32)
        D = pack_digits(rows[:, :n], basebit, t).reshape(cr, n * t).astype(np.float64)          # [c][i t + j]
        for poly in range(2):
            acc = np.zeros(N, np.uint64)
            for c0 in range(0, cr, step):
                d = D[c0:c0 + step]
                G = (d @ halves[poly][0]).astype(np.uint64) + ((d @ halves[poly][1]).astype(np.uint64) << np.uint64(16))
                flat = np.ascontiguousarray(G).ravel()
                # element (c, k) = G[c][k - (c0 + c) + N] = flat[c (2N - 1) + N - c0 + k]
                view = np.lib.stride_tricks.as_strided(flat[N - c0:], shape=(len(d), N), strides=((2 * N - 1) * 8, 8))
                acc += view.sum(axis=0, dtype=np.uint64)
            with np.errstate(over="ignore"):
                out[r, poly] -= (acc & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out.view(np.int32)


def pack_sigma(n, N, basebit, t, count, stdev):
    """Deviation of the packing error of one slot, as a real in [-1/2, 1/2): the key noise under the n t digit polynomials of
    count_r = min(count, N) slots (a uniform digit has mean square (2^basebit - 1)(2^(basebit+1) - 1) / 6) and the rounding of the
    digits over the n / 2 set key bits:
      sigma^2 = n t count_r (2^basebit - 1)(2^(basebit+1) - 1)/6 sigma_k^2  +  (n/2) 2^(-2 t basebit)/12"""
    basebit, t = _check_digits(basebit, t)
    cr = min(int(count), int(N))
    base = 1 << basebit
    return float(np.sqrt(n * t * cr * (base - 1) * (2 * base - 1) / 6.0 * float(stdev) ** 2 + (n / 2.0) * 2.0 ** (-2 * t * basebit) / 12.0))


# ---- re-keying (rs_rekey_dev restated) ----

def rekey_default(dst_name):
    """(basebit, t) of a re-keying key whose destination is a secret of set dst_name: (2, 8) to default-128, whose rows carry the
    set's ks_stdev 2^-15 and whose results are +-1/8 bits (8 rekey_sigma stays below 1/16 from n_src = 630); (4, 5) to
    redsec_small_v2 and redsec_small, (4, 6) to redsec_medium and redsec_large, whose 1/4096-scale values need 8 rekey_sigma below
    the half step 1/8192 from a source of the set's own n (20 bits of digits leave the rounding sqrt(n_src / 24) 2^-20 alone at
    1.5e-5 from n_src = 6144). INTEGRATION.md section 21 has the table."""
    _shape(dst_name)
    return (2, 8) if dst_name == "default128" else (4, 6) if dst_name in ("redsec_medium", "redsec_large") else (4, 5)


def rekey_row_stdev(dst_name):
    """The default deviation of a seeded row of a re-keying key under a secret of dst_name: the set's ks_stdev, the deviation of
    the rows of its own keyswitching key. ValueError where that truncates to zero in a 32-bit torus (redsec_medium, redsec_large)."""
    stdev = _shape(dst_name)["ks_stdev"]
    if stdev < MIN_STDEV:
        raise ValueError("the ks_stdev of %s (%.3g) truncates to zero in a 32-bit torus and noise-free rows publish the secret: "
                         "pass an explicit stdev >= 2^-31" % (dst_name, stdev))
    return stdev


def rekey_messages(lwe_key, basebit, t):
    """The torus words a re-keying key encrypts: s_i 2^(32-(j+1) basebit) at row i t + j -> int32 [n_src t]."""
    basebit, t = _check_digits(basebit, t)
    s = np.asarray(lwe_key).ravel().astype(np.uint32)
    g = (np.uint32(1) << (32 - (np.arange(t) + 1) * basebit).astype(np.uint32)).astype(np.uint32)
    return (s[:, None] * g[None, :]).ravel().view(np.int32)


def rekey_alternate(rows):
    """The odd rows negated mod 2^32 (its own inverse): rows int32 [R] (messages) or [R][W] (samples) -> the same shape. A key made
    under an RLWE public key carries row r in slot r of a ciphertext whose N slots share one selector u and the key's and the
    ciphertext's noise polynomials; a binary u has mean 1/2, so the noise of neighbouring slots has a common part, fixed by the key,
    which the unsigned digits (mean (2^basebit - 1) / 2) would add up over all n_src t rows into an offset of many rekey_sigma
    (measured: up to 40 at n_src = 350, (4, 5)). Encrypting every other row negated and negating it back after the extraction
    makes the common part cancel in pairs; what is left fits rekey_sigma."""
    out = np.array(rows, np.int32, copy=True)
    with np.errstate(over="ignore"):
        out[1::2] = (np.uint32(0) - out[1::2].view(np.uint32)).view(np.int32)
    return out


def rekey(ct, key, basebit, t):
    """rs_rekey_dev restated: ct int32 [B][n_src+1], key int32 [n_src][t][n_dst+1] -> int32 [B][n_dst+1], out[r] = (0, b_r) -
    sum_{i,j} d_ij(r) K[i][j]. The sum over the n_src t rows is ONE float64 matrix product per 16-bit half of the key words (every
    entry below 2^8 2^16 n_src t < 2^53: exact), recombined in 64-bit integers: nothing like the device's tiled 32-bit multiply-adds."""
    basebit, t = _check_digits(basebit, t)
    key = np.ascontiguousarray(key, np.int32)
    assert key.ndim == 3 and key.shape[1] == t, "key must hold [n_src][t][n_dst+1] words"
    n_src, W = key.shape[0], key.shape[2]
    assert W >= 2 and n_src * t < 1 << 28, "key rows need n_dst >= 1 and n_src t below 2^28"
    ct = np.ascontiguousarray(ct, np.int32).reshape(-1, n_src + 1)
    B = ct.shape[0]
    out = np.zeros((B, W), np.uint64)
    ku = key.view(np.uint32).reshape(n_src * t, W)
    lo, hi = (ku & np.uint32(0xFFFF)).astype(np.float64), (ku >> np.uint32(16)).astype(np.float64)
    for r0 in range(0, B, 4096):
        D = pack_digits(ct[r0:r0 + 4096, :n_src], basebit, t).reshape(-1, n_src * t).astype(np.float64)      # [r][i t + j]
        out[r0:r0 + 4096] = (D @ lo).astype(np.uint64) + ((D @ hi).astype(np.uint64) << np.uint64(16))
    with np.errstate(over="ignore"):
        out = np.uint64(0) - out
        out[:, W - 1] += ct[:, n_src].view(np.uint32)
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def rekey_sigma(n_src, basebit, t, sigma_row):
    """Deviation of the re-keying error of one sample, as a real in [-1/2, 1/2): the noise of the n_src t key rows under the
    digits (a uniform digit has mean square (2^basebit - 1)(2^(basebit+1) - 1) / 6) and the rounding of the digits over the n_src / 2
    set key bits. sigma_row is the deviation of one key row's phase: the stdev of a seeded row, stdev sqrt(N + 1) for a row made
    under an RLWE public key.
      sigma^2 = n_src t (2^basebit - 1)(2^(basebit+1) - 1)/6 sigma_row^2  +  (n_src/2) 2^(-2 t basebit)/12"""
    basebit, t = _check_digits(basebit, t)
    base = 1 << basebit
    return float(np.sqrt(n_src * t * (base - 1) * (2 * base - 1) / 6.0 * float(sigma_row) ** 2 + (n_src / 2.0) * 2.0 ** (-2 * t * basebit) / 12.0))


# ---- ring re-keying (rs_ring_rekey_dev restated) ----

RING_REKEY_MAX_BITS = 31   # t basebit <= 31: h_j = 2^(31 - (j+1) basebit) is an integer


def _check_ring_digits(basebit, t):
    basebit, t = _check_digits(basebit, t)
    if t * basebit > RING_REKEY_MAX_BITS:
        raise ValueError("basebit = %d, t = %d: a ring re-keying key needs t basebit <= 31" % (basebit, t))
    return basebit, t


def ring_rekey_default(name, form="seeded"):
    """(basebit, t) of a ring re-keying key to a secret of set `name`, per key form ("seeded" rows of the ring's alpha, or "rlwe" rows
    made from an RLWE public key, alpha sqrt(N + 1)), chosen so that 8 ring_rekey_sigma stays inside the use of the re-keyed phase:
    1/8 for default-128's +-1/8 bits, the half step 1/8192 for the networks' 1/4096-scale values. (2, 8) for default-128 in both
    forms; seeded: (4, 5) at N = 1024 and (4, 6) at N = 4096 and 8192 (20 bits leave the rounding sqrt(N / 24) 2^-20 alone at
    1.8e-5 on the large ring); rlwe: (2, 12) for redsec_small_v2 and redsec_small and (1, 24) for redsec_medium, whose wider row
    noise needs the small digits. No shape reaches 8 sigma for redsec_large in the rlwe form. INTEGRATION.md section 22 has the
    table."""
    N = _shape(name)["N"]
    if form not in ("seeded", "rlwe"):
        raise ValueError("form must be 'seeded' or 'rlwe', not %r" % (form,))
    if name == "default128":
        return (2, 8)
    if form == "seeded":
        return (4, 5) if N <= 1024 else (4, 6)
    return (2, 12) if N <= 1024 else (1, 24)


def ring_rekey_messages(tlwe_key, basebit, t):
    """The torus polynomials a ring re-keying key encrypts -> int32 [t+1][N]: row j < t is h_j S, h_j = 2^(31-(j+1) basebit); row t
    is c0 (1 + X + ... + X^(N-1)) S (negacyclic), c0 = (2^basebit - 1) sum_j h_j, what the centring of the digits took away. The
    rows hold the source secret: zero them after use."""
    basebit, t = _check_ring_digits(basebit, t)
    S = np.asarray(tlwe_key).ravel().astype(np.int64)
    N = S.size
    h = [1 << (31 - (j + 1) * basebit) for j in range(t)]
    out = np.empty((t + 1, N), np.int64)
    for j in range(t):
        out[j] = S * h[j]
    # coefficient k of (1 + X + ... + X^(N-1)) S: the bits at or below k minus the bits above k
    below = np.cumsum(S)
    out[t] = (2 * below - below[-1]) * (((1 << basebit) - 1) * sum(h))
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def ring_rekey_digits(a, basebit, t):
    """The odd digits d_j(k) = 2 ((abar_k >> (32-(j+1) basebit)) & (2^basebit - 1)) - (2^basebit - 1), abar = a + 2^(31 - t basebit),
    of mask polynomials a int32 [..., N] -> int64 [..., t, N]."""
    basebit, t = _check_ring_digits(basebit, t)
    abar = (np.asarray(a, np.int32).view(np.uint32).astype(np.int64) + (1 << (31 - t * basebit))) & 0xFFFFFFFF
    B1 = (1 << basebit) - 1
    return np.stack([2 * ((abar >> (32 - (j + 1) * basebit)) & B1) - B1 for j in range(t)], axis=-2)


def _negacyclic(d, p):
    """d(X) p(X) mod X^N + 1 for int64 d (|d| < 2^9) and words p (below 2^32) as int64: every sum stays below 2^54 -> int64 [N]."""
    N = d.size
    c = np.convolve(d, p)
    out = c[:N].copy()
    out[:N - 1] -= c[N:]
    return out


def ring_rekey(rlwe, key, basebit, t, unsigned=False):
    """rs_ring_rekey_dev restated: rlwe int32 [R][2][N], key int32 [t+1][2][N] -> int32 [R][2][N], out[r] = (0, b_r) - K[t] -
    sum_j D_j(X) K[j]. Each product is one int64 linear convolution folded negacyclically (numpy.convolve): nothing like the
    device's tiled 32-bit multiply-adds. unsigned=True is NOT the device's convention: the unsigned digits of rs_pack_dev /
    rs_rekey_dev over rows that encrypt 2^(32-(j+1) basebit) S, and no constant row (K[t] is ignored); kept to show what a digit
    polynomial with a mean does to a key made from an RLWE public key."""
    basebit, t = _check_ring_digits(basebit, t)
    key = np.ascontiguousarray(key, np.int32)
    assert key.ndim == 3 and key.shape[0] == t + 1 and key.shape[1] == 2, "key must hold [t+1][2][N] words"
    N = key.shape[2]
    rlwe = np.ascontiguousarray(rlwe, np.int32).reshape(-1, 2, N)
    ku = key.view(np.uint32).astype(np.int64)
    D = ring_rekey_digits(rlwe[:, 0], basebit, t)
    if unsigned:
        D = (D + ((1 << basebit) - 1)) >> 1
    out = np.zeros(rlwe.shape, np.int64)
    out[:, 1] = rlwe[:, 1].view(np.uint32)
    if not unsigned:
        out -= ku[t]
    for r in range(rlwe.shape[0]):
        for j in range(t):
            for poly in range(2):
                out[r, poly] = (out[r, poly] - _negacyclic(D[r, j], ku[j, poly])) & 0xFFFFFFFF
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def ring_rekey_mask(mask_seed, N, rows):
    """The mask polynomials a_j of ring re-keying rows: words 0 .. N-1 of stream (16, row) of the mask seed -> int32 [R][N]."""
    rows = np.asarray(rows, np.int64).ravel()
    return chacha20_words(mask_seed, DOMAIN_RING_REKEY_MASK, rows.astype(np.uint64), int(N)).reshape(len(rows), int(N)).view(np.int32)


def ring_rekey_key(src_tlwe_key, dst_tlwe_key, mask_seed, noise_seed, basebit, t, stdev):
    """The bodies b_j = a_j*S' + e_j + m_j of the seeded ring re-keying key from the ring secret S = src_tlwe_key to S' =
    dst_tlwe_key -> int32 [t+1][N]: a_j = ring_rekey_mask(mask_seed, N, j), e_j the N Gaussians of stream (17, j) of the private
    noise seed, m = ring_rekey_messages(S, basebit, t). The t + 1 products by the binary S' run here (_times_binary): the key is
    t + 1 rows, there is no device generator. Equal seeds are refused."""
    _check_seeds(mask_seed, noise_seed)
    basebit, t = _check_ring_digits(basebit, t)
    S, S2 = np.asarray(src_tlwe_key).ravel(), np.asarray(dst_tlwe_key).ravel()
    N = S.size
    if S2.size != N:
        raise ValueError("source and destination rings differ: N = %d and %d (crossing between rings is out of scope)" % (N, S2.size))
    rows = np.arange(t + 1)
    B = _times_binary(np.ascontiguousarray(ring_rekey_mask(mask_seed, N, rows)).view(np.uint32), S2)
    mu = ring_rekey_messages(S, basebit, t)
    with np.errstate(over="ignore"):
        if stdev:
            B += noise32(chacha20_words(noise_seed, DOMAIN_RING_REKEY_NOISE, rows.astype(np.uint64), 4 * N), stdev).reshape(t + 1, N).view(np.uint32)
        B += mu.view(np.uint32)
    mu[...] = 0
    return B.view(np.int32)


def ring_rekey_expand(mask_seed, body):
    """[t+1][2][N], what rs_ring_rekey_dev takes, from the public mask seed and the bodies int32 [t+1][N]."""
    body = np.ascontiguousarray(body, np.int32)
    assert body.ndim == 2, "body must hold [t+1][N] words"
    return np.ascontiguousarray(np.stack([ring_rekey_mask(mask_seed, body.shape[1], np.arange(body.shape[0])), body], axis=1))


def ring_rekey_sigma(N, basebit, t, sigma_row):
    """Deviation of the ring re-keying error of one coefficient, as a real in [-1/2, 1/2): the noise of the t key rows under the N
    odd digits of each (a uniform odd digit has mean square (4^basebit - 1)/3), the constant row once, and the rounding of abar
    to t basebit bits over the N / 2 set key bits. sigma_row is the deviation of one key row's phase per coefficient: the stdev of
    a seeded row, stdev sqrt(N + 1) for a row made under an RLWE public key.
      sigma^2 = (t N (4^basebit - 1)/3 + 1) sigma_row^2  +  (N/2) 2^(-2 t basebit)/12"""
    basebit, t = _check_ring_digits(basebit, t)
    return float(np.sqrt((t * N * (4.0 ** basebit - 1) / 3.0 + 1.0) * float(sigma_row) ** 2 + (N / 2.0) * 2.0 ** (-2 * t * basebit) / 12.0))


# ---- encrypted selection (rs_ring_cmux_dev / rs_ring_lookup_dev restated) ----

RING_CMUX_MAX_BITS = 31    # l basebit <= 31: the half step 2^(31 - l basebit) is an integer
RING_LOOKUP_MAX_DEPTH = 30
RING_CMUX_USE = 1.0 / 8192   # the half step of the networks' 1/4096-scale values: what 8 sigma has to stay inside


def _check_cmux_digits(basebit, l):
    basebit, l = int(basebit), int(l)
    if not (1 <= basebit <= 8 and l >= 1 and l * basebit <= RING_CMUX_MAX_BITS):
        raise ValueError("basebit = %d, l = %d: basebit must lie in 1 .. 8, l >= 1 and l basebit <= 31" % (basebit, l))
    return basebit, l


def ring_cmux_offset(basebit, l):
    """off = sum_j (B/2) h_j + 2^(31 - l basebit): w + off puts every digit B/2 above the signed one and rounds to nearest."""
    basebit, l = _check_cmux_digits(basebit, l)
    return (sum(1 << (31 - j * basebit) for j in range(l)) + (1 << (31 - l * basebit))) & 0xFFFFFFFF


RING_CMUX_DIGITS = ("signed", "alternating")


def _check_cmux_form(digits):
    if digits not in RING_CMUX_DIGITS:
        raise ValueError("digits = %r: the digit form must be 'signed' or 'alternating'" % (digits,))
    return digits


def ring_cmux_digits(x, basebit, l, digits="signed"):
    """The signed digits dig_j(w) = (((w + off) >> (32-(j+1) basebit)) & (B - 1)) - B/2 of words x int32 [..., N] -> int64
    [..., l, N], each in -B/2 .. B/2 - 1; sum_j dig_j h_j = w rounded to l basebit bits (mod 2^32).
    digits="alternating" (rs_ring_cmux_alt_dev): dig'_j(x_k) = eps_k dig_j(eps_k x_k), eps_k = +1 for even and -1 for odd k, the
    index along the last axis; each in -B/2 .. B/2, the same rounding within the same half step, mean -eps_k / 2."""
    basebit, l = _check_cmux_digits(basebit, l)
    x = np.asarray(x, np.int32).view(np.uint32).astype(np.int64)
    if _check_cmux_form(digits) == "alternating":
        eps = 1 - 2 * (np.arange(x.shape[-1], dtype=np.int64) & 1)
        x = (eps * x) & 0xFFFFFFFF
    xbar = (x + ring_cmux_offset(basebit, l)) & 0xFFFFFFFF
    B = 1 << basebit
    D = np.stack([((xbar >> (32 - (j + 1) * basebit)) & (B - 1)) - B // 2 for j in range(l)], axis=-2)
    return D * eps if digits == "alternating" else D


def ring_cmux(d1, d0, sel, basebit, l, digits="signed"):
    """rs_ring_cmux_dev restated: d0, d1 int32 [R][2][N] (d1 = None: all zero), sel int32 [2l][2][N] -> int32 [R][2][N], out[r] =
    d0[r] + sum_j Da_j(X) sel[j] + sum_j Db_j(X) sel[l+j] over the digits of d1[r] - d0[r]. Each product is one int64 linear
    convolution folded negacyclically (numpy.convolve): nothing like the device's tiled 32-bit multiply-adds. A stride is the
    caller's slice (d0[::2], d1[1::2]). digits="alternating": rs_ring_cmux_alt_dev, the digits of ring_cmux_digits in that form."""
    basebit, l = _check_cmux_digits(basebit, l)
    _check_cmux_form(digits)
    sel = np.ascontiguousarray(sel, np.int32)
    assert sel.ndim == 3 and sel.shape[0] == 2 * l and sel.shape[1] == 2, "sel must hold [2l][2][N] words"
    N = sel.shape[2]
    d0 = np.ascontiguousarray(d0, np.int32).reshape(-1, 2, N)
    with np.errstate(over="ignore"):
        x = (np.uint32(0) - d0.view(np.uint32)) if d1 is None else (np.ascontiguousarray(d1, np.int32).reshape(-1, 2, N).view(np.uint32) - d0.view(np.uint32))
    assert x.shape == d0.shape, "d1 and d0 must hold the same number of ciphertexts"
    D = ring_cmux_digits(x.view(np.int32), basebit, l, digits)    # [R][2][l][N]
    su = sel.view(np.uint32).astype(np.int64)
    out = d0.view(np.uint32).astype(np.int64)
    for r in range(d0.shape[0]):
        for jr in range(2 * l):
            for poly in range(2):
                out[r, poly] = (out[r, poly] + _negacyclic(D[r, jr // l, jr % l], su[jr, poly])) & 0xFFFFFFFF
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def ring_lookup(table, sel, basebit, l, digits="signed"):
    """rs_ring_lookup_dev restated: table int32 [entries][2][N], sel int32 [depth][2l][2][N], entries <= 2^depth -> int32 [2][N]:
    level k is ring_cmux over the pairs (2r, 2r + 1) of the previous level under sel[k]; an unpaired last row meets d1 = None.
    digits="alternating": rs_ring_lookup_alt_dev, every level in that form."""
    basebit, l = _check_cmux_digits(basebit, l)
    _check_cmux_form(digits)
    sel = np.ascontiguousarray(sel, np.int32)
    assert sel.ndim == 4 and sel.shape[1:3] == (2 * l, 2), "sel must hold [depth][2l][2][N] words"
    depth, N = sel.shape[0], sel.shape[3]
    rows = np.ascontiguousarray(table, np.int32).reshape(-1, 2, N)
    if not (1 <= depth <= RING_LOOKUP_MAX_DEPTH and 1 <= rows.shape[0] <= 1 << depth):
        raise ValueError("depth = %d, entries = %d: depth must lie in 1 .. 30 and entries in 1 .. 2^depth" % (depth, rows.shape[0]))
    for k in range(depth):
        pairs = rows.shape[0] // 2
        nxt = [ring_cmux(rows[1:2 * pairs:2], rows[0:2 * pairs:2], sel[k], basebit, l, digits)] if pairs else []
        if rows.shape[0] & 1:
            nxt.append(ring_cmux(None, rows[-1:], sel[k], basebit, l, digits))
        rows = np.concatenate(nxt)
    return rows[0]


def ring_lookup_rows(table, sel, basebit, l, entries, R, row_stride=0, entry_stride=1, per_row=None, digits="signed"):
    """rs_ring_lookup_rows_dev restated (digits="alternating": rs_ring_lookup_rows_alt_dev) as a loop over
    ring_lookup: table int32 ciphertexts [..][2][N], entry e of row q the ciphertext q row_stride + e entry_stride; sel int32
    [depth][2l][2][N] (one hidden index for all rows) or, with per_row (inferred from five dimensions where None),
    [R][depth][2l][2][N] -> int32 [R][2][N], out[q] = ring_lookup of row q's entries under row q's selectors. Nothing like the
    device's levels of all rows at once."""
    basebit, l = _check_cmux_digits(basebit, l)
    _check_cmux_form(digits)
    sel = np.ascontiguousarray(sel, np.int32)
    per_row = sel.ndim == 5 if per_row is None else bool(per_row)
    assert sel.ndim == (5 if per_row else 4) and sel.shape[-3:-1] == (2 * l, 2), "sel must hold [depth][2l][2][N] words ([R][depth].. per row)"
    N = sel.shape[-1]
    entries, R, row_stride, entry_stride = int(entries), int(R), int(row_stride), int(entry_stride)
    if row_stride < 0 or entry_stride < 1:
        raise ValueError("row_stride = %d, entry_stride = %d: row_stride must be at least 0 and entry_stride at least 1" % (row_stride, entry_stride))
    assert not per_row or sel.shape[0] == R, "one selector set per row"
    cts = np.ascontiguousarray(table, np.int32).reshape(-1, 2, N)
    out = np.zeros((R, 2, N), np.int32)
    for q in range(R):
        rows = cts[[q * row_stride + e * entry_stride for e in range(entries)]]
        out[q] = ring_lookup(rows, sel[q] if per_row else sel, basebit, l, digits)
    return out


def ring_trivial(values):
    """Plaintext torus polynomials int32 [..., N] as trivial ring ciphertexts (0, p) -> int32 [..., 2, N]: the rows of a server-held
    plaintext table."""
    p = np.ascontiguousarray(values, np.int32)
    return np.ascontiguousarray(np.stack([np.zeros_like(p), p], axis=-2))


# ---- encrypted rotation (rs_ring_rotate_dev / rs_ring_heads_dev restated) ----

def ring_monomial(rlwe, e):
    """X^e times ring elements int32 [..., N] mod X^N + 1 (both polynomials of a ciphertext [..., 2, N] alike), e any integer: the
    coefficients move up by e mod 2N and change sign each time they pass the top. A concatenate-and-negate, nothing like the
    device's indexing (rs_ring_rotate.h ro_source)."""
    v = np.ascontiguousarray(rlwe, np.int32).view(np.uint32)
    N = v.shape[-1]
    e = int(e) % (2 * N)
    with np.errstate(over="ignore"):
        ext = np.concatenate([v, np.uint32(0) - v], axis=-1)                 # the coefficients of v as a polynomial mod X^2N - 1
        return np.ascontiguousarray(np.roll(ext, e, axis=-1)[..., :N]).view(np.int32)


def ring_rotate(rlwe, sel, step, basebit, l, digits="signed", per_row=False, stride=1):
    """rs_ring_rotate_dev restated (digits="alternating": rs_ring_rotate_alt_dev): rlwe int32 [rows][2][N], read at `stride` (0:
    every row starts from rlwe[0], and R is then the number of selector sets), sel int32 [depth][2l][2][N] (one hidden index for
    all rows) or, with per_row, [R][depth][2l][2][N] -> int32 [R][2][N]. Level k is ring_cmux between the accumulator and
    ring_monomial(accumulator, step 2^k) under sample k, least significant bit first, so phase(out[r]) = X^(step index_r)
    phase(rlwe[r stride]) + noise: step = -1 brings slot `index` to coefficient 0.
    Noise: that of `depth` CMUXes, ring_cmux_sigma(..., depth) for a client's selectors and circuit_bootstrap_sigma(..., depth,
    coefficient=None) for produced ones. Later levels move a level's error to other coefficients and flip signs; they do not grow
    it, so the worst-coefficient deviation per level still bounds every coefficient. There is no formula of its own."""
    basebit, l = _check_cmux_digits(basebit, l)
    _check_cmux_form(digits)
    sel = np.ascontiguousarray(sel, np.int32)
    assert sel.ndim == (5 if per_row else 4) and sel.shape[-3:-1] == (2 * l, 2), "sel must hold [depth][2l][2][N] words ([R][depth].. per row)"
    depth, N = sel.shape[-4], sel.shape[-1]
    if not 1 <= depth <= RING_LOOKUP_MAX_DEPTH:
        raise ValueError("depth = %d is outside 1 .. %d" % (depth, RING_LOOKUP_MAX_DEPTH))
    rows = np.ascontiguousarray(rlwe, np.int32).reshape(-1, 2, N)
    stride = int(stride)
    if stride < 0:
        raise ValueError("stride = %d is below 0" % stride)
    if stride == 0:
        acc = np.repeat(rows[:1], sel.shape[0] if per_row else 1, axis=0)
    else:
        acc = rows[::stride].copy()
    assert not per_row or sel.shape[0] == acc.shape[0], "one selector set per row"
    for k in range(depth):
        turned = ring_monomial(acc, int(step) << k)
        if per_row:
            acc = np.concatenate([ring_cmux(turned[r:r + 1], acc[r:r + 1], sel[r, k], basebit, l, digits) for r in range(acc.shape[0])])
        else:
            acc = ring_cmux(turned, acc, sel[k], basebit, l, digits)
    return acc


def ring_heads(rlwe, width=1):
    """rs_ring_heads_dev restated: sample r width + c is the LWE sample of coefficient c < width of ciphertext r (rlwe_extract's
    formula with the slot index replaced) -> int32 [R width][N+1]."""
    rlwe = np.ascontiguousarray(rlwe, np.int32)
    N = rlwe.shape[-1]
    rlwe = rlwe.reshape(-1, 2, N)
    width = int(width)
    if not 1 <= width <= N:
        raise ValueError("width = %d is outside 1 .. %d" % (width, N))
    out = np.empty((rlwe.shape[0], width, N + 1), np.int32)
    j, c = np.arange(N)[None, :], np.arange(width)[:, None]
    with np.errstate(over="ignore"):
        for r in range(rlwe.shape[0]):
            words = rlwe[r, 0].view(np.uint32)[(c - j) % N]
            out[r, :, :N] = np.where(j > c, np.uint32(0) - words, words).view(np.int32)
            out[r, :, N] = rlwe[r, 1, :width]
    return out.reshape(-1, N + 1)


def ring_selector_mask(mask_seed, N, rows):
    """The mask polynomials of selector rows: words 0 .. N-1 of stream (18, row) of the mask seed -> int32 [R][N]."""
    rows = np.asarray(rows, np.int64).ravel()
    return chacha20_words(mask_seed, DOMAIN_RING_SELECTOR_MASK, rows.astype(np.uint64), int(N)).reshape(len(rows), int(N)).view(np.int32)


def ring_selector_rows(bits, tlwe_key, mask_seed, noise_seed, basebit, l, stdev):
    """The bodies of the seeded RGSW samples of `bits` (0 / 1, one sample each) under the ring secret -> int32 [depth][2l][N]. Row
    k 2l + j: a = ring_selector_mask(mask_seed, N, row), e the N Gaussians of stream (19, row) of the private noise seed; the body is
    a*S + e - m h_j S for j < l and a*S + e + m h_j (coefficient 0) for row l + j, h_j = 2^(32-(j+1) basebit). The products by the
    binary S run here (_times_binary): there is no device generator. Equal seeds are refused."""
    _check_seeds(mask_seed, noise_seed)
    basebit, l = _check_cmux_digits(basebit, l)
    bits = np.asarray(bits, np.int64).ravel()
    assert bits.size >= 1 and ((bits == 0) | (bits == 1)).all(), "bits must be 0 / 1"
    S = np.asarray(tlwe_key).ravel()
    N, depth = S.size, bits.size
    rows = np.arange(depth * 2 * l)
    B = _times_binary(np.ascontiguousarray(ring_selector_mask(mask_seed, N, rows)).view(np.uint32), S)
    with np.errstate(over="ignore"):
        if stdev:
            B += noise32(chacha20_words(noise_seed, DOMAIN_RING_SELECTOR_NOISE, rows.astype(np.uint64), 4 * N), stdev).reshape(len(rows), N).view(np.uint32)
        B = B.reshape(depth, 2 * l, N)
        Su = (S.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
        for k in np.flatnonzero(bits):
            for j in range(l):
                h = np.uint32(1 << (32 - (j + 1) * basebit))
                B[k, j] -= h * Su
                B[k, l + j, 0] += h
    return B.view(np.int32)


def ring_selector_expand(mask_seed, body):
    """[depth][2l][2][N], what rs_ring_lookup_dev takes (rs_ring_cmux_dev: one sample of it), from the public mask seed and the
    bodies int32 [depth][2l][N]."""
    body = np.ascontiguousarray(body, np.int32)
    assert body.ndim == 3, "body must hold [depth][2l][N] words"
    depth, rows, N = body.shape
    mask = ring_selector_mask(mask_seed, N, np.arange(depth * rows)).reshape(depth, rows, N)
    return np.ascontiguousarray(np.stack([mask, body], axis=2))


def ring_cmux_sigma(N, basebit, l, sigma_row, depth=1, bit=1):
    """Deviation of the error of one coefficient after `depth` CMUXes (a lookup of that depth), as a real in [-1/2, 1/2): the noise
    of the 2l selector rows under the N signed digits of each (a uniform digit of -B/2 .. B/2 - 1 has mean square (B^2 + 2)/12),
    and the rounding of x to l basebit bits on its own coefficient and over the N / 2 set key bits. sigma_row is the deviation
    of one selector row's phase per coefficient.
      sigma^2 = depth (2 l N (B^2 + 2)/12 sigma_row^2  +  (1 + N/2) 2^(-2 l basebit)/12)
    The rounding reaches the phase multiplied by the selected bit: the formula is that of a selector of 1 (and of a lookup whose
    index has every bit set), the larger of the two. bit=0 leaves the second term out: the error under a selector of 0.
    The formula holds for both digit forms (ring_cmux_digits): the rows of a client's selector carry independent noise, so a digit
    enters by its mean square alone, and eps_k dig_j(eps_k x_k) has the mean square of dig_j; the rounding error of the alternating
    form is eps_k times that of the signed form at eps_k x_k, of the same size. Hence no digits= keyword here."""
    basebit, l = _check_cmux_digits(basebit, l)
    B = 2.0 ** basebit
    rounding = (1.0 + N / 2.0) * 2.0 ** (-2 * l * basebit) / 12.0 if bit else 0.0
    return float(np.sqrt(int(depth) * (2.0 * l * N * (B * B + 2.0) / 12.0 * float(sigma_row) ** 2 + rounding)))


def ring_selector_default_stdev(name):
    """The deviation of a selector row by default: the set's rlwe_default_stdev, or 2^-31 where that is refused."""
    try:
        return rlwe_default_stdev(name)
    except ValueError:
        return MIN_STDEV


def ring_cmux_default(name, depth=1):
    """(basebit, l) of a selector for a lookup of `depth` levels on set `name`: the cheapest shape, meaning the smallest l (the work
    is 2l rows) and for that l the basebit of the smallest ring_cmux_sigma, with l basebit <= 31, for which 8 ring_cmux_sigma stays
    inside the half step 1/8192 of the networks' 1/4096-scale values at rows of ring_selector_default_stdev(name). ValueError
    where no shape reaches it (INTEGRATION.md section 23 lists those)."""
    N, stdev = _shape(name)["N"], ring_selector_default_stdev(name)
    for l in range(1, RING_CMUX_MAX_BITS + 1):
        fits = [(ring_cmux_sigma(N, b, l, stdev, depth), b) for b in range(1, 9) if b * l <= RING_CMUX_MAX_BITS]
        fits = [f for f in fits if 8 * f[0] <= RING_CMUX_USE]
        if fits:
            return (min(fits)[1], l)
    raise ValueError("no (basebit, l) keeps 8 sigma inside 1/8192 on %s at depth %d" % (name, depth))


# ---- circuit bootstrapping (rs_ring_selector_dev restated) ----

SELECTOR_MAX_SRC = 65536
CIRCUIT_BOOTSTRAP_STEP = 1.0 / 16   # the payload step of the default shape: 8 sigma has to stay inside half of it


def _check_selector_digits(ks_basebit, ks_t):
    ks_basebit, ks_t = int(ks_basebit), int(ks_t)
    if not (1 <= ks_basebit <= 8 and ks_t >= 1 and ks_t * ks_basebit <= 32):
        raise ValueError("ks_basebit = %d, ks_t = %d: ks_basebit must lie in 1 .. 8, ks_t >= 1 and ks_t ks_basebit <= 32" % (ks_basebit, ks_t))
    return ks_basebit, ks_t


def selector_key_mask(mask_seed, N, rows):
    """The mask polynomials of selector-key rows: words 0 .. N-1 of stream (20, row) of the mask seed -> int32 [R][N]."""
    rows = np.asarray(rows, np.int64).ravel()
    return chacha20_words(mask_seed, DOMAIN_SELECTOR_KEY_MASK, rows.astype(np.uint64), int(N)).reshape(len(rows), int(N)).view(np.int32)


def selector_key(lwe_key, tlwe_key, mask_seed, noise_seed, ks_basebit, ks_t, stdev, chunk=512):
    """The bodies of the seeded selector key from the LWE secret lwe_key (any dimension n_src) to the ring secret tlwe_key -> int32
    [2][n_src+1][ks_t][N]. Row (f (n_src+1) + i) ks_t + q: a = selector_key_mask(mask_seed, N, row), e the N Gaussians of stream (21,
    row) of the private noise seed, sg = (s, -1), g_q = 2^(32-(q+1) ks_basebit); the body is a*S + e + sg_i g_q (coefficient 0) for
    family f = 1 and a*S + e - sg_i g_q S for family 0: a sample of zero with the message folded into the mask side, as selector
    rows are. The products by the binary S run here (_times_binary): there is no device generator. Equal seeds are refused."""
    _check_seeds(mask_seed, noise_seed)
    ks_basebit, ks_t = _check_selector_digits(ks_basebit, ks_t)
    s = np.asarray(lwe_key, np.int64).ravel()
    S = np.asarray(tlwe_key).ravel()
    n, N = s.size, S.size
    assert 1 <= n <= SELECTOR_MAX_SRC, "n_src must lie in 1 .. 65536"
    per = (n + 1) * ks_t
    body = np.empty((2 * per, N), np.uint32)
    for lo in range(0, 2 * per, chunk):
        rows = np.arange(lo, min(lo + chunk, 2 * per))
        B = _times_binary(np.ascontiguousarray(selector_key_mask(mask_seed, N, rows)).view(np.uint32), S)
        if stdev:
            with np.errstate(over="ignore"):
                B += noise32(chacha20_words(noise_seed, DOMAIN_SELECTOR_KEY_NOISE, rows.astype(np.uint64), 4 * N), stdev).reshape(len(rows), N).view(np.uint32)
        body[lo:lo + len(rows)] = B
    body = body.reshape(2, n + 1, ks_t, N)
    sg = np.concatenate([s, [-1]])
    Su = (S.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    with np.errstate(over="ignore"):
        for q in range(ks_t):
            m = ((sg << (32 - (q + 1) * ks_basebit)) & 0xFFFFFFFF).astype(np.uint32)      # sg_i g_q
            body[1, :, q, 0] += m
            body[0, :, q, :] -= m[:, None] * Su[None, :]
    return body.view(np.int32)


def selector_key_expand(mask_seed, body):
    """[2][n_src+1][ks_t][2][N], what rs_ring_selector_dev takes, from the public mask seed and the bodies int32 [2][n_src+1][ks_t][N]."""
    body = np.ascontiguousarray(body, np.int32)
    assert body.ndim == 4 and body.shape[0] == 2, "body must hold [2][n_src+1][ks_t][N] words"
    N = body.shape[3]
    mask = selector_key_mask(mask_seed, N, np.arange(body.size // N)).reshape(body.shape)
    return np.ascontiguousarray(np.stack([mask, body], axis=3))


def ring_selector_switch(ct, basebit, l, key, ks_basebit, ks_t):
    """rs_ring_selector_dev restated: ct int32 [depth l][n_src+1] (row k l + j the bootstrap of bit k at level j, phase +-h_j/2),
    key int32 [2][n_src+1][ks_t][2][N] -> int32 [depth][2l][2][N], sel[k][f l + j] = - sum_{i,q} d_iq K[f][i][q] over the unsigned
    rounding digits of x = (a, b + h_j/2). One uint64 matrix product of the digit matrix [rows][(n_src+1) ks_t] with each family's
    key [(n_src+1) ks_t][2 N], reduced mod 2^32: nothing like the device's tiled 32-bit multiply-adds."""
    basebit, l = _check_cmux_digits(basebit, l)
    ks_basebit, ks_t = _check_selector_digits(ks_basebit, ks_t)
    key = np.ascontiguousarray(key, np.int32)
    assert key.ndim == 5 and key.shape[0] == 2 and key.shape[2] == ks_t and key.shape[3] == 2, "key must hold [2][n_src+1][ks_t][2][N] words"
    n_src, N = key.shape[1] - 1, key.shape[4]
    x = np.ascontiguousarray(ct, np.int32).reshape(-1, n_src + 1).view(np.uint32).astype(np.int64)
    rows = x.shape[0]
    assert rows % l == 0, "ct must hold depth l rows"
    x[:, n_src] += np.array([1 << (31 - (j + 1) * basebit) for j in range(l)], np.int64)[np.arange(rows) % l]
    off = 0 if ks_t * ks_basebit >= 32 else 1 << (31 - ks_t * ks_basebit)
    xbar = (x + off) & 0xFFFFFFFF
    D = np.stack([(xbar >> (32 - (q + 1) * ks_basebit)) & ((1 << ks_basebit) - 1) for q in range(ks_t)], axis=-1)   # [rows][n_src+1][ks_t]
    D = D.reshape(rows, -1).astype(np.uint64)
    out = np.empty((rows // l, 2, l, 2 * N), np.uint32)
    for f in range(2):
        K = key[f].view(np.uint32).reshape(-1, 2 * N).astype(np.uint64)
        with np.errstate(over="ignore"):
            acc = (np.uint64(0) - D @ K) & np.uint64(0xFFFFFFFF)
        out[:, f] = acc.astype(np.uint32).reshape(rows // l, l, 2 * N)
    return out.reshape(rows // l, 2 * l, 2, N).view(np.int32)


def bootstrap_sigma(name, n=None):
    """Deviation sigma_u of the phase error of one bootstrapped sample of set `name` (blind rotation and LWE keyswitch), as a real:
      sigma_u^2 = n (2 l N (Bg^2 + 2)/12 sigma_bk^2 + (1/2)(1 + N/2) 2^(-2 l Bgbit)/12)  +  N t sigma_ks^2 + (N/2) 2^(-2 t basebit)/12
    n CMUXes under the signed gadget digits (the rounding reaches the phase where the key bit is set), then the keyswitch's N t
    table rows and the rounding of the N mask words over the N / 2 set ring-key bits."""
    s = _shape(name, n)
    Bg = 2.0 ** s["Bgbit"]
    rotate = s["n"] * (2.0 * s["l"] * s["N"] * (Bg * Bg + 2.0) / 12.0 * s["bk_stdev"] ** 2
                       + 0.5 * (1.0 + s["N"] / 2.0) * 2.0 ** (-2 * s["l"] * s["Bgbit"]) / 12.0)
    switch = s["N"] * s["t"] * s["ks_stdev"] ** 2 + s["N"] / 2.0 * 2.0 ** (-2 * s["t"] * s["basebit"]) / 12.0
    return float(np.sqrt(rotate + switch))


def selector_row_sigma(n_src, ks_basebit, ks_t, sigma_u, sigma_k):
    """(sigma_w, sigma_key) of one produced selector row, as reals. sigma_w is the deviation of the message-side error w = u -
    sum_i r_i sg_i: the bootstrap's sigma_u and the rounding of the n_src + 1 coordinates to ks_t ks_basebit bits (the b word and
    the n_src / 2 set key bits); family 1 carries it on coefficient 0, family 0 multiplied by -S(X), so on every coefficient where S
    has a bit. sigma_key is the key noise under the unsigned digits, on every coefficient of both families:
      sigma_w^2 = sigma_u^2 + (1 + n_src/2) 2^(-2 ks_t ks_basebit)/12,   sigma_key^2 = (n_src + 1) ks_t (Bk - 1)(2 Bk - 1)/6 sigma_k^2"""
    ks_basebit, ks_t = _check_selector_digits(ks_basebit, ks_t)
    Bk = 2.0 ** ks_basebit
    w = float(sigma_u) ** 2 + (1.0 + n_src / 2.0) * 2.0 ** (-2 * ks_t * ks_basebit) / 12.0
    key = (n_src + 1.0) * ks_t * (Bk - 1.0) * (2.0 * Bk - 1.0) / 6.0 * float(sigma_k) ** 2
    return float(np.sqrt(w)), float(np.sqrt(key))


def circuit_bootstrap_sigma(N, n_src, basebit, l, ks_basebit, ks_t, sigma_u, sigma_k, depth=1, bit=1, coefficient=None, digits="signed"):
    """Deviation of the error of coefficient c = `coefficient` after `depth` CMUXes under produced selectors (a lookup of that
    depth), as a real. Both families of a level come from the SAME bootstrapped sample, so its error w_j multiplies the digit
    polynomial Db_j(X) - Da_j(X) S(X), and it is the same w_j on every coefficient. The signed digits of rs_ring_cmux_dev have
    variance (B^2 - 1)/12 and MEAN -1/2; under independent row noise the mean only adds 1/4 to the mean square, but here the
    means of the N digits of Da_j add up along S: coefficient c collects -(1 - T_c)/2 of w_j, T_c = (bits of S at or below c) -
    (bits above c), of expectation t_c = c + 1 - N/2 and variance N/4. The term is largest at the two ends of the polynomial
    (c = 0, the default: the worst coefficient) and vanishes in the middle. The key noise enters as the row noise of
    ring_cmux_sigma, and the CMUX's own rounding is unchanged (bit=0 leaves it out):
      sigma^2 = depth (l sigma_w^2 ((1 + N/2)(B^2 - 1)/12 + ((1 - t_c)^2 + N/4)/4)  +  2 l N (B^2 + 2)/12 sigma_key^2  +  (1 + N/2) 2^(-2 l basebit)/12)
    with (sigma_w, sigma_key) = selector_row_sigma(n_src, ks_basebit, ks_t, sigma_u, sigma_k). `coefficient` may be an array. A
    trivial ciphertext (a = 0, a plaintext table row) has Da_j = 0, and the first term is then far smaller: an upper bound there.
    coefficient=None is the worst coefficient of the form: 0 here.
    digits="alternating" (rs_ring_cmux_alt_dev): the digit at position k has mean -eps_k / 2, eps_k = (-1)^k, so the mean of
    Db_j - Da_j S is -V(X)(1 - S(X))/2 with V = sum_k (-1)^k X^k. Coefficient c of V S mod X^N + 1 is (-1)^c (sum_{i <= c}
    (-1)^i S_i - sum_{i > c} (-1)^i S_i): N independent terms +-S_i of variance 1/4 each, N/4 in all at every c, and of expectation
    (-1)^c (e_c + e_c)/2 with e_c = sum_{i <= c} (-1)^i = [c even] (the alternating signs of the N positions cancel, so the sum above
    c is -e_c): 1 at even c, 0 at odd c. Coefficient c of V(1 - S) therefore has expectation (-1)^c - [c even] = -[c odd] and
    mean square N/4 + [c odd]. The ramp is gone and what is left of c is its parity, one part in N/4:
      sigma^2 = depth (l sigma_w^2 ((1 + N/2)(B^2 - 1)/12 + (N/4 + [c odd])/4)  +  the same key and rounding terms)
    coefficient=None is then any odd one."""
    basebit, l = _check_cmux_digits(basebit, l)
    sw, sk = selector_row_sigma(n_src, ks_basebit, ks_t, sigma_u, sigma_k)
    B = 2.0 ** basebit
    if _check_cmux_form(digits) == "alternating":
        mean_sq = N / 4.0 + (1.0 if coefficient is None else (np.asarray(coefficient, np.int64) & 1).astype(np.float64))
    else:
        t = np.asarray(0 if coefficient is None else coefficient, np.float64) + 1.0 - N / 2.0
        mean_sq = (1.0 - t) ** 2 + N / 4.0
    sample = l * sw * sw * ((1.0 + N / 2.0) * (B * B - 1.0) / 12.0 + mean_sq / 4.0)
    rounding = (1.0 + N / 2.0) * 2.0 ** (-2 * l * basebit) / 12.0 if bit else 0.0
    out = np.sqrt(int(depth) * (sample + 2.0 * l * N * (B * B + 2.0) / 12.0 * sk * sk + rounding))
    return float(out) if out.ndim == 0 else out


def circuit_bootstrap_default(name, depth=1, step=CIRCUIT_BOOTSTRAP_STEP, digits="signed"):
    """(basebit, l, ks_basebit, ks_t) of circuit bootstrapping for a lookup of `depth` levels on set `name`: the cheapest shape for
    which 8 circuit_bootstrap_sigma of the worst coefficient stays inside step / 2, the half step of payloads that are multiples of
    `step`, at sigma_u =
    bootstrap_sigma(name) and key rows of ring_selector_default_stdev(name). Cheapest: the smallest l (l bootstraps a bit), for that
    l the smallest ks_t (the key is 2 (n + 1) ks_t ring samples), and for that pair the (basebit, ks_basebit) of the smallest
    sigma. ValueError where no shape reaches it: default-128, whose bootstrap output noise alone is too large for every shape.
    digits: the digit form of the CMUX the selectors will drive ("signed": rs_ring_cmux_dev; "alternating": rs_ring_cmux_alt_dev,
    whose sigma has no ramp); the selectors themselves are the same."""
    _check_cmux_form(digits)
    sh = _shape(name)
    N, n, su, sk = sh["N"], sh["n"], bootstrap_sigma(name), ring_selector_default_stdev(name)
    for l in range(1, RING_CMUX_MAX_BITS + 1):
        for ks_t in range(1, 33):
            fits = [(circuit_bootstrap_sigma(N, n, b, l, kb, ks_t, su, sk, depth, digits=digits), b, kb)
                    for b in range(1, 9) if b * l <= RING_CMUX_MAX_BITS for kb in range(1, 9) if kb * ks_t <= 32]
            fits = [f for f in fits if 8 * f[0] <= step / 2.0]
            if fits:
                _, b, kb = min(fits)
                return (b, l, kb, ks_t)
    raise ValueError("no shape keeps 8 sigma inside half of %g on %s at depth %d with %s digits" % (step, name, depth, digits))


# ---- noise audit (rs_audit_keys_dev / rs_audit_compressed_keys_dev restated) ----

GAUSS_BOUND = 8.58   # Box-Muller with u1 >= 2^-53: |z| <= sqrt(2 * 53 * ln 2) = 8.572


def noise_limits(name):
    """Default (bk_limit, ksk_limit) of the audit = floor(8.58 sigma 2^32) + 1 for the set's deviations. A bound, not a statistic:
    u1 >= 2^-53 gives |z| <= 8.572, so no noise word of an honestly generated key exceeds it."""
    s = _shape(name)
    return tuple(int(np.floor(GAUSS_BOUND * sigma * 2.0 ** 32)) + 1 for sigma in (s["bk_stdev"], s["ks_stdev"]))


def bk_noise(name, lwe_key, tlwe_key, stored, rows=None, mask_seed=None, chunk=256):
    """Noise words of bk rows i 2l + p (all n 2l rows if rows is None) -> int32 [R][N]. Full key (mask_seed None): stored holds the
    rows [R][2][N]; compressed: stored holds the body rows [R][N] and the masks are the domain-3 streams of mask_seed. The LWE
    dimension is len(lwe_key)."""
    s = _shape(name, len(lwe_key))
    l, Bgbit, N = s["l"], s["Bgbit"], s["N"]
    rows = np.arange(s["n"] * 2 * l) if rows is None else np.asarray(rows, np.int64).ravel()
    stored = np.asarray(stored, np.int32).reshape(len(rows), -1, N)
    assert stored.shape[1] == (2 if mask_seed is None else 1), "stored rows have the wrong shape"
    lwe = np.asarray(lwe_key).astype(np.uint32)
    tlwe = np.asarray(tlwe_key).astype(np.uint32)
    out = np.empty((len(rows), N), np.int32)
    with np.errstate(over="ignore"):
        for lo in range(0, len(rows), chunk):
            r = rows[lo:lo + chunk]
            if mask_seed is None:
                A = np.ascontiguousarray(stored[lo:lo + chunk, 0]).view(np.uint32)
            else:
                A = chacha20_words(mask_seed, DOMAIN_BK_MASK, r, N)
            E = np.ascontiguousarray(stored[lo:lo + chunk, -1]).view(np.uint32) - _times_binary(A, tlwe_key)
            p = r % (2 * l)
            c, j = p // l, p % l
            gadget = lwe[r // (2 * l)] * (np.uint32(1) << (32 - (j + 1) * Bgbit).astype(np.uint32))
            E[c == 1, 0] -= gadget[c == 1]
            E[c == 0] += gadget[c == 0, None] * tlwe[None, :]
            out[lo:lo + chunk] = E.view(np.int32)
    return out


def ksk_noise(name, lwe_key, tlwe_key, stored, rows=None, mask_seed=None, chunk=4096):
    """Noise words of ksk samples s = (i t + j) 2^basebit + v (all of them if rows is None) -> int32 [R]; 0 for v = 0. Full key
    (mask_seed None): stored holds the samples [R][n+1]; compressed: stored holds the body words [R] (those of v = 0 are ignored)
    and the masks are the domain-5 streams of mask_seed."""
    s = _shape(name, len(lwe_key))
    n, N, t, basebit = s["n"], s["N"], s["t"], s["basebit"]
    base = 1 << basebit
    rows = np.arange(N * t * base) if rows is None else np.asarray(rows, np.int64).ravel()
    stored = np.asarray(stored, np.int32).reshape(len(rows), -1)
    assert stored.shape[1] == (n + 1 if mask_seed is None else 1), "stored samples have the wrong shape"
    lwe = np.asarray(lwe_key).astype(np.uint64)
    tlwe = np.asarray(tlwe_key).astype(np.uint64)
    out = np.zeros(len(rows), np.int32)
    for lo in range(0, len(rows), chunk):
        r = rows[lo:lo + chunk]
        live = np.flatnonzero(r % base != 0)
        if len(live) == 0:
            continue
        rl = r[live]
        A = stored[lo + live, :n].view(np.uint32) if mask_seed is None else chacha20_words(mask_seed, DOMAIN_KS_MASK, rl, n)
        dot = (A.astype(np.uint64) * lwe).sum(axis=-1)
        ij = rl >> basebit
        i, j = ij // t, ij % t
        mess = (tlwe[i] * (rl % base).astype(np.uint64)) << (32 - (j + 1) * basebit).astype(np.uint64)
        b = stored[lo + live, -1].view(np.uint32).astype(np.uint64)
        out[lo + live] = ((b - dot - mess) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return out


def audit(name, lwe_key, tlwe_key, bk=None, ksk=None, mask_seed=None, limits=None, bk_rows=None, ksk_rows=None):
    """The report of rs_audit_keys_dev (mask_seed None; bk [R][2][N], ksk [R'][n+1]) or rs_audit_compressed_keys_dev (bk, ksk the
    bodies) for the given rows (None: the whole half; a half that is None is skipped) -> a dict of the rs_key_audit fields plus
    bk_noise int32 [R][N] and ksk_noise int32 [R'] (None for a skipped half). limits defaults to noise_limits(name)."""
    bk_limit, ksk_limit = noise_limits(name) if limits is None else limits
    s = _shape(name, len(lwe_key))
    base = 1 << s["basebit"]
    rep = dict(bk_max_abs=0, ksk_max_abs=0, bk_over=0, ksk_over=0, ksk_zero_bad=0, bk_words=0, ksk_words=0, bk_noise=None, ksk_noise=None)
    mag = lambda e: np.abs(e.astype(np.int64))
    if bk is not None:
        e = bk_noise(name, lwe_key, tlwe_key, bk, bk_rows, mask_seed)
        rep.update(bk_noise=e, bk_words=int(e.size), bk_max_abs=int(mag(e).max(initial=0)), bk_over=int((mag(e) > bk_limit).sum()))
    if ksk is not None:
        rows = np.arange(s["N"] * s["t"] * base) if ksk_rows is None else np.asarray(ksk_rows, np.int64).ravel()
        e = ksk_noise(name, lwe_key, tlwe_key, ksk, rows, mask_seed)
        live = rows % base != 0
        rep.update(ksk_noise=e, ksk_words=int(live.sum()), ksk_max_abs=int(mag(e).max(initial=0)), ksk_over=int((mag(e) > ksk_limit).sum()))
        if mask_seed is None:
            rep["ksk_zero_bad"] = int(np.asarray(ksk, np.int32).reshape(len(rows), -1)[~live].any(axis=-1).sum())
    return rep
