"""Ground truth for ring ciphertexts, written from the definitions and from nothing else: plain numpy, no import of redsec_amd.

A ring ciphertext is int32 [2][N] = (a, b) over Z[X]/(X^N + 1) with words mod 2^32; under the binary ring secret S its phase is
b - a*S. An LWE sample is int32 [n+1] = (a_0 .. a_{n-1}, b) with phase b - sum_i a_i s_i. Sample extraction reads coefficient k of a
ring ciphertext as an LWE sample of dimension N under the coefficients of S. The tests decrypt what the device computed with these
functions and the host's copy of the secrets, so that a convention shared by a kernel and the product's own numpy restatement of it
(a sign, the order of two key families, a gadget level) cannot hide: a ciphertext that follows a wrong convention does not decrypt.
"""
import numpy as np


def _u(words):
    """32-bit words (int32 or uint32, any shape) as int64 in 0 .. 2^32 - 1"""
    w = np.asarray(words)
    assert w.dtype in (np.int32, np.uint32), "words must be 32-bit"
    return w.astype(np.int64) & 0xFFFFFFFF


def _i32(values):
    """int64 values reduced mod 2^32 -> int32 words"""
    return (np.asarray(values, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def negacyclic(a, s):
    """a(X) s(X) mod (X^N + 1, 2^32) for a 32-bit polynomial a [N] and a small-coefficient polynomial s [N] -> int32 [N].
    Coefficient k is sum_{i+j=k} a_i s_j - sum_{i+j=k+N} a_i s_j. The linear convolution runs in int64 over the words read as
    0 .. 2^32 - 1: every partial sum stays below N 2^32 max|s|, which has to fit 63 bits."""
    a, s = _u(a).ravel(), np.asarray(s, np.int64).ravel()
    N = a.size
    assert s.size == N, "both polynomials must have N coefficients"
    bound = int(np.abs(s).max()) if N else 0
    assert N * (1 << 32) * bound < (1 << 63), "N 2^32 max|s| does not fit int64"
    full = np.convolve(a, s)                     # 2N - 1 coefficients of the product over Z
    low = full[:N].copy()
    low[:N - 1] -= full[N:]                      # X^N = -1
    return _i32(low)


def rlwe_phase(ct, S):
    """b - a*S of one ring ciphertext int32 [2][N] under the ring secret S [N] -> int32 [N]"""
    ct = np.asarray(ct)
    assert ct.ndim == 2 and ct.shape[0] == 2, "a ring ciphertext is [2][N]"
    return _i32(_u(ct[1]) - _u(negacyclic(ct[0], S)))


def lwe_phase(ct, s):
    """b - sum_i a_i s_i of LWE samples int32 [B][n+1] (or one, [n+1]) under the secret s [n] -> int32 [B] (or a scalar)"""
    ct, s = np.asarray(ct), np.asarray(s, np.int64).ravel()
    assert ct.shape[-1] == s.size + 1, "samples must hold n + 1 words"
    assert s.size * (1 << 32) * max(1, int(np.abs(s).max())) < (1 << 63), "n 2^32 max|s| does not fit int64"
    u = _u(ct)
    return _i32(u[..., -1] - (u[..., :-1] * s).sum(axis=-1))


def extract(ct, k):
    """Coefficient k of the ring ciphertext int32 [2][N] as an LWE sample of dimension N -> int32 [N+1]: (a', b_k) with
    a'_i = a_{k-i} for i <= k and -a_{N+k-i} for i > k, so that lwe_phase(extract(ct, k), S) is coefficient k of rlwe_phase(ct, S):
    (a*S)_k = sum_{i<=k} a_{k-i} S_i - sum_{i>k} a_{N+k-i} S_i."""
    ct = np.asarray(ct)
    assert ct.ndim == 2 and ct.shape[0] == 2, "a ring ciphertext is [2][N]"
    N = ct.shape[1]
    assert 0 <= k < N
    a = _u(ct[0])
    i = np.arange(N)
    mask = np.where(i <= k, a[(k - i) % N], -a[(N + k - i) % N])
    return _i32(np.concatenate([mask, _u(ct[1])[k:k + 1]]))


def centred(words):
    """32-bit words as reals in [-1/2, 1/2): the torus"""
    return _i32(_u(words)).astype(np.float64) / 2.0 ** 32


def error(phase, want):
    """phase - want mod 2^32 as reals in [-1/2, 1/2)"""
    return centred(_i32(_u(phase) - _u(want)))
