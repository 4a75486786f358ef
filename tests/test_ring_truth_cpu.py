"""tests/ring_truth.py pinned on the CPU: against a schoolbook product in Python integers at N = 64, and against the client's own
host decryption at N = 1024 and N = 4096 on a seeded ciphertext of a known message. ring_truth imports nothing from the product;
this file does, to show that the two agree where both are right."""
import ast
import os

import numpy as np
import pytest

import ring_truth
from redsec_amd import client, keygen

KEY_SEED = bytes(range(23, 55))
MASK_SEED = bytes(range(140, 172))
NOISE_SEED = bytes(range(71, 103))
RAND_SEED = bytes(range(200, 232))


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _schoolbook(a, s):
    """the N^2 products in Python integers, X^N = -1, reduced mod 2^32 at the end"""
    N = len(a)
    out = [0] * N
    for i in range(N):
        for j in range(N):
            k, sign = (i + j, 1) if i + j < N else (i + j - N, -1)
            out[k] += sign * (int(a[i]) & 0xFFFFFFFF) * int(s[j])
    return np.array([v % (1 << 32) for v in out], np.uint64).astype(np.uint32).view(np.int32)


def test_ring_truth_imports_nothing_from_the_product():
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ring_truth.py")).read())
    names = [a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names]
    names += [node.module for node in ast.walk(tree) if isinstance(node, ast.ImportFrom)]
    assert names == ["numpy"]


@pytest.mark.parametrize("kind", ["binary", "signed digits", "extreme words"])
def test_negacyclic_equals_a_schoolbook_in_python_integers(kind):
    N = 64
    rng = np.random.default_rng(len(kind))
    a = _words(rng, N)
    s = rng.integers(0, 2, N) if kind == "binary" else rng.integers(-128, 128, N)
    if kind == "extreme words":                                  # the largest words against the largest digits: where a sum would wrap
        a[:] = np.array([-1, -(1 << 31), (1 << 31) - 1, 0], np.int64).astype(np.int32)[rng.integers(0, 4, N)]
        s = np.where(rng.integers(0, 2, N) == 1, 127, -128)
    want = _schoolbook(a, s)
    assert np.array_equal(ring_truth.negacyclic(a, s), want)
    assert np.array_equal(ring_truth.negacyclic(a.view(np.uint32), s), want)
    # X^k a(X): a rotation with the wrapped part negated
    for k in (0, 1, N - 1):
        mono = np.zeros(N, np.int64)
        mono[k] = 1
        rot = np.concatenate([(np.uint32(0) - a.view(np.uint32)[N - k:]), a.view(np.uint32)[:N - k]]).view(np.int32)
        assert np.array_equal(ring_truth.negacyclic(a, mono), rot)


def test_negacyclic_refuses_coefficients_whose_sums_would_not_fit():
    a = np.zeros(8192, np.int32)
    ring_truth.negacyclic(a, np.full(8192, (1 << 18) - 1))              # 2^13 2^32 (2^18 - 1) < 2^63
    with pytest.raises(AssertionError, match="does not fit"):
        ring_truth.negacyclic(a, np.full(8192, 1 << 18))
    with pytest.raises(AssertionError):
        ring_truth.negacyclic(a.astype(np.int64), np.ones(8192))        # words must be 32-bit


def test_phases_and_extraction_agree_with_a_schoolbook():
    N = 64
    rng = np.random.default_rng(9)
    S = rng.integers(0, 2, N)
    ct = _words(rng, 2, N)
    want = (ct[1].view(np.uint32) - _schoolbook(ct[0], S).view(np.uint32)).view(np.int32)
    phase = ring_truth.rlwe_phase(ct, S)
    assert phase.dtype == np.int32 and np.array_equal(phase, want)
    for k in range(N):
        sample = ring_truth.extract(ct, k)
        assert sample.shape == (N + 1,) and sample[N] == ct[1, k]
        assert ring_truth.lwe_phase(sample, S) == want[k]
    lwe = _words(rng, 5, 17)
    s = rng.integers(0, 2, 16)
    brute = [(int(r[16]) - sum(int(r[i]) * int(s[i]) for i in range(16))) % (1 << 32) for r in lwe]
    assert np.array_equal(ring_truth.lwe_phase(lwe, s).view(np.uint32), np.array(brute, np.uint64).astype(np.uint32))
    assert ring_truth.error(np.int32([5, -3]), np.int32([2, 1])).tolist() == [3 / 2.0 ** 32, -4 / 2.0 ** 32]
    assert ring_truth.centred(np.uint32([1 << 31])).tolist() == [-0.5]


@pytest.mark.parametrize("name,N", [("redsec_small_v2", 1024), ("redsec_medium", 4096)])
def test_rlwe_phase_equals_the_clients_host_decryption_of_a_known_message(name, N):
    """One ciphertext of N multiples of 1/16 under the set's ring secret, made by the product's own public-key encryption on the host
    from fixed seeds: ring_truth and client.SecretKeySet.packed_phase give the same words, both round to the message, and extraction
    gives the product's LWE samples."""
    sk = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, KEY_SEED, n=16))
    assert sk.N == N
    pk = sk.rlwe_public_key(MASK_SEED, NOISE_SEED, stdev=2.0 ** -30)
    values = np.random.default_rng(N).integers(0, 16, N)
    mu = (values << 28).astype(np.uint32).view(np.int32)
    ct = keygen.rlwe_pk_encrypt(pk.expand(), mu, RAND_SEED, 0, stdev=2.0 ** -30)
    assert ct.shape == (1, 2, N)
    phase = ring_truth.rlwe_phase(ct[0], sk.tlwe_key)
    assert np.array_equal(phase, sk.packed_phase(ct, N))
    err = ring_truth.error(phase, mu)
    assert np.abs(err).max() < 2.0 ** -12                           # sqrt(N) 2^-30 is 2^-24 on the large ring
    assert np.array_equal(((phase.view(np.uint32).astype(np.int64) + (1 << 27)) >> 28) & 15, values)
    rows = keygen.rlwe_extract(ct, N)
    for k in (0, 1, N // 2, N - 1):
        assert np.array_equal(ring_truth.extract(ct[0], k), rows[k])
        assert ring_truth.lwe_phase(rows[k], sk.tlwe_key) == phase[k]


def test_lwe_phase_equals_the_clients_host_decryption_of_known_bits():
    sk = client.SecretKeySet.from_secret("redsec_medium", *keygen.secret_keys("redsec_medium", KEY_SEED, n=16))
    bits = np.random.default_rng(3).integers(0, 2, 40)
    ct = sk.encrypt_bits(bits, seed=11)
    phase = ring_truth.lwe_phase(ct, sk.lwe_key)
    assert np.array_equal(phase, sk.phase(ct))
    assert np.array_equal((phase > 0).astype(np.int64), bits)
    assert np.abs(ring_truth.error(phase, np.where(bits == 1, 1 << 29, -(1 << 29)).astype(np.int32))).max() < 2.0 ** -10
