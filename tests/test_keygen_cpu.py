"""Key generation streams and key contents without a GPU: the numpy restatement (redsec_amd/keygen.py) against RFC 8439, against the
device code's own RS_HD functions (compiled into the lane emulator), and a restated key against the CPU oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib
from redsec_amd import client, keygen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chacha20_words_reproduce_rfc8439_block_function_vector():
    """RFC 8439 section 2.3.2: key 00 01 .. 1f, nonce 00000009 0000004a 00000000 (bytes), block counter 1."""
    seed = bytes(range(32))
    nonce = np.frombuffer(bytes.fromhex("000000090000004a00000000"), "<u4")
    domain, row = int(nonce[0]), int(nonce[1]) | (int(nonce[2]) << 32)
    want = [int(x, 16) for x in ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 466482d2 09aa9f07 05d7c214 "
                                 "a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()]
    got = keygen.chacha20_words(seed, domain, row, 32)
    assert [int(x) for x in got[16:]] == want
    # the same words for an array of rows
    assert np.array_equal(keygen.chacha20_words(seed, domain, [row, row + 1], 32)[0], got)


def _emu():
    L = emu_lib.lib()
    u32p = C.POINTER(C.c_uint32)
    L.rs_emu_chacha_block.argtypes = [u32p, C.c_uint32, C.c_uint64, C.c_uint32, u32p]
    L.rs_emu_keygen_uniforms.argtypes = [u32p, C.POINTER(C.c_double)]
    L.rs_emu_keygen_noise.argtypes = [u32p, C.c_double]
    L.rs_emu_keygen_noise.restype = C.c_int32
    return L, u32p


def test_device_stream_functions_equal_numpy_bit_for_bit():
    """csrc/rs_keygen.h's ChaCha block and u1 / u2 (the functions the kernels run) against the numpy restatement, over a sweep of
    (domain, row, block) with rows past 2^32 and block counters past 2^16."""
    L, u32p = _emu()
    rng = np.random.default_rng(11)
    seed = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    key = np.frombuffer(seed, "<u4").astype(np.uint32).copy()
    cases = [(d, r, b) for d in (1, 2, 3, 4, 5, 6, 0xFFFFFFFF) for r in (0, 1, 12345, (1 << 32) - 1, 1 << 32, (7 << 32) + 3, (1 << 64) - 1)
             for b in (0, 1, 15, 1 << 16, (1 << 16) + 5, (1 << 32) - 1)]
    for d, r, b in cases:
        out = np.zeros(16, np.uint32)
        L.rs_emu_chacha_block(key.ctypes.data_as(u32p), d, r, b, out.ctypes.data_as(u32p))
        want = keygen._chacha_blocks(keygen._seed_words(seed), d, np.array([r], np.uint64), np.array([b], np.uint32))[0]
        assert np.array_equal(out, want), (d, r, b)
        if b < (1 << 20):   # through the word interface as well
            assert np.array_equal(out, keygen.chacha20_words(seed, d, r, 16 * (b + 1))[16 * b:]), (d, r, b)
    words = rng.integers(0, 1 << 32, (4000, 4), dtype=np.uint64).astype(np.uint32)
    words[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0xFFFFFFFF, 0, 0]]
    u1, u2 = keygen.uniforms(words.reshape(-1, 4))
    u1, u2 = u1[:, 0], u2[:, 0]
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert u1[0] == 2.0 ** -53 and u1[1] == 1.0 and u2[0] == 0.0
    got = np.zeros(2)
    for k in range(len(words)):
        w = np.ascontiguousarray(words[k])
        L.rs_emu_keygen_uniforms(w.ctypes.data_as(u32p), got.ctypes.data_as(C.POINTER(C.c_double)))
        assert got[0] == u1[k] and got[1] == u2[k], k
    # the noise words through the host's libm: equal but for values within a last-bit change of an integer
    sig = 2.0 ** -25
    mine = keygen.noise32(words.reshape(-1), sig)
    emu = np.array([L.rs_emu_keygen_noise(np.ascontiguousarray(words[k]).ctypes.data_as(u32p), sig) for k in range(len(words))], np.int32)
    assert np.mean(mine == emu) >= 0.999 and np.abs(mine.astype(np.int64) - emu).max() <= 1
    assert L.rs_emu_keygen_noise(np.ascontiguousarray(words[5]).ctypes.data_as(u32p), 0.0) == 0


def test_secret_keys_are_deterministic_binary_and_independent():
    a = keygen.secret_keys("default128", b"\x01" * 32)
    b = keygen.secret_keys("default128", b"\x01" * 32)
    c = keygen.secret_keys("default128", b"\x02" + b"\x01" * 31)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    lwe, tlwe = a
    assert lwe.shape == (630,) and tlwe.shape == (1024,) and lwe.dtype == np.int32
    assert set(np.unique(lwe)) <= {0, 1} and set(np.unique(tlwe)) <= {0, 1}
    assert 0.4 < lwe.mean() < 0.6 and 0.4 < tlwe.mean() < 0.6
    assert not np.array_equal(lwe, c[0]) and not np.array_equal(tlwe, c[1])
    # the LWE and TRLWE keys come from different streams (domain 1, domain 2): not a prefix of each other
    assert np.mean(lwe == tlwe[:630]) < 0.6
    L, N = keygen.secret_keys("redsec_large", b"\x01" * 32)
    assert L.shape == (6144,) and N.shape == (8192,)


def test_negacyclic_product_over_the_support_equals_the_matrix_product():
    rng = np.random.default_rng(3)
    A = rng.integers(0, 1 << 32, (3, 1024), dtype=np.uint64).astype(np.uint32)
    S = rng.integers(0, 2, 1024).astype(np.int32)
    want = keygen._times_binary(A, S)
    big = np.zeros((3, 2048), np.uint32)          # N = 2048 takes the support loop; with S in the low half the
    big[:, :1024] = A                             # product's low half is not a wrap-around of the N = 1024 one, so
    S2 = np.zeros(2048, np.int32); S2[:1024] = S  # check it against a direct schoolbook sum instead
    got = keygen._times_binary(big, S2)
    ref = np.zeros((3, 2048), np.int64)
    for m in np.flatnonzero(S2):
        sh = np.roll(big.astype(np.int64), m, axis=1)
        sh[:, :m] *= -1
        ref += sh
    assert np.array_equal(got, (ref % (1 << 32)).astype(np.uint32))
    assert want.shape == (3, 1024)


@pytest.mark.parametrize("name,toy", [("default128", "toy"), ("redsec_small_v2", "toy_redsec")])
def test_restated_toy_key_runs_the_cpu_oracle_gates(name, toy):
    """A key restated with its set's noise at a toy LWE dimension, fed to the CPU oracle: NAND / AND / MUX decrypt correctly. Pins
    the key CONTENTS (gadget placement, component order, keyswitch messages) independently of the GPU."""
    import oracle_lib as ol
    p = ol.params(toy)
    seed = bytes(range(100, 132))
    lwe, tlwe = keygen.secret_keys(name, seed, n=p.n)
    (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    bk, ksk = keygen.restate(name, seed, lwe, tlwe, bk_stdev, ks_stdev)

    class K:
        pass
    ks = K()
    ks.p, ks.bk, ks.ksk = p, np.ascontiguousarray(bk).ravel(), np.ascontiguousarray(ksk).ravel()
    ctx = ol.Ctx(ks)
    sk = client.SecretKeySet.from_secret(name, lwe, tlwe)
    assert sk.n == p.n and sk.bk is None
    rng = np.random.default_rng(5)
    a, b, c = (rng.integers(0, 2, 24) for _ in range(3))
    ca, cb, cc = sk.encrypt_bits(a, seed=1), sk.encrypt_bits(b, seed=2), sk.encrypt_bits(c, seed=3)
    assert np.array_equal(sk.decrypt_bits(ctx.gate_batch("NAND", ca, cb)), 1 - (a & b))
    assert np.array_equal(sk.decrypt_bits(ctx.gate_batch("AND", ca, cb)), a & b)
    assert np.array_equal(sk.decrypt_bits(ctx.mux_batch(ca, cb, cc)), np.where(a == 1, b, c))
    ctx.close()


def test_keygen_kernels_are_built_within_their_scratch_budget():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    hits = {n: k for n, k in ks.items() if re.search(r"20gen_keygen_bk_kernelILi1[0-3]E|17keygen_ksk_kernel", n)}
    assert len(hits) == 5, sorted(hits)
    for n, k in hits.items():
        assert k["scratch"] <= 96 and k["lds"] <= 163840, (n, k)


def test_generate_and_backend_bindings_exist():
    import redsec_amd
    assert "rs_keygen_dev" in redsec_amd.ABI_SYMBOLS and "rs_load_keys_dev" in redsec_amd.ABI_SYMBOLS
    assert callable(redsec_amd.Backend.keygen) and callable(redsec_amd.Backend.load_keys_dev)
    p = redsec_amd.params("redsec_medium", n=16)
    assert keygen.set_name(p) == "redsec_medium"
    assert keygen.set_name(redsec_amd.params("default128")) == "default128"
