"""Public-key encryption without a GPU (include/redsec_hip.h rs_pk_encrypt_dev): the kernel's own selection
function (compiled into the lane emulator) against the numpy restatement, the exact phase identity of the restatement, 70 bits under a
default-128 public key of the default size, the symbol in the header, the library and the binding, the failure without a context, and
the scratch budget of the new kernel."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import emu_lib
import redsec_amd
from redsec_amd import client, keygen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAND_SEED = bytes(range(40, 72))
MASK_SEED = bytes(range(120, 152))
NOISE_SEED = bytes(range(5, 37))
ROWS = (0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1)
E8 = 1 << 29


def _emu():
    L = emu_lib.lib()
    L.rs_emu_pk_select.argtypes = [C.c_char_p, C.c_uint64, C.c_long, C.POINTER(C.c_uint32)]
    L.rs_emu_pk_select.restype = None
    L.rs_emu_pk_tile.argtypes = []
    return L


@pytest.mark.parametrize("m", [1, 31, 32, 33, 512, 513, 1100])
def test_emulated_selection_equals_numpy(m):
    """kg_pk_select_block, chunk by chunk as the kernel walks it, gives the bits of keygen.pk_selection at every row of ROWS."""
    L = _emu()
    for row in ROWS:
        words = np.full((m + 31) // 32, 0xDEADBEEF, np.uint32)
        L.rs_emu_pk_select(RAND_SEED, row, m, words.ctypes.data_as(C.POINTER(C.c_uint32)))
        got = ((words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).ravel()[:m].astype(np.uint8)
        want = keygen.pk_selection(RAND_SEED, m, row, 1)
        assert want.shape == (1, m) and want.dtype == np.uint8
        assert np.array_equal(got, want[0]), (m, row)
    assert 1 <= L.rs_emu_pk_tile() <= 64


def test_selection_is_the_domain_9_stream_and_is_disjoint_from_the_other_domains():
    assert keygen.DOMAIN_PK_SELECT == 9
    sel = keygen.pk_selection(RAND_SEED, 1100, (1 << 32) - 2, 4)
    for i in range(4):
        words = keygen.chacha20_words(RAND_SEED, 9, (1 << 32) - 2 + i, 35)
        for j in (0, 1, 31, 32, 511, 512, 1099):
            assert sel[i, j] == (int(words[j >> 5]) >> (j & 31)) & 1
    assert 0.4 < sel.mean() < 0.6
    for domain in range(1, 9):
        other = keygen.chacha20_words(RAND_SEED, domain, 0, 35)
        assert np.mean(other == keygen.chacha20_words(RAND_SEED, 9, 0, 35)) < 0.1
    with pytest.raises(ValueError):
        keygen.pk_selection(RAND_SEED, 8, (1 << 64) - 1, 2)
    for bad_m in (0, 1 << 31):
        with pytest.raises(ValueError):
            keygen.pk_selection(RAND_SEED, bad_m, 0, 1)
    assert keygen.pk_selection(RAND_SEED, 8, (1 << 64) - 1, 1).shape == (1, 8)
    assert keygen.pk_rows(630) == 32 * 631 + 256 == 20448 and keygen.pk_rows(350) == 11488


def test_restated_phase_identity_is_exact():
    """phase(ct_i) = mu_i + phase(base_i) + the sum of the phases of the selected rows (mod 2^32), for every combination of mu and
    base, across 2^32 in `first`; B = 0 gives an empty batch."""
    sk = client.SecretKeySet.from_secret("redsec_small_v2", *keygen.secret_keys("redsec_small_v2", NOISE_SEED, 64))
    m, B = 300, 37
    pk_s = sk.public_key(m, mask_seed=MASK_SEED, noise_seed=NOISE_SEED, first=11)
    assert isinstance(pk_s, client.SeededCiphertexts) and len(pk_s) == m and pk_s.first == 11
    pk = pk_s.expand()
    ph_pk = sk.phase(pk).astype(np.int64)
    assert 0 < np.abs(ph_pk).max() < 8 * client.SECALPHA * 2 ** 32          # encryptions of zero: the phase is the noise alone
    rng = np.random.default_rng(2)
    mu = rng.integers(-(1 << 31), 1 << 31, B, dtype=np.int64)
    base = sk.encrypt_torus(rng.integers(-(1 << 31), 1 << 31, B, dtype=np.int64), seed=3)
    for first in (0, (1 << 32) - 20):
        sel = keygen.pk_selection(RAND_SEED, m, first, B).astype(np.int64)
        for use_mu, use_base in ((1, 0), (0, 1), (1, 1), (0, 0)):
            ct = keygen.pk_encrypt(pk, mu if use_mu else None, RAND_SEED, first, base if use_base else None, B=B)
            assert ct.shape == (B, 65) and ct.dtype == np.int32
            want = sel @ ph_pk + (mu if use_mu else 0) + (sk.phase(base).astype(np.int64) if use_base else 0)
            assert np.array_equal(sk.phase(ct), (want & 0xFFFFFFFF).astype(np.uint32).view(np.int32)), (first, use_mu, use_base)
            # and word for word: the plain integer subset sums
            words = sel.astype(np.uint64) @ pk.view(np.uint32).astype(np.uint64)
            if use_base:
                words += base.view(np.uint32)
            if use_mu:
                words[:, 64] += (mu & 0xFFFFFFFF).astype(np.uint64)
            assert np.array_equal(ct.view(np.uint32), (words & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert keygen.pk_encrypt(pk, np.zeros(0, np.int64), RAND_SEED).shape == (0, 65)
    with pytest.raises(ValueError):
        keygen.pk_encrypt(pk, mu, RAND_SEED, first=(1 << 64) - B + 1)


def test_seventy_bits_under_a_default128_public_key_decrypt():
    """m = pk_rows(630) = 20,448 rows of alpha = 2^-15: all 70 bits decrypt and every error stays inside the margin of 1/8 (largest
    seen here: 4.7e-3). With e_j the noise of row j, the error of an output is sum_j b_j e_j over fair bits b_j: for ONE key its mean is
    the fixed offset sum_j e_j / 2 and its spread sqrt(sum_j e_j^2) / 2 = alpha sqrt(m / 4) = 2.2e-3; over keys the offset has that same
    deviation, which makes the root mean square alpha sqrt(m / 2) = 3.1e-3. The test holds the 70 errors to the offset and the spread
    of its own key (known exactly from the secret): the mean of 70 samples within 4 deviations of a mean (4 / sqrt(70) of the
    spread), the sample deviation within 4 of its own relative deviations 1 / sqrt(140) = 8.5 % (a factor 1.34)."""
    name = "default128"
    sk = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, NOISE_SEED))
    m = keygen.pk_rows(sk.n)
    pk_s = sk.public_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    assert len(pk_s) == m == 20448 and pk_s.nbytes == 40 + 4 * m
    f = io.BytesIO()
    client.write_seeded_ciphertexts(f, pk_s)                                 # a public key is an RSC1 file
    back = client.read_seeded_ciphertexts(io.BytesIO(f.getvalue()), n=630)
    pk = back.expand()
    assert pk.shape == (m, 631)
    bits = np.random.default_rng(7).integers(0, 2, 70)
    ct = keygen.pk_encrypt(pk, np.where(bits != 0, E8, -E8), RAND_SEED)
    assert np.array_equal(sk.decrypt_bits(ct), bits)
    err = (sk.phase(ct).astype(np.int64) - np.where(bits != 0, E8, -E8)) / 2.0 ** 32
    e = sk.phase(pk).astype(np.float64) / 2.0 ** 32
    offset, spread = e.sum() / 2, np.sqrt((e * e).sum()) / 2
    print("largest error %.3g, mean %.3g (key's offset %.3g), deviation %.3g (key's spread %.3g)"
          % (np.abs(err).max(), err.mean(), offset, err.std(), spread))
    assert np.abs(err).max() < 1 / 8
    assert abs(spread - client.SECALPHA * np.sqrt(m / 4)) < 0.05 * spread     # 20,448 Gaussians: 0.5 % relative deviation
    assert abs(err.mean() - offset) < 4 * spread / np.sqrt(70)
    assert spread / 1.34 < err.std() < spread * 1.34


def test_symbol_is_in_the_header_the_library_and_the_binding():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_pk_encrypt_dev\(rs_ctx\* ctx, int32_t\* ct, const int32_t\* pk, size_t m, const int32_t\* mu, "
                     r"const int32_t\* base,\s+size_t B, const uint8_t\* rand_seed, uint64_t first, void\* stream\);", header)
    assert "domain 9   selection bits" in header
    assert "rs_pk_encrypt_dev" in redsec_amd.ABI_SYMBOLS
    assert hasattr(redsec_amd.load_library(), "rs_pk_encrypt_dev")
    for f in ("pk_encrypt", "pk_encrypt_bits"):
        assert callable(getattr(redsec_amd.Backend, f))
    assert callable(client.SecretKeySet.public_key)
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_pubkey", "rs_pubkey.hip", [])' in build


def test_failure_without_a_context_matches_expand_ciphertexts():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    rc_e = L.rs_expand_ciphertexts_dev(None, p, RAND_SEED, 0, p, 1, None)
    msg_e = L.rs_last_error()
    rc_p = L.rs_pk_encrypt_dev(None, p, p, 1, None, None, 1, RAND_SEED, 0, None)
    assert rc_p == rc_e != 0 and L.rs_last_error() == msg_e
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(redsec_amd.RedsecHipError, match="no HIP device"):
            redsec_amd.Backend(redsec_amd.params("default128"))


def test_new_kernel_holds_zero_scratch_and_little_lds():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    hits = {n: k for n, k in ks.items() if "17pk_encrypt_kernel" in n}
    assert len(hits) == 1, sorted(hits)
    for n, k in hits.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] <= 4096, (n, k)
