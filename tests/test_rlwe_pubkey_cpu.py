"""Compact RLWE public keys without a GPU (include/redsec_hip.h rs_rlwe_pk_encrypt_dev, rs_rlwe_extract_dev; INTEGRATION.md section
17): the numpy restatement decrypts exactly without noise and with the predicted noise with it, extraction has the phase of its
coefficient under the ring key read as an LWE key, RSP1 files round-trip, the seed and deviation rules hold, the kernels' own
helpers (compiled into the lane emulator) and the emulated kernel agree with numpy, and the symbols are everywhere they belong."""
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
KEY_SEED = bytes(range(9, 41))
ROWS = (0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1)
_i32p = C.POINTER(C.c_int32)


def _emu():
    L = emu_lib.lib()
    L.rs_emu_rlwe_select.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    L.rs_emu_rlwe_select.restype = None
    L.rs_emu_rlwe_term_index.argtypes = [C.c_int, C.c_int, C.c_int]
    L.rs_emu_rlwe_extract_word.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.rs_emu_rlwe_tile.argtypes = []
    L.rs_emu_rlwe_pk_encrypt.argtypes = [_i32p, _i32p, C.c_long, C.c_int, C.c_char_p, C.c_uint64, C.c_double, _i32p]
    L.rs_emu_rlwe_pk_encrypt.restype = None
    L.rs_emu_rlwe_extract.argtypes = [_i32p, C.c_long, C.c_int, _i32p]
    L.rs_emu_rlwe_extract.restype = None
    return L


def _key(name, seed=KEY_SEED, stdev=None, mask_seed=MASK_SEED, noise_seed=NOISE_SEED):
    sk = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, seed))
    return sk, sk.rlwe_public_key(mask_seed, noise_seed, stdev)


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("count", [1, 1023, 1024, 1027])
def test_noise_free_key_decrypts_exactly(count):
    """stdev = 0 in the key and in the ciphertexts: the phase is mu in the first `count` slots and 0 in the padding, word for word,
    across 2^32 in `first`."""
    sk, pk = _key("redsec_small_v2", stdev=0.0)
    mu = _words(np.random.default_rng(count), count)
    first = (1 << 32) - 1
    ct = keygen.rlwe_pk_encrypt(pk.expand(), mu, RAND_SEED, first, stdev=0.0)
    R = -(-count // 1024)
    assert ct.shape == (R, 2, 1024) and ct.dtype == np.int32
    ph = keygen.rlwe_phase(ct, sk.tlwe_key).ravel()
    assert np.array_equal(ph[:count], mu) and not ph[count:].any()
    # the mask half is a * u, the product with the selector of the row: nothing of mu in it
    u = keygen.rlwe_pk_selector(RAND_SEED, 1024, first, R)
    assert u.shape == (R, 1024) and set(np.unique(u)) <= {0, 1} and 0.4 < u.mean() < 0.6
    a = pk.expand()[0].view(np.uint32).astype(np.uint64)
    k = 700                                                                  # one coefficient by the plain definition
    idx = (k - np.arange(1024)) % 1024
    sign = np.where(np.arange(1024) > k, -1, 1).astype(np.int64)
    want = int((a[idx].astype(np.int64) * sign * u[0]).sum()) & 0xFFFFFFFF
    assert int(ct[0, 0, k]) & 0xFFFFFFFF == want


@pytest.mark.parametrize("name", ["default128", "redsec_small_v2"])
def test_noisy_key_has_the_predicted_phase_error(name):
    """The error e*u + e2 - e1*S has deviation alpha sqrt(N + 1) over keys and encryptions (N/2 set bits in u and in S on average). For
    ONE key the e*u part splits, as in section 16, into a spread over u (alpha sqrt(N/4)) and an offset fixed by the key, which along
    the coefficients is a random walk with steps e_k: a single key's sample deviation lies 0.96 +- 0.08 of the formula. So the sample
    is four keys x four ciphertexts and the deviation is the root mean square about the predicted mean, zero. At alpha = 2^-30 (the
    REDsec set) dtot32's truncation toward zero of a word of deviation 4 lowers the deviation of every noise word to 0.906 alpha: the
    expected ratio there is 0.91, still inside the 25 %. The largest error stays below 8 alpha sqrt(N + 1)."""
    alpha = keygen.rlwe_default_stdev(name)
    assert alpha == client.PARAM_SETS[name][8]
    N = 1024
    sigma = alpha * np.sqrt(N + 1)
    errs = []
    for k in range(4):
        seeds = [bytes((b + 37 * k + 11 * q) & 0xFF for b in range(32)) for q in range(4)]
        sk, pk = _key(name, seeds[0], None, seeds[1], seeds[2])
        mu = _words(np.random.default_rng(k), 4 * N)
        ct = keygen.rlwe_pk_encrypt(pk.expand(), mu, seeds[3], 5, stdev=alpha)
        errs.append((keygen.rlwe_phase(ct, sk.tlwe_key).ravel().view(np.uint32) - mu.view(np.uint32)).view(np.int32) / 2.0 ** 32)
    err = np.concatenate(errs)
    rms, worst = np.sqrt(np.mean(err * err)), np.abs(err).max()
    print("%s: rms %.3g, alpha sqrt(N + 1) %.3g (ratio %.3f), largest %.3g = %.2f sigma" % (name, rms, sigma, rms / sigma, worst, worst / sigma))
    assert err.size == 16 * N
    assert abs(rms - sigma) < 0.25 * sigma
    assert worst < 8 * sigma


def test_extracted_rows_have_the_phase_of_their_coefficient():
    """Row rN + c of rlwe_extract under the ring key read as an LWE key (plain dot product) has the phase of coefficient c of
    ciphertext r, word for word; the index helper of the kernel says the same."""
    sk, pk = _key("redsec_small_v2")
    N, count = 1024, 1024 + 3
    mu = _words(np.random.default_rng(3), count)
    ct = keygen.rlwe_pk_encrypt(pk.expand(), mu, RAND_SEED, 0, stdev=2.0 ** -30)
    rows = keygen.rlwe_extract(ct, count)
    assert rows.shape == (count, N + 1) and rows.dtype == np.int32
    S = sk.tlwe_key.astype(np.uint64)
    dot = (rows[:, :N].view(np.uint32).astype(np.uint64) * S).sum(axis=1)
    ph = ((rows[:, N].view(np.uint32).astype(np.uint64) - dot) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    assert np.array_equal(ph, keygen.rlwe_phase(ct, sk.tlwe_key).ravel()[:count])
    assert np.abs((ph.view(np.uint32) - mu.view(np.uint32)).view(np.int32)).max() < 8 * 2.0 ** -30 * np.sqrt(N + 1) * 2.0 ** 32
    assert keygen.rlwe_extract(ct, 0).shape == (0, N + 1)
    L = _emu()
    neg = C.c_int(0)
    for r, c, j in ((0, 0, 0), (0, 0, 1), (0, 5, 5), (0, 5, 6), (0, 1023, 1023), (1, 2, 1023), (1, 2, 0)):
        idx = L.rs_emu_rlwe_extract_word(N, c, j, C.byref(neg))
        want = int(ct[r, 0, idx]) * (-1 if neg.value else 1)
        assert (int(rows[r * N + c, j]) - want) % (1 << 32) == 0, (r, c, j)
        assert (neg.value == 1) == (j > c) and idx == (c - j) % N


def test_rsp1_files_round_trip_and_reject_damage():
    sk, pk = _key("redsec_small_v2")
    assert isinstance(pk, client.RlwePublicKey) and pk.name == "redsec_small_v2" and pk.mask_seed == MASK_SEED
    assert pk.body.shape == (1024,) and pk.body.dtype == np.int32 and pk.nbytes == 32 + 4 * 1024
    full = pk.expand()
    assert full.shape == (2, 1024) and full.dtype == np.int32
    assert np.array_equal(full[0], keygen.rlwe_pk_mask(MASK_SEED, 1024)) and np.array_equal(full[1], pk.body)
    assert np.array_equal(full[0].view(np.uint32), keygen.chacha20_words(MASK_SEED, 10, 0, 1024))
    # b - a*S is the key's noise: small, not zero
    e = keygen.rlwe_phase(full[None], sk.tlwe_key)[0]
    assert 0 < np.abs(e).max() < 8.58 * 2.0 ** -30 * 2.0 ** 32 + 1
    f = io.BytesIO()
    client.write_rlwe_public_key(f, pk)
    raw = f.getvalue()
    assert raw[:4] == b"RSP1" and len(raw) == client._RS_HEADER.itemsize + pk.nbytes
    back = client.read_rlwe_public_key(io.BytesIO(raw))
    assert back.name == pk.name and back.mask_seed == pk.mask_seed and np.array_equal(back.body, pk.body)
    for damaged in (raw[:-4], raw + b"\0\0\0\0", raw[:40], raw[:3], b"RSC1" + raw[4:]):
        with pytest.raises(ValueError):
            client.read_rlwe_public_key(io.BytesIO(damaged))
    with pytest.raises(ValueError):
        client.read_seeded_ciphertexts(io.BytesIO(raw))                      # an RSP1 file is not an RSC1 file


def test_equal_seeds_and_vanishing_default_deviations_are_refused():
    sk = client.SecretKeySet.from_secret("redsec_small_v2", *keygen.secret_keys("redsec_small_v2", KEY_SEED))
    with pytest.raises(ValueError, match="equal"):
        sk.rlwe_public_key(MASK_SEED, MASK_SEED)
    with pytest.raises(ValueError, match="equal"):
        keygen.rlwe_public_key("redsec_small_v2", sk.tlwe_key, MASK_SEED, MASK_SEED, 0.0)
    a, b = sk.rlwe_public_key(), sk.rlwe_public_key()                        # fresh seeds by default
    assert a.mask_seed != b.mask_seed and not np.array_equal(a.body, b.body)
    # bk_stdev = 2^-45 and 2^-46 truncate to zero in a 32-bit torus (2^-36 of redsec_small too): no silent noise-free key
    for name in ("redsec_medium", "redsec_large", "redsec_small"):
        big = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, KEY_SEED))
        with pytest.raises(ValueError, match="explicit stdev"):
            big.rlwe_public_key(MASK_SEED, NOISE_SEED)
        with pytest.raises(ValueError, match="explicit stdev"):
            keygen.rlwe_default_stdev(name)
        assert big.rlwe_public_key(MASK_SEED, NOISE_SEED, stdev=2.0 ** -30).body.shape == (big.N,)
    for name in ("default128", "redsec_small_v2"):
        assert keygen.rlwe_default_stdev(name) == client.PARAM_SETS[name][8] >= keygen.MIN_STDEV
    with pytest.raises(ValueError):
        keygen.rlwe_pk_encrypt(a.expand(), np.zeros(1025, np.int64), RAND_SEED, (1 << 64) - 1, stdev=0.0)   # two rows from the last one
    assert keygen.rlwe_pk_encrypt(a.expand(), np.zeros(0, np.int64), RAND_SEED, stdev=0.0).shape == (0, 2, 1024)


def test_an_explicit_deviation_serves_the_large_rings():
    """N = 4096 with an explicit 2^-30: noise-free slots decrypt, the error has the predicted size."""
    name, N = "redsec_medium", 4096
    sk, pk = _key(name, stdev=2.0 ** -30)
    assert pk.nbytes == 32 + 4 * N
    mu = _words(np.random.default_rng(4), N + 1)
    ct = keygen.rlwe_pk_encrypt(pk.expand(), mu, RAND_SEED, 0, stdev=2.0 ** -30)
    err = (keygen.rlwe_phase(ct, sk.tlwe_key).ravel()[:N + 1].view(np.uint32) - mu.view(np.uint32)).view(np.int32) / 2.0 ** 32
    assert np.abs(err).max() < 8 * 2.0 ** -30 * np.sqrt(N + 1)
    assert np.any(err != 0)


@pytest.mark.parametrize("N", [1024, 4096, 8192])
def test_emulated_selector_and_index_helpers_equal_numpy(N):
    L = _emu()
    for row in ROWS:
        words = np.full(N // 32, 0xDEADBEEF, np.uint32)
        L.rs_emu_rlwe_select(RAND_SEED, row, N, words.ctypes.data_as(C.POINTER(C.c_uint32)))
        got = ((words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).ravel().astype(np.uint8)
        want = keygen.rlwe_pk_selector(RAND_SEED, N, row, 1)
        assert want.shape == (1, N) and np.array_equal(got, want[0]), (N, row)
        assert np.array_equal(words, keygen.chacha20_words(RAND_SEED, 12, row, N // 32))
    # coefficient k of X^j p is word k - j + N of (-p, p): p[k - j] for j <= k, -p[N + k - j] above
    p = _words(np.random.default_rng(N), N).view(np.uint32)
    ext = np.concatenate([np.uint32(0) - p, p])
    for k, j in ((0, 0), (0, 1), (0, N - 1), (N - 1, 0), (N - 1, N - 1), (511, 512), (512, 511), (N // 2, N // 2 + 1)):
        i = L.rs_emu_rlwe_term_index(N, k, j)
        assert 0 < i < 2 * N and int(ext[i]) == (int(p[k - j]) if j <= k else -int(p[N + k - j]) & 0xFFFFFFFF), (k, j)
    assert L.rs_emu_rlwe_tile() == 512 and N % L.rs_emu_rlwe_tile() == 0
    for domain in list(range(1, 10)) + [10, 11, 13]:
        assert np.mean(keygen.chacha20_words(RAND_SEED, domain, 0, 32) == keygen.chacha20_words(RAND_SEED, 12, 0, 32)) < 0.1


@pytest.mark.parametrize("N,count,stdev,first", [(1024, 1, 0.0, 0), (1024, 2 * 1024 + 5, 2.0 ** -25, (1 << 32) - 1),
                                                 (4096, 4097, 2.0 ** -25, 3), (8192, 8193, 0.0, (1 << 64) - 2)])
def test_emulated_kernels_equal_numpy_word_for_word(N, count, stdev, first):
    """rlwe_pk_encrypt_kernel and rlwe_extract_kernel as the emulator walks them -- the staged window of (-p, p), a 4-word chunk per
    thread and four selector bits, the seven live words -- against the restatement, over every tile of every ring."""
    L = _emu()
    rng = np.random.default_rng(N + count)
    pk, mu = _words(rng, 2, N), _words(rng, count)
    R = -(-count // N)
    got = np.full((R, 2, N), 0x5A5A5A5A, np.int32)
    L.rs_emu_rlwe_pk_encrypt(pk.ctypes.data_as(_i32p), mu.ctypes.data_as(_i32p), count, N, RAND_SEED, first, stdev, got.ctypes.data_as(_i32p))
    want = keygen.rlwe_pk_encrypt(pk, mu, RAND_SEED, first, stdev=stdev)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    rows = np.zeros((count, N + 1), np.int32)
    L.rs_emu_rlwe_extract(got.ctypes.data_as(_i32p), count, N, rows.ctypes.data_as(_i32p))
    assert np.array_equal(rows, keygen.rlwe_extract(want, count))


def test_symbols_are_in_the_header_the_library_the_binding_and_the_recipe():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_rlwe_pk_encrypt_dev\(rs_ctx\* ctx, int32_t\* rlwe, const int32_t\* pk, const int32_t\* mu, size_t count, "
                     r"const uint8_t\* rand_seed,\s+uint64_t first, double stdev, void\* stream\);", header)
    assert re.search(r"int rs_rlwe_extract_dev\(rs_ctx\* ctx, int32_t\* u, const int32_t\* rlwe, size_t count, void\* stream\);", header)
    for d in ("domain 10  public-key mask", "domain 11  public-key noise", "domain 12  selector u", "domain 13  encryption noise"):
        assert d in header and d in (keygen.__doc__ or "") and d in open(os.path.join(ROOT, "INTEGRATION.md")).read(), d
    L = redsec_amd.load_library()
    for sym in ("rs_rlwe_pk_encrypt_dev", "rs_rlwe_extract_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and hasattr(L, sym)
    for f in ("rlwe_pk_encrypt", "rlwe_extract", "rlwe_unpack", "rlwe_pk_encrypt_image"):
        assert callable(getattr(redsec_amd.Backend, f))
    assert (keygen.DOMAIN_RLWE_MASK, keygen.DOMAIN_RLWE_NOISE, keygen.DOMAIN_RLWE_SELECT, keygen.DOMAIN_RLWE_ENC_NOISE) == (10, 11, 12, 13)
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_rlwe", "rs_rlwe.hip", [])' in build


def test_failure_without_a_context_matches_pk_encrypt():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    rc_p = L.rs_pk_encrypt_dev(None, p, p, 1, None, None, 1, RAND_SEED, 0, None)
    msg_p = L.rs_last_error()
    assert rc_p != 0
    assert L.rs_rlwe_pk_encrypt_dev(None, p, p, p, 1, RAND_SEED, 0, 0.0, None) == rc_p and L.rs_last_error() == msg_p
    assert L.rs_rlwe_extract_dev(None, p, p, 1, None) == rc_p and L.rs_last_error() == msg_p


def test_new_kernels_hold_zero_scratch_and_no_static_lds():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    enc = {n: k for n, k in ks.items() if "22rlwe_pk_encrypt_kernel" in n}
    ext = {n: k for n, k in ks.items() if "19rlwe_extract_kernel" in n}
    assert len(enc) == 1 and len(ext) == 1, (sorted(enc), sorted(ext))
    for k in enc.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, k   # the LDS is dynamic: (N + 512 + N / 32) words
    for k in ext.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 32 and k["lds"] == 0, k
