"""Device decryption and the exact noise audit of evaluation keys without a GPU (include/redsec_hip.h rs_phase_dev, rs_audit_keys_dev,
rs_audit_compressed_keys_dev): the numpy restatement against the generator's noise streams, the kernels'
own per-word functions (csrc/rs_audit.h, compiled into the lane emulator) against numpy, corrupted keys, the default limits, the
scratch budget of the new kernels and the bindings. Nothing here computes a phase in the product library: there is no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib
from redsec_amd import client, keygen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes(range(40, 72))
MASK_SEED = bytes(range(100, 132))
BK_STDEV, KS_STDEV = 2.0 ** -20, 2.0 ** -15     # non-zero noise words on every ring (the large rings' own deviations truncate to 0)
i32p = C.POINTER(C.c_int32)


def _p(a):
    return a.ctypes.data_as(i32p)


def _bk_gauss(seed, rows, N, stdev):
    return keygen.noise32(keygen.chacha20_words(seed, keygen.DOMAIN_BK_NOISE, np.asarray(rows), 4 * N), stdev)


def _ksk_gauss(seed, rows, base, stdev):
    rows = np.asarray(rows)
    e = keygen.noise32(keygen.chacha20_words(seed, keygen.DOMAIN_KS_NOISE, rows, 4), stdev)[:, 0]
    return np.where(rows % base != 0, e, 0).astype(np.int32)


@pytest.mark.parametrize("name,n", [("default128", 5), ("redsec_small_v2", 3), ("redsec_medium", 2)])
def test_numpy_audit_recovers_the_generators_noise_words(name, n):
    s = keygen._shape(name, n)
    N, l, t, base = s["N"], s["l"], s["t"], 1 << s["basebit"]
    lwe, tlwe = keygen.secret_keys(name, SEED, n)
    lwe[0], lwe[1] = 1, 0
    bk_rows, ksk_rows = np.arange(n * 2 * l), np.arange(N * t * base)
    want_bk, want_ksk = _bk_gauss(SEED, bk_rows, N, BK_STDEV), _ksk_gauss(SEED, ksk_rows, base, KS_STDEV)
    assert np.abs(want_bk).max() > 0 and np.abs(want_ksk).max() > 0
    # the full key
    bk, ksk = keygen.restate(name, SEED, lwe, tlwe, BK_STDEV, KS_STDEV)
    assert np.array_equal(keygen.bk_noise(name, lwe, tlwe, bk), want_bk)
    assert np.array_equal(keygen.ksk_noise(name, lwe, tlwe, ksk), want_ksk)
    limits = (int(np.abs(want_bk.astype(np.int64)).max()) // 2, int(np.abs(want_ksk.astype(np.int64)).max()) // 2)
    rep = keygen.audit(name, lwe, tlwe, bk, ksk, limits=limits)
    mag_b, mag_k = np.abs(want_bk.astype(np.int64)), np.abs(want_ksk.astype(np.int64))
    assert (rep["bk_max_abs"], rep["ksk_max_abs"]) == (mag_b.max(), mag_k.max())
    assert (rep["bk_over"], rep["ksk_over"]) == ((mag_b > limits[0]).sum(), (mag_k > limits[1]).sum()) and rep["bk_over"] > 0
    assert (rep["bk_words"], rep["ksk_words"], rep["ksk_zero_bad"]) == (n * 2 * l * N, N * t * (base - 1), 0)
    assert np.array_equal(rep["bk_noise"], want_bk) and np.array_equal(rep["ksk_noise"], want_ksk)
    ksk_bad = ksk.copy()
    ksk_bad.reshape(-1, n + 1)[base * 7, 2] = 5            # a v = 0 sample
    assert keygen.audit(name, lwe, tlwe, None, ksk_bad)["ksk_zero_bad"] == 1
    # the compressed key: the noise of the noise seed under the masks of the mask seed
    bb, kb = keygen.restate_compressed(name, MASK_SEED, SEED, lwe, tlwe, BK_STDEV, KS_STDEV)
    assert np.array_equal(keygen.bk_noise(name, lwe, tlwe, bb, mask_seed=MASK_SEED), want_bk)
    assert np.array_equal(keygen.ksk_noise(name, lwe, tlwe, kb, mask_seed=MASK_SEED), want_ksk)
    rep = keygen.audit(name, lwe, tlwe, bb, kb, mask_seed=MASK_SEED, limits=limits)
    assert (rep["bk_max_abs"], rep["bk_over"], rep["ksk_zero_bad"]) == (mag_b.max(), (mag_b > limits[0]).sum(), 0)
    # noiseless keys audit to zeros
    bk0, ksk0 = keygen.restate(name, SEED, lwe, tlwe, 0.0, 0.0)
    rep = keygen.audit(name, lwe, tlwe, bk0, ksk0)
    assert not rep["bk_noise"].any() and not rep["ksk_noise"].any() and rep["bk_max_abs"] == rep["ksk_max_abs"] == 0
    bb0, kb0 = keygen.restate_compressed(name, MASK_SEED, SEED, lwe, tlwe, 0.0, 0.0)
    rep = keygen.audit(name, lwe, tlwe, bb0, kb0, mask_seed=MASK_SEED)
    assert not rep["bk_noise"].any() and not rep["ksk_noise"].any()


def _emu():
    L = emu_lib.lib()
    L.rs_emu_phase.argtypes = [i32p, C.c_long, C.c_int, i32p, i32p]
    L.rs_emu_audit_bk_row.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint64, i32p, i32p, C.c_int, i32p, i32p]
    L.rs_emu_audit_ksk_word.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint64, i32p, i32p, C.c_int32, C.POINTER(C.c_int)]
    L.rs_emu_audit_ksk_word.restype = C.c_int32
    L.rs_emu_audit_reduce.argtypes = [i32p, C.c_long, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    return L


def _emu_bk_row(L, s, n, row, stored, lwe, tlwe, mask_seed=None):
    out = np.full(s["N"], 7, np.int32)
    stored = np.ascontiguousarray(stored, np.int32)
    L.rs_emu_audit_bk_row(0 if mask_seed is None else 1, mask_seed, s["N"], s["l"], s["Bgbit"], int(row), _p(stored), _p(lwe), n, _p(tlwe), _p(out))
    return out


def _emu_ksk_word(L, s, n, sample, stored, lwe, tlwe, mask_seed=None):
    stored = np.ascontiguousarray(stored, np.int32).ravel()
    bad = C.c_int(-1)
    i = (int(sample) >> s["basebit"]) // s["t"]
    e = L.rs_emu_audit_ksk_word(0 if mask_seed is None else 1, mask_seed, n, s["t"], s["basebit"], int(sample), _p(stored), _p(lwe), int(tlwe[i]),
                                C.byref(bad))
    return e, bad.value


@pytest.mark.parametrize("name,n", [("default128", 40), ("redsec_medium", 33), ("redsec_large", 6)])
def test_emulated_audit_kernels_equal_numpy(name, n):
    """N = 1024, 4096, 8192: bk rows 0, the last, and a c = 0 and a c = 1 row of a key bit equal to 1 and of one equal to 0; ksk samples
    with v = 0, j = 0 and j = t - 1; full and seeded, word for word against keygen.bk_noise / ksk_noise and the generator's Gaussians."""
    L = _emu()
    s = keygen._shape(name, n)
    N, l, t, base = s["N"], s["l"], s["t"], 1 << s["basebit"]
    lwe, tlwe = keygen.secret_keys(name, SEED, n)
    lwe[2], lwe[3] = 1, 0
    bk_rows = np.array([0, n * 2 * l - 1, 2 * 2 * l + 1, 2 * 2 * l + l + (l - 1), 3 * 2 * l + (l - 1), 3 * 2 * l + l])
    last_i = N - 1
    ksk_rows = np.array([0, 1, base - 1, (0 * t + t - 1) * base + 1, (5 * t + 0) * base, (5 * t + 0) * base + base - 1,
                         (last_i * t + t - 1) * base, (last_i * t + t - 1) * base + base - 1])
    bk, ksk = keygen.restate(name, SEED, lwe, tlwe, BK_STDEV, KS_STDEV, rows=(bk_rows, ksk_rows))
    bb, kb = keygen.restate_compressed(name, MASK_SEED, SEED, lwe, tlwe, BK_STDEV, KS_STDEV, rows=(bk_rows, ksk_rows))
    want_bk = keygen.bk_noise(name, lwe, tlwe, bk, bk_rows)
    assert np.array_equal(want_bk, _bk_gauss(SEED, bk_rows, N, BK_STDEV)) and want_bk.any()
    assert np.array_equal(want_bk, keygen.bk_noise(name, lwe, tlwe, bb, bk_rows, mask_seed=MASK_SEED))
    for r, row in enumerate(bk_rows):
        assert np.array_equal(_emu_bk_row(L, s, n, row, bk[r], lwe, tlwe), want_bk[r]), ("full", row)
        assert np.array_equal(_emu_bk_row(L, s, n, row, bb[r], lwe, tlwe, MASK_SEED), want_bk[r]), ("seeded", row)
    want_ksk = keygen.ksk_noise(name, lwe, tlwe, ksk, ksk_rows)
    assert np.array_equal(want_ksk, _ksk_gauss(SEED, ksk_rows, base, KS_STDEV)) and want_ksk.any()
    assert np.array_equal(want_ksk, keygen.ksk_noise(name, lwe, tlwe, kb, ksk_rows, mask_seed=MASK_SEED))
    for r, sample in enumerate(ksk_rows):
        assert _emu_ksk_word(L, s, n, sample, ksk[r], lwe, tlwe) == (want_ksk[r], 0), ("full", sample)
        assert _emu_ksk_word(L, s, n, sample, kb[r:r + 1], lwe, tlwe, MASK_SEED) == (want_ksk[r], 0), ("seeded", sample)
    # a v = 0 sample with a non-zero word (the body, or the last mask word) counts; a compressed body word there is ignored
    for word in (n, n - 1):
        bad = ksk[0].copy()
        bad[word] = 1
        assert _emu_ksk_word(L, s, n, ksk_rows[0], bad, lwe, tlwe) == (0, 1)
    assert _emu_ksk_word(L, s, n, ksk_rows[0], np.array([9], np.int32), lwe, tlwe, MASK_SEED) == (0, 0)


@pytest.mark.parametrize("dim", [350, 630, 1024, 6144, 8192])
def test_emulated_phase_equals_numpy(dim):
    L = _emu()
    rng = np.random.default_rng(dim)
    key = rng.integers(0, 2, dim).astype(np.int32)
    ct = rng.integers(-(1 << 31), 1 << 31, (5, dim + 1), dtype=np.int64).astype(np.int32)
    out = np.zeros(5, np.int32)
    L.rs_emu_phase(_p(ct), 5, dim, _p(key), _p(out))
    dot = (ct[:, :dim].view(np.uint32).astype(np.uint64) * key.astype(np.uint64)).sum(axis=-1)
    want = ((ct[:, dim].view(np.uint32).astype(np.uint64) - dot) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    assert np.array_equal(out, want)
    if dim in (350, 630):                      # the client's own phase
        sk = client.SecretKeySet.from_secret("redsec_small_v2" if dim == 350 else "default128", key, np.zeros(1024, np.int32))
        assert np.array_equal(out, sk.phase(ct))


@pytest.mark.parametrize("name,n", [("default128", 4), ("redsec_large", 2)])
def test_corrupted_words_change_exactly_the_predicted_noise_words(name, n):
    L = _emu()
    s = keygen._shape(name, n)
    N, l = s["N"], s["l"]
    lwe, tlwe = keygen.secret_keys(name, SEED, n)
    rows = np.array([1, l + 1])                    # a c = 0 and a c = 1 row
    bk, _ = keygen.restate(name, SEED, lwe, tlwe, BK_STDEV, KS_STDEV, rows=(rows, None))
    set_bits = np.flatnonzero(tlwe)
    delta, pos = 12345, N - 3
    for r, row in enumerate(rows):
        clean = _emu_bk_row(L, s, n, row, bk[r], lwe, tlwe)
        body = bk[r].copy()
        body[1, 77] = np.int32((int(body[1, 77]) + (1 << 20) + (1 << 31)) % (1 << 32) - (1 << 31))
        diff = (_emu_bk_row(L, s, n, row, body, lwe, tlwe).astype(np.int64) - clean) % (1 << 32)
        assert np.flatnonzero(diff).tolist() == [77] and diff[77] == 1 << 20
        mask = bk[r].copy()
        mask[0, pos] = np.int32((int(mask[0, pos]) + delta + (1 << 31)) % (1 << 32) - (1 << 31))
        diff = (_emu_bk_row(L, s, n, row, mask, lwe, tlwe).astype(np.int64) - clean) % (1 << 32)
        want = np.zeros(N, np.int64)
        for m in set_bits:                         # X^m a: a[pos] lands at pos + m, negated once it wraps; the noise is b - a*S
            want[(pos + m) % N] = (-delta if pos + m < N else delta) % (1 << 32)
        assert np.array_equal(diff, want) and np.count_nonzero(diff) == len(set_bits)


def test_report_reduction_and_default_limits():
    L = _emu()
    rng = np.random.default_rng(3)
    e = rng.integers(-5000, 5000, 10007).astype(np.int32)
    for extreme, want_max in ((None, None), (-(1 << 31), 1 << 31), ((1 << 31) - 1, (1 << 31) - 1)):
        w = e.copy()
        if extreme is not None:
            w[4321] = extreme
        mag = np.abs(w.astype(np.int64))
        for parts in (1, 64, 256):
            mx, over = C.c_uint32(), C.c_uint64()
            L.rs_emu_audit_reduce(_p(w), w.size, 3000, parts, C.byref(mx), C.byref(over))
            assert (mx.value, over.value) == (mag.max(), (mag > 3000).sum())
            assert want_max is None or mx.value == want_max
    zmax = np.sqrt(2 * 53 * np.log(2.0))           # Box-Muller with u1 >= 2^-53
    assert 8.57 < zmax < 8.58 == keygen.GAUSS_BOUND
    for name, (_, _, _, _, _, _, _, ks_stdev, bk_stdev) in client.PARAM_SETS.items():
        bk_limit, ksk_limit = keygen.noise_limits(name)
        for limit, sigma in ((bk_limit, bk_stdev), (ksk_limit, ks_stdev)):
            assert limit == int(np.floor(8.58 * sigma * 2.0 ** 32)) + 1 and limit > zmax * sigma * 2.0 ** 32 and limit < 2 ** 31
    # the extreme Gaussian itself: u1 = 2^-53, u2 = 0
    w = np.zeros((1, 4), np.uint32)
    assert abs(int(keygen.noise32(w, 2.0 ** -15)[0, 0])) <= keygen.noise_limits("default128")[1]


def test_new_kernels_hold_zero_scratch():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    hits = {n: k for n, k in ks.items() if re.search(r"16lwe_phase_kernel|15audit_bk_kernelILb[01]E|16audit_ksk_kernelILb[01]E", n)}
    assert len(hits) == 5, sorted(hits)
    for n, k in hits.items():
        assert k["scratch"] == 0 and k["lds"] <= 4096 and k["vgpr"] <= 64, (n, k)     # static LDS; the bk kernel's is dynamic (51 KB at N = 8192)


def test_audit_arithmetic_is_integer_only():
    """The audit must not share the generator's arithmetic: its sources include neither the split-key product nor a transform, and
    hold no floating-point type."""
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_audit.h", "rs_audit.hip"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\b(double|float)\b|rs_general\.h|rs_fft\.h", code), f


def test_audit_bindings_exist():
    import redsec_amd
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    L = redsec_amd.load_library()
    for sym in ("rs_phase_dev", "rs_audit_keys_dev", "rs_audit_compressed_keys_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and re.search(r"\bint %s\(rs_ctx\* ctx" % sym, header) and hasattr(L, sym)
    assert "typedef struct rs_key_audit" in header
    for f in ("phase", "audit_keys", "audit_compressed_keys"):
        assert callable(getattr(redsec_amd.Backend, f))
    for f in ("noise_limits", "bk_noise", "ksk_noise", "audit"):
        assert callable(getattr(keygen, f))
