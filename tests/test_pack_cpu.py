"""Packed results without a GPU (include/redsec_hip.h rs_pack_dev): the numpy restatement keeps the phase
of every sample up to exactly the digits' rounding under a noise-free key and up to the predicted noise under a real one, the emulated
kernel (its own workgroup / segment / row / four-slot walk, compiled into the lane emulator) equals numpy word for word, a packed
ciphertext unpacks into rows of the same phase, RSK1 files round-trip, the seed and deviation rules hold, and the symbol is
everywhere it belongs."""
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
MASK_SEED = bytes(range(140, 172))
NOISE_SEED = bytes(range(7, 39))
KEY_SEED = bytes(range(9, 41))
_i32p = C.POINTER(C.c_int32)
PAIRS = [(4, 5), (2, 8), (8, 4), (3, 5), (1, 32)]


def _emu():
    L = emu_lib.lib()
    L.rs_emu_pack.argtypes = [_i32p, C.c_long, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, _i32p]
    L.rs_emu_pack.restype = None
    L.rs_emu_pack_offset.argtypes = [C.c_int, C.c_int]
    L.rs_emu_pack_offset.restype = C.c_uint32
    L.rs_emu_pack_digit.argtypes = [C.c_uint32, C.c_int, C.c_int]
    L.rs_emu_pack_digit.restype = C.c_uint32
    L.rs_emu_pack_slot_blocks.argtypes = [C.c_long, C.c_int]
    L.rs_emu_pack_chunks.argtypes = [C.c_int]
    L.rs_emu_pack_groups.argtypes = [C.c_long, C.c_int, C.c_int]
    L.rs_emu_pack_groups.restype = C.c_long
    L.rs_emu_pack_window_word.argtypes = [C.c_int] * 6
    return L


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _secret(name, n, seed=KEY_SEED):
    lwe, tlwe = keygen.secret_keys(name, seed, n)
    return client.SecretKeySet.from_secret(name, lwe, tlwe)


def _samples(sk, mu, seed, alpha=0.0):
    return sk.encrypt_torus(mu, alpha, seed)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _rounding(sk, ct, basebit, t):
    """sum_i s_i (a_i - the digits' value of a_i): what the packing adds to a phase under a noise-free key, computed from the mask
    words alone."""
    a = ct[:, :sk.n].astype(np.int64) & 0xFFFFFFFF
    bits = t * basebit
    off = (1 << (31 - bits)) if bits < 32 else 0
    kept = (((a + off) & 0xFFFFFFFF) >> (32 - bits)) << (32 - bits)
    return (((a - kept) * sk.lwe_key.astype(np.int64)).sum(axis=1) & 0xFFFFFFFF).astype(np.uint32)


@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, 2 * 1024 + 5])
def test_noise_free_key_keeps_every_phase_up_to_exactly_the_rounding(count):
    """stdev = 0 in the key: the phase of slot c is the phase of sample c plus sum_i s_i (a_i - digits(a_i)), word for word; the
    padding slots are exactly zero."""
    N, n, (basebit, t) = 1024, 16, keygen.pack_default("redsec_small_v2")
    sk = _secret("redsec_small_v2", n)
    key = sk.packing_key(basebit, t, MASK_SEED, NOISE_SEED, stdev=0.0)
    mu = _words(np.random.default_rng(count), count)
    ct = _samples(sk, mu, count, 2.0 ** -20)
    rlwe = keygen.pack(ct, key.expand(), basebit, t)
    R = -(-count // N)
    assert rlwe.shape == (R, 2, N) and rlwe.dtype == np.int32
    ph = keygen.rlwe_phase(rlwe, sk.tlwe_key).ravel()
    want = _u32(sk.phase(ct)) + _rounding(sk, ct, basebit, t)
    assert np.array_equal(_u32(ph[:count]), want) and not ph[count:].any()
    assert np.array_equal(sk.packed_phase(rlwe, count), ph[:count])
    # the rounding is at most n 2^(31 - t basebit), half a unit of the last digit per key bit
    assert np.abs((want - _u32(sk.phase(ct))).view(np.int32)).max() <= n << (31 - t * basebit)


NOISY_SHAPE = dict(name="default128", n=8, basebit=4, t=5, count=256, keys=48, stdev=2.0 ** -25)


def test_noisy_keys_have_the_predicted_packing_error():
    """48 independent keys at N = 1024, n = 8, (basebit, t) = (4, 5), 256 slots, sigma_k = 2^-25 (NOISY_SHAPE): the error of a slot is
    sum_{i,j} (D_ij e_ij)[c] plus the rounding. The digits are unsigned, mean (2^basebit - 1) / 2: 73 % of the variance is that mean
    times a sliding sum of the key's noise words, fixed by the key and correlated along the slots, so single keys scatter widely.
    Measured with this file: root mean square 0.986 of pack_sigma over the 48 keys (0.934 over the first 16), single keys 0.57 ..
    1.55 with standard deviation 0.234, hence 0.034 for the pooled value; largest error 3.66 sigma, mean 0.07 sigma. The band is
    +-0.15, four and a half of those pooled deviations. Hard conditions: every +-1/8 message decrypts, the largest error is below
    8 sigma, the mean within one sigma of zero."""
    s = NOISY_SHAPE
    N = 1024
    sigma = keygen.pack_sigma(s["n"], N, s["basebit"], s["t"], s["count"], s["stdev"])
    errs, per_key = [], []
    for k in range(s["keys"]):
        seeds = [bytes((b + 41 * k + 13 * q) & 0xFF for b in range(32)) for q in range(3)]
        sk = _secret(s["name"], s["n"], seeds[0])
        key = sk.packing_key(s["basebit"], s["t"], seeds[1], seeds[2], s["stdev"])
        bits = np.random.default_rng(k).integers(0, 2, s["count"])
        ct = sk.encrypt_bits(bits, seed=100 + k)
        rlwe = keygen.pack(ct, key.expand(), s["basebit"], s["t"])
        assert np.array_equal(sk.decrypt_packed_bits(rlwe, s["count"]), bits)
        e = (_u32(sk.packed_phase(rlwe, s["count"])) - _u32(sk.phase(ct))).view(np.int32) / 2.0 ** 32
        errs.append(e)
        per_key.append(np.sqrt(np.mean(e * e)) / sigma)
    err = np.concatenate(errs)
    rms, worst, mean = np.sqrt(np.mean(err * err)), np.abs(err).max(), err.mean()
    print("pack_sigma %.4g, rms %.4g (ratio %.3f), single keys %.3f .. %.3f (std %.3f), largest %.2f sigma, mean %.3f sigma"
          % (sigma, rms, rms / sigma, min(per_key), max(per_key), np.std(per_key), worst / sigma, mean / sigma))
    assert err.size == s["keys"] * s["count"]
    assert abs(rms / sigma - 1.0) < 0.15
    assert worst < 8 * sigma
    assert abs(mean) < sigma


def _check_emulator(N, n, count, basebit, t):
    L = _emu()
    rng = np.random.default_rng(N + 3 * n + count + 100 * basebit + t)
    key, ct = _words(rng, n, t, 2, N), _words(rng, count, n + 1)
    R = -(-count // N)
    got = np.full((R, 2, N), 0x5A5A5A5A, np.int32)
    L.rs_emu_pack(ct.ctypes.data_as(_i32p), count, n, N, key.ctypes.data_as(_i32p), basebit, t, got.ctypes.data_as(_i32p))
    want = keygen.pack(ct, key, basebit, t)
    assert np.array_equal(got, want), (N, n, count, basebit, t, np.argwhere(got != want)[:4].tolist())
    return want


@pytest.mark.parametrize("N,n,count", [(1024, 16, 1), (1024, 37, 2 * 1024 + 5), (4096, 8, 4097), (8192, 5, 8193)])
def test_emulated_kernel_equals_numpy_on_every_ring(N, n, count):
    """pack_init_kernel and pack_kernel as the emulator walks them against the restatement at (4, 5): one slot; three ciphertexts with a
    ragged last one and n = 37, no multiple of the index chunk of 8 (the last chunk has 5 indices); four and eight slot blocks on
    the large rings with n below one chunk, the last ciphertext with one slot."""
    want = _check_emulator(N, n, count, 4, 5)
    assert want.shape == (-(-count // N), 2, N)


@pytest.mark.parametrize("basebit,t", PAIRS)
def test_emulated_kernel_equals_numpy_for_every_digit_shape(basebit, t):
    """(2, 8) and (8, 4): the narrowest and widest digits of 16 and 32 bits; (3, 5): a basebit that does not divide 32; (1, 32) and
    (8, 4): all 32 bits, offset 0. At one slot (N = 1024, n = 16) and at 1,025 slots: two ciphertexts, two slot blocks' worth of
    window arithmetic in the first."""
    _check_emulator(1024, 16, 1, basebit, t)
    _check_emulator(1024, 16, 1025, basebit, t)


def test_emulated_helpers_equal_numpy():
    L = _emu()
    rng = np.random.default_rng(5)
    a = _words(rng, 64)
    for basebit, t in PAIRS:
        off = L.rs_emu_pack_offset(basebit, t)
        assert off == ((1 << (31 - t * basebit)) if t * basebit < 32 else 0)
        want = keygen.pack_digits(a, basebit, t)
        got = np.array([[L.rs_emu_pack_digit((int(x) + off) & 0xFFFFFFFF, basebit, j) for j in range(t)] for x in _u32(a)], np.uint32)
        assert np.array_equal(got, want), (basebit, t)
        assert want.max() < 1 << basebit
    assert L.rs_emu_pack_offset(8, 4) == 0 and L.rs_emu_pack_offset(1, 32) == 0 and L.rs_emu_pack_offset(4, 4) == 1 << 15
    # coefficient k0 + x of X^(c0 + cc) p is word k - c + N of (-p, p), as rs_rlwe.h places it
    for N, k0, c0, cpad, x, cc in ((1024, 0, 0, 4, 0, 3), (1024, 512, 0, 1024, 511, 1023), (8192, 7680, 7168, 1024, 0, 1023),
                                   (8192, 0, 7168, 1024, 0, 1023), (4096, 512, 1024, 12, 3, 9)):
        assert L.rs_emu_pack_window_word(N, k0, c0, cpad, x, cc) == (k0 + x) - (c0 + cc) + N
        assert 0 <= L.rs_emu_pack_window_word(N, k0, c0, cpad, 0, cpad - 1) and L.rs_emu_pack_window_word(N, k0, c0, cpad, 511, 0) < 2 * N
    assert L.rs_emu_pack_tile() == 512 and L.rs_emu_pack_slots() == 1024
    assert L.rs_emu_pack_slot_blocks(1, 1024) == 1 and L.rs_emu_pack_slot_blocks(5 * 1024, 1024) == 1
    assert L.rs_emu_pack_slot_blocks(4097, 4096) == 4 and L.rs_emu_pack_slot_blocks(1025, 8192) == 2
    # index chunks of 8: n = 37 has five, the last of 5 indices; the grid is tiles x 2 x slot blocks x chunks x ciphertexts
    assert [L.rs_emu_pack_chunks(n) for n in (1, 8, 9, 37, 630)] == [1, 1, 2, 5, 79]
    assert L.rs_emu_pack_groups(64, 630, 1024) == 2 * 2 * 79 and L.rs_emu_pack_groups(8193, 5, 8192) == 2 * 16 * 2 * 8
    for domain in range(1, 14):
        assert np.mean(keygen.chacha20_words(MASK_SEED, domain, 3, 32) == keygen.chacha20_words(MASK_SEED, 14, 3, 32)) < 0.1
        assert np.mean(keygen.chacha20_words(MASK_SEED, domain, 3, 32) == keygen.chacha20_words(MASK_SEED, 15, 3, 32)) < 0.1


def test_pack_then_unpack_gives_rows_of_the_packed_phase():
    """keygen.rlwe_extract of a packed ciphertext: row rN + c under the ring key read as an LWE key has the phase of slot c, which is
    the phase of sample rN + c up to the packing error."""
    N, n, count, (basebit, t) = 1024, 12, 1024 + 7, (4, 5)
    sk = _secret("redsec_small_v2", n)
    key = sk.packing_key(basebit, t, MASK_SEED, NOISE_SEED)
    v = np.random.default_rng(8).integers(-2048, 2048, count)
    ct = _samples(sk, v * (1 << 20), 3, 2.0 ** -25)
    rlwe = keygen.pack(ct, key.expand(), basebit, t)
    rows = keygen.rlwe_extract(rlwe, count)
    S = sk.tlwe_key.astype(np.uint64)
    dot = (_u32(rows[:, :N]).astype(np.uint64) * S).sum(axis=1)
    ph = ((_u32(rows[:, N]).astype(np.uint64) - dot) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert np.array_equal(ph, _u32(sk.packed_phase(rlwe, count)))
    sigma = keygen.pack_sigma(n, N, basebit, t, count, 2.0 ** -30)
    assert np.abs((ph - _u32(sk.phase(ct))).view(np.int32)).max() < 8 * sigma * 2.0 ** 32
    assert np.array_equal(sk.decrypt_packed_ints(rlwe, count), v) and np.array_equal(sk.decrypt_ints(ct), v)


def test_rsk1_files_round_trip_and_reject_damage():
    sk = _secret("redsec_small_v2", 6)
    key = sk.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    assert isinstance(key, client.PackingKey) and (key.name, key.n, key.basebit, key.t) == ("redsec_small_v2", 6, 4, 5)
    assert key.body.shape == (6, 5, 1024) and key.body.dtype == np.int32 and key.nbytes == 32 + 4 * 6 * 5 * 1024
    full = key.expand()
    assert full.shape == (6, 5, 2, 1024) and full.dtype == np.int32 and np.array_equal(full[:, :, 1], key.body)
    assert np.array_equal(_u32(full[2, 3, 0]), keygen.chacha20_words(MASK_SEED, 14, 2 * 5 + 3, 1024))
    assert np.array_equal(keygen.pack_key("redsec_small_v2", sk.lwe_key, sk.tlwe_key, MASK_SEED, NOISE_SEED, 4, 5, rows=[13, 2]),
                          key.body.reshape(30, 1024)[[13, 2]])
    # b_ij - a_ij*S is the row's noise plus s_i 2^(32 - (j+1) basebit) at X^0: small, not zero
    e = keygen.rlwe_phase(full.reshape(30, 2, 1024), sk.tlwe_key).view(np.uint32).copy()
    e[:, 0] -= np.repeat(sk.lwe_key.astype(np.uint32), 5) * np.tile(np.uint32(1) << (32 - 4 * (np.arange(5) + 1)).astype(np.uint32), 6)
    assert 0 < np.abs(e.view(np.int32)).max() < 8.58 * 2.0 ** -30 * 2.0 ** 32 + 1
    f = io.BytesIO()
    client.write_packing_key(f, key)
    raw = f.getvalue()
    assert raw[:4] == b"RSK1" and len(raw) == client._RS_HEADER.itemsize + 8 + key.nbytes
    back = client.read_packing_key(io.BytesIO(raw))
    assert (back.name, back.n, back.basebit, back.t, back.mask_seed) == (key.name, key.n, key.basebit, key.t, key.mask_seed)
    assert np.array_equal(back.body, key.body)
    hs = client._RS_HEADER.itemsize
    bad_digits = raw[:hs] + np.array([9, 4], "<i4").tobytes() + raw[hs + 8:]
    for damaged in (raw[:-4], raw + b"\0\0\0\0", raw[:40], raw[:3], raw[:hs + 20], b"RSP1" + raw[4:], bad_digits):
        with pytest.raises(ValueError):
            client.read_packing_key(io.BytesIO(damaged))
    with pytest.raises(ValueError):
        client.read_rlwe_public_key(io.BytesIO(raw))                         # a packing key is not an RSP1 file


def test_equal_seeds_and_vanishing_default_deviations_are_refused():
    sk = _secret("redsec_small_v2", 4)
    with pytest.raises(ValueError, match="equal"):
        sk.packing_key(mask_seed=MASK_SEED, noise_seed=MASK_SEED)
    with pytest.raises(ValueError, match="equal"):
        keygen.pack_key("redsec_small_v2", sk.lwe_key, sk.tlwe_key, MASK_SEED, MASK_SEED, 4, 5, 0.0)
    a, b = sk.packing_key(), sk.packing_key()                                # fresh seeds by default
    assert a.mask_seed != b.mask_seed and not np.array_equal(a.body, b.body)
    for name in ("redsec_medium", "redsec_large", "redsec_small"):
        big = _secret(name, 2)
        with pytest.raises(ValueError, match="explicit stdev"):
            big.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
        assert big.packing_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED, stdev=2.0 ** -30).body.shape == (2, 5, big.N)
    assert keygen.pack_default("default128") == (4, 4)
    for name in ("redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large"):
        assert keygen.pack_default(name) == (4, 5)
    with pytest.raises(KeyError):
        keygen.pack_default("no_such_set")
    for basebit, t in ((0, 4), (9, 2), (4, 0), (4, 9), (8, 5)):
        with pytest.raises(ValueError):
            keygen.pack_sigma(16, 1024, basebit, t, 1, 0.0)
        with pytest.raises(ValueError):
            sk.packing_key(basebit, t, MASK_SEED, NOISE_SEED)
    # sqrt(n / 24) 2^(-t basebit) at n = 350: 16 bits leave 5.8e-5 of rounding (7e-5 at n = 500), 20 bits 3.6e-6; default-128 with full slots 4.3e-4 at t = 4 (4.7e-4 at t = 5)
    assert 5e-5 < keygen.pack_sigma(350, 1024, 4, 4, 1, 0.0) < 6e-5 < keygen.pack_sigma(500, 1024, 4, 4, 1, 0.0) < 8e-5 and 3e-6 < keygen.pack_sigma(350, 1024, 4, 5, 1, 0.0) < 5e-6
    assert 4.2e-4 < keygen.pack_sigma(630, 1024, 4, 4, 1024, 2.0 ** -25) < 4.4e-4 < 4.6e-4 < keygen.pack_sigma(630, 1024, 4, 5, 1024, 2.0 ** -25) < 4.8e-4
    assert keygen.pack_sigma(630, 1024, 4, 4, 5000, 2.0 ** -25) == keygen.pack_sigma(630, 1024, 4, 4, 1024, 2.0 ** -25)
    assert keygen.pack(np.zeros((0, 5), np.int32), np.zeros((4, 5, 2, 1024), np.int32), 4, 5).shape == (0, 2, 1024)


def test_symbol_and_domains_are_in_the_header_the_library_the_binding_the_recipe_and_the_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_pack_dev\(rs_ctx\* ctx, int32_t\* rlwe, const int32_t\* ct, size_t count,\s+const int32_t\* pack_key, "
                     r"int32_t basebit, int32_t t, void\* stream\);", header)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for d in ("domain 14  packing-key mask    row i t + j   mask seed (public)             a_ij[k] = word k, k < N",
              "domain 15  packing-key noise   row i t + j   owner's noise seed (private)   e_ij[k] = Gaussian k (words 4k .. 4k+3, kg_noise32)"):
        assert d in header and d in (keygen.__doc__ or "") and d in integration, d
    formula = "sigma^2 = n t count_r (2^basebit - 1)(2^(basebit+1) - 1)/6 sigma_k^2  +  (n/2) 2^(-2 t basebit)/12"
    assert formula in header and formula in integration
    L = redsec_amd.load_library()
    assert "rs_pack_dev" in redsec_amd.ABI_SYMBOLS and hasattr(L, "rs_pack_dev")
    for f in ("pack", "upload_packing_key"):
        assert callable(getattr(redsec_amd.Backend, f))
    for f in ("packing_key", "packed_phase", "decrypt_packed_bits", "decrypt_packed_ints"):
        assert callable(getattr(client.SecretKeySet, f))
    assert (keygen.DOMAIN_PACK_MASK, keygen.DOMAIN_PACK_NOISE) == (14, 15)
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_pack", "rs_pack.hip", [])' in build
    assert "rs_pack_dev" in integration and "rs_pack_dev" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "rs_pack_dev" in open(os.path.join(ROOT, "README.md")).read()
    for path in re.findall(r"profiles/r20/[\w./-]*\w", integration + open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_failure_without_a_context_matches_rlwe_extract():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    rc = L.rs_rlwe_extract_dev(None, p, p, 1, None)
    msg = L.rs_last_error()
    assert rc != 0
    assert L.rs_pack_dev(None, p, p, 1, p, 4, 5, None) == rc and L.rs_last_error() == msg
    assert L.rs_pack_dev(None, None, None, 0, None, 0, 0, None) == rc and L.rs_last_error() == msg


def test_new_kernels_hold_zero_scratch_and_no_static_lds():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    main = {n: k for n, k in ks.items() if "11pack_kernel" in n}
    init = {n: k for n, k in ks.items() if "16pack_init_kernel" in n}
    assert len(main) == 1 and len(init) == 1, (sorted(main), sorted(init))
    for k in main.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 64 and k["lds"] == 0, k    # the LDS is dynamic: (9 cpad + 512) words, cpad <= 1024
    for k in init.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 32 and k["lds"] == 0, k


def test_pack_sources_are_integer_only():
    """As rs_audit.*: the sources name no floating type and include neither a transform nor the split-key product."""
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_pack.h", "rs_pack.hip", "rs_ring_sweep.h"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\b(double|float|half|__fp16|_Float16)\b|rs_general\.h|rs_fft\.h|rs_ntt\.h", code), f
