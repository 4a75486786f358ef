"""Re-keying without a GPU (include/redsec_hip.h rs_rekey_dev): under a real seeded key the numpy
restatement moves every phase by exactly the digits' rounding minus the key noise under the digits, the error of noisy keys has the
predicted deviation, the emulated kernel (its own workgroup / chunk / index / wave walk, compiled into the lane emulator) equals
numpy word for word at the kernel's real edges, a key made from an RLWE public key decrypts under the ring key, RSR1 files
round-trip, the seed and deviation rules hold, and the symbol is everywhere it belongs."""
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
MASK_SEED = bytes(range(160, 192))
NOISE_SEED = bytes(range(11, 43))
RAND_SEED = bytes(range(70, 102))
KEY_SEED = bytes(range(9, 41))
OTHER_SEED = bytes(range(90, 122))
_i32p = C.POINTER(C.c_int32)
PAIRS = [(2, 8), (8, 4), (3, 5), (1, 32), (4, 4)]


def _emu():
    L = emu_lib.lib()
    L.rs_emu_rekey.argtypes = [_i32p, C.c_long, C.c_int, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p]
    L.rs_emu_rekey.restype = None
    L.rs_emu_rekey_offset.argtypes = [C.c_int, C.c_int]
    L.rs_emu_rekey_offset.restype = C.c_uint32
    L.rs_emu_rekey_digit.argtypes = [C.c_uint32, C.c_int, C.c_int]
    L.rs_emu_rekey_digit.restype = C.c_uint32
    L.rs_emu_rekey_chunks.argtypes = [C.c_int]
    for f in (L.rs_emu_rekey_span, L.rs_emu_rekey_splits, L.rs_emu_rekey_groups):
        f.argtypes = [C.c_long, C.c_int, C.c_int]
    L.rs_emu_rekey_groups.restype = C.c_long
    return L


def _tiles():
    L = _emu()
    return L.rs_emu_rekey_tile(), L.rs_emu_rekey_words(), L.rs_emu_rekey_seg()


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _secret(name, n, seed=KEY_SEED):
    lwe, tlwe = keygen.secret_keys(name, seed, n)
    return client.SecretKeySet.from_secret(name, lwe, tlwe)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _rounding(sk, ct, basebit, t):
    """sum_i s_i (a_i - the digits' value of a_i), computed from the mask words alone."""
    a = ct[:, :sk.n].astype(np.int64) & 0xFFFFFFFF
    bits = t * basebit
    off = (1 << (31 - bits)) if bits < 32 else 0
    kept = (((a + off) & 0xFFFFFFFF) >> (32 - bits)) << (32 - bits)
    return (((a - kept) * sk.lwe_key.astype(np.int64)).sum(axis=1) & 0xFFFFFFFF).astype(np.uint32)


@pytest.mark.parametrize("stdev", [2.0 ** -25, 0.0])
@pytest.mark.parametrize("basebit,t", [(4, 5), (2, 8)])
def test_a_real_seeded_key_moves_every_phase_by_exactly_rounding_minus_noise(basebit, t, stdev):
    """phase of out[r] under s' - phase of ct[r] under s = sum_i s_i (a_i - digits' value of a_i) - sum_ij d_ij e_ij, word for word,
    the e_ij from keygen.ct_noise; with stdev = 0 the second sum vanishes. Across sets: redsec_small_v2 (n = 16) to default-128
    (n = 24)."""
    src, dst = _secret("redsec_small_v2", 16), _secret("default128", 24, OTHER_SEED)
    key = src.rekey_to(dst, basebit, t, MASK_SEED, NOISE_SEED, stdev=stdev)
    assert (key.form, key.src_name, key.dst_name, key.n_src, key.n_dst) == ("seeded", "redsec_small_v2", "default128", 16, 24)
    full = key.expand()
    assert full.shape == (16, t, 25) and full.dtype == np.int32
    # every row decrypts under s' to its message plus its noise word
    e = keygen.ct_noise(NOISE_SEED, 0, 16 * t, stdev)
    assert np.array_equal(_u32(dst.phase(full.reshape(-1, 25))), _u32(keygen.rekey_messages(src.lwe_key, basebit, t)) + _u32(e))
    assert bool(e.any()) == (stdev > 0)
    mu = _words(np.random.default_rng(basebit), 77)
    ct = src.encrypt_torus(mu, 2.0 ** -20, 5)
    out = keygen.rekey(ct, full, basebit, t)
    assert out.shape == (77, 25) and out.dtype == np.int32
    d = keygen.pack_digits(ct[:, :16], basebit, t).reshape(77, 16 * t).astype(np.uint64)
    noise = ((d * _u32(e).astype(np.uint64)[None, :]).sum(axis=1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    want = _u32(src.phase(ct)) + _rounding(src, ct, basebit, t) - noise
    assert np.array_equal(_u32(dst.phase(out)), want)
    if stdev == 0:
        assert not noise.any()
        # the rounding is at most n_src 2^(31 - t basebit), half a unit of the last digit per key bit
        assert np.abs((want - _u32(src.phase(ct))).view(np.int32)).max() <= 16 << (31 - t * basebit)


NOISY_SHAPE = dict(n_src=8, n_dst=16, basebit=4, t=5, samples=256, keys=256, stdev=2.0 ** -25)


def test_noisy_keys_have_the_predicted_rekeying_error():
    """256 independent keys at n_src = 8, n_dst = 16, (4, 5), 256 samples each, sigma_row = 2^-25 (NOISY_SHAPE): the pooled root mean
    square of the error is within 15 % of rekey_sigma and the largest error below 8 sigma. The digits are unsigned, so most of the
    variance is the digits' mean times the sum of a key's noise words, fixed by the key: single keys scatter widely and the pooled
    value needs many keys (a numpy model of sum d e over six seeds gave ratios 0.94 .. 1.02 and largest errors 3.7 .. 4.6 sigma at
    256 keys; 48 keys scatter to 0.83). Every +-1/8 message decrypts."""
    s = NOISY_SHAPE
    sigma = keygen.rekey_sigma(s["n_src"], s["basebit"], s["t"], s["stdev"])
    errs, per_key = [], []
    for k in range(s["keys"]):
        seeds = [bytes((b + 41 * k + 13 * q) & 0xFF for b in range(32)) for q in range(4)]
        src, dst = _secret("default128", s["n_src"], seeds[0]), _secret("default128", s["n_dst"], seeds[1])
        key = src.rekey_to(dst, s["basebit"], s["t"], seeds[2], seeds[3], s["stdev"])
        bits = np.random.default_rng(k).integers(0, 2, s["samples"])
        ct = src.encrypt_bits(bits, seed=100 + k)
        out = keygen.rekey(ct, key.expand(), s["basebit"], s["t"])
        assert np.array_equal(dst.decrypt_bits(out), bits)
        e = (_u32(dst.phase(out)) - _u32(src.phase(ct))).view(np.int32) / 2.0 ** 32
        errs.append(e)
        per_key.append(np.sqrt(np.mean(e * e)) / sigma)
    err = np.concatenate(errs)
    rms, worst, mean = np.sqrt(np.mean(err * err)), np.abs(err).max(), err.mean()
    print("rekey_sigma %.4g, rms %.4g (ratio %.3f), single keys %.3f .. %.3f (std %.3f), largest %.2f sigma, mean %.3f sigma"
          % (sigma, rms, rms / sigma, min(per_key), max(per_key), np.std(per_key), worst / sigma, mean / sigma))
    assert err.size == s["keys"] * s["samples"]
    assert abs(rms / sigma - 1.0) < 0.15
    assert worst < 8 * sigma


def _check_emulator(B, n_src, n_dst, basebit, t, span=0):
    L = _emu()
    rng = np.random.default_rng(B + 3 * n_src + 7 * n_dst + 100 * basebit + t)
    key, ct = _words(rng, n_src, t, n_dst + 1), _words(rng, B, n_src + 1)
    guard = np.full((B + 2, n_dst + 1), 0x5A5A5A5A, np.int32)
    got = guard[1:B + 1]
    L.rs_emu_rekey(ct.ctypes.data_as(_i32p), B, n_src, key.ctypes.data_as(_i32p), n_dst, basebit, t, span, got.ctypes.data_as(_i32p))
    want = keygen.rekey(ct, key, basebit, t)
    assert np.array_equal(got, want), (B, n_src, n_dst, basebit, t, span, np.argwhere(got != want)[:4].tolist())
    assert (guard[0] == 0x5A5A5A5A).all() and (guard[B + 1] == 0x5A5A5A5A).all()
    return want


def test_emulated_kernel_equals_numpy_at_every_ciphertext_tile_edge():
    """B = 1, T - 1, T, T + 1, 2 T + 5 with T the exported ciphertext tile (128: four waves of 32), and the edges of a wave's 32
    and of its groups of 8, at n_src = 9 (two chunks, the second of one index), n_dst = 64 (two word tiles, the second of one word)."""
    T, _, _ = _tiles()
    wave = _emu().rs_emu_rekey_wave_cts()
    for B in (1, T - 1, T, T + 1, 2 * T + 5, 7, 8, 9, wave - 1, wave, wave + 1):
        _check_emulator(B, 9, 64, 4, 5)


def test_emulated_kernel_equals_numpy_at_every_word_tile_and_index_chunk_edge():
    """n_dst + 1 one short of, exactly and one past the word tile (and two tiles and one); n_src one short of, exactly and one past
    the index chunk; every index split the launcher can choose: the kernel's own plan (one chunk per workgroup at these sizes), all
    chunks in one workgroup, and two chunks per workgroup with a ragged last split."""
    T, words, seg = _tiles()
    for W in (words - 1, words, words + 1, 2 * words + 1, 2):
        _check_emulator(T + 1, 5, W - 1, 4, 5)
    for n_src in (1, seg - 1, seg, seg + 1, 2 * seg + 3):
        _check_emulator(5, n_src, 16, 2, 8)
    for span in (0, 1, 2, 5):
        _check_emulator(33, 4 * seg + 5, 37, 4, 5, span)


@pytest.mark.parametrize("basebit,t", PAIRS)
def test_emulated_kernel_equals_numpy_for_every_digit_shape(basebit, t):
    """(2, 8) and (8, 4): the narrowest and widest digits of 16 and 32 bits; (3, 5): a basebit that does not divide 32 and an odd t
    (the lone last digit); (1, 32) and (8, 4): all 32 bits, offset 0; (4, 4): 16 bits."""
    _check_emulator(65, 16, 37, basebit, t)


def test_emulated_helpers_equal_numpy_and_name_the_launch_plan():
    L = _emu()
    a = _words(np.random.default_rng(5), 64)
    for basebit, t in PAIRS:
        off = L.rs_emu_rekey_offset(basebit, t)
        assert off == ((1 << (31 - t * basebit)) if t * basebit < 32 else 0)
        want = keygen.pack_digits(a, basebit, t)
        got = np.array([[L.rs_emu_rekey_digit((int(x) + off) & 0xFFFFFFFF, basebit, j) for j in range(t)] for x in _u32(a)], np.uint32)
        assert np.array_equal(got, want), (basebit, t)
    assert _tiles() == (128, 64, 8) and L.rs_emu_rekey_wave_cts() == 32 and L.rs_emu_rekey_fill() == 2048
    assert [L.rs_emu_rekey_chunks(n) for n in (1, 8, 9, 37, 350, 630)] == [1, 1, 2, 5, 44, 79]
    # default-128 to default-128: ten samples split every chunk apart, 1,024 take four chunks a workgroup, 65,536 fill the device
    # with their tiles alone (512 x 10 workgroups) and walk all 79 chunks in one workgroup
    plan = lambda B, n_src, n_dst: (L.rs_emu_rekey_span(B, n_src, n_dst), L.rs_emu_rekey_splits(B, n_src, n_dst), L.rs_emu_rekey_groups(B, n_src, n_dst))
    assert plan(10, 630, 630) == (1, 79, 790)
    assert plan(1024, 630, 630) == (4, 20, 8 * 10 * 20)
    assert plan(65536, 630, 630) == (79, 1, 512 * 10)
    assert plan(65536, 350, 1024) == (44, 1, 512 * 17)
    assert plan(1, 1, 1) == (1, 1, 1)


def test_messages_sigma_and_defaults():
    s = np.array([1, 0, 1], np.int32)
    assert keygen.rekey_messages(s, 4, 2).view(np.uint32).tolist() == [1 << 28, 1 << 24, 0, 0, 1 << 28, 1 << 24]
    assert keygen.rekey_messages(s, 1, 32).view(np.uint32)[[0, 31]].tolist() == [1 << 31, 1]
    # the issue's arithmetic: (2, 8) to default-128 at its ks_stdev from n_src = 630; (4, 5) to redsec_small_v2 with seeded rows at
    # 2^-25 and with RLWE rows at 2^-30 sqrt(1025)
    assert keygen.rekey_default("default128") == (2, 8)
    assert 4.0e-3 < keygen.rekey_sigma(630, 2, 8, 2.0 ** -15) < 4.2e-3
    assert 8 * keygen.rekey_sigma(630, 2, 8, 2.0 ** -15) < 1 / 16
    assert keygen.rekey_default("redsec_small_v2") == (4, 5) == keygen.rekey_default("redsec_small")
    assert 1.0e-5 < keygen.rekey_sigma(350, 4, 5, 2.0 ** -25) < 1.2e-5
    assert 1.0e-5 < keygen.rekey_sigma(350, 4, 5, 2.0 ** -30 * np.sqrt(1025.0)) < 1.2e-5
    # a REDsec destination from a source of its own n: 8 sigma stays below the half step of 1/4096-scale values, at the set's own
    # row deviation where that exists and at 2^-31 where it truncates to zero
    for name in ("redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large"):
        n, row = client.PARAM_SETS[name][0], max(client.PARAM_SETS[name][7], 2.0 ** -31)
        assert 8 * keygen.rekey_sigma(n, *keygen.rekey_default(name), row) < 1 / 8192, name
    assert keygen.rekey_default("redsec_large") == (4, 6)
    # default-128 (n_src = 630) to redsec_small_v2 leaves no margin for 1/4096-scale values at (4, 5); bits pass easily
    assert 1 / 8192 < 8 * keygen.rekey_sigma(630, 4, 5, 2.0 ** -25) < 1 / 16
    with pytest.raises(KeyError):
        keygen.rekey_default("no_such_set")
    for basebit, t in ((0, 4), (9, 2), (4, 0), (4, 9), (8, 5)):
        with pytest.raises(ValueError):
            keygen.rekey_sigma(16, basebit, t, 0.0)
        with pytest.raises(ValueError):
            keygen.rekey_messages(s, basebit, t)
    assert keygen.rekey(np.zeros((0, 4), np.int32), np.zeros((3, 5, 9), np.int32), 4, 5).shape == (0, 9)


def test_a_key_made_from_an_rlwe_public_key_decrypts_under_the_ring_key():
    """rekey_for needs only the recipient's RlwePublicKey: its rows, expanded through keygen.rlwe_extract, decrypt under the ring key
    read as an LWE key to rekey_messages within 8 stdev sqrt(N + 1) per row, and samples re-keyed with it decrypt with ring=True."""
    src, dst = _secret("default128", 12), _secret("redsec_small_v2", 9, OTHER_SEED)
    pk = dst.rlwe_public_key(MASK_SEED, NOISE_SEED)
    key = src.rekey_for(pk, rand_seed=RAND_SEED)
    N, stdev = 1024, client.PARAM_SETS["redsec_small_v2"][8]
    assert (key.form, key.n_src, key.n_dst, key.basebit, key.t) == ("rlwe", 12, N, 4, 5)
    assert key.rlwe.shape == (1, 2, N) and key.nbytes == 8 * N
    full = key.expand()
    assert full.shape == (12, 5, N + 1)
    raw = keygen.rlwe_extract(key.rlwe, 60)                                  # slot r carries row r, negated when r is odd
    assert np.array_equal(full.reshape(60, N + 1)[0::2], raw[0::2])
    assert np.array_equal(_u32(full.reshape(60, N + 1)[1::2]), np.uint32(0) - _u32(raw[1::2]))
    assert np.array_equal(keygen.rekey_alternate(keygen.rekey_alternate(raw)), raw)
    e = (_u32(dst.phase(full.reshape(60, N + 1), ring=True)) - _u32(keygen.rekey_messages(src.lwe_key, 4, 5))).view(np.int32)
    assert 0 < np.abs(e).max() < 8 * stdev * np.sqrt(N + 1.0) * 2.0 ** 32
    v = np.random.default_rng(3).integers(-2048, 2048, 40)
    ct = src.encrypt_torus(v * (1 << 20), 2.0 ** -25, 6)
    out = keygen.rekey(ct, full, 4, 5)
    sigma = keygen.rekey_sigma(12, 4, 5, stdev * np.sqrt(N + 1.0))
    err = (_u32(dst.phase(out, ring=True)) - _u32(src.phase(ct))).view(np.int32)
    assert np.abs(err).max() < 8 * sigma * 2.0 ** 32
    assert np.array_equal(dst.decrypt_ints(out, ring=True), v)
    # 61 source indices need 305 rows of 1,024: one ciphertext; 205 need 1,025: two
    assert _secret("default128", 205).rekey_for(pk, rand_seed=RAND_SEED).rlwe.shape == (2, 2, N)


def test_rlwe_form_keys_at_full_size_have_no_offset_fixed_by_the_key():
    """redsec_small_v2 to a redsec_small_v2 ring key at n_src = 350, (4, 5), four independent key pairs, 64 samples each: every error
    is below 8 rekey_sigma with sigma_row = stdev sqrt(N + 1). The 1,750 rows sit in two ciphertexts and share their selector and
    noise polynomials; without the alternating signs of keygen.rekey_alternate the unsigned digits add the common part of their
    noise into an offset fixed by the key (measured over eight key pairs: mean errors of -38.9 .. 18.1 sigma, six of eight beyond
    4 sigma; with the signs: means within 0.8 sigma, largest error 2.6 sigma, pooled root mean square 0.73 sigma over twelve)."""
    name, N = "redsec_small_v2", 1024
    stdev = client.PARAM_SETS[name][8]
    sigma = keygen.rekey_sigma(350, 4, 5, stdev * np.sqrt(N + 1.0))
    worst = []
    for k in range(4):
        seeds = [bytes((b + 41 * k + 13 * q) & 0xFF for b in range(32)) for q in range(5)]
        src, dst = _secret(name, None, seeds[0]), _secret(name, None, seeds[1])
        key = src.rekey_for(dst.rlwe_public_key(seeds[2], seeds[3]), rand_seed=seeds[4])
        assert key.rlwe.shape == (2, 2, N)
        v = np.random.default_rng(k).integers(-2048, 2048, 64)
        ct = src.encrypt_torus(v * (1 << 20), 2.0 ** -25, 5)
        out = keygen.rekey(ct, key.expand(), 4, 5)
        err = (_u32(dst.phase(out, ring=True)) - _u32(src.phase(ct))).view(np.int32) / 2.0 ** 32
        worst.append(np.abs(err).max() / sigma)
        assert np.array_equal(dst.decrypt_ints(out, ring=True), v)
    print("rlwe form, n_src = 350, (4, 5): largest errors %s sigma (rekey_sigma %.4g)" % (", ".join("%.2f" % w for w in worst), sigma))
    assert max(worst) < 8


def test_rsr1_files_round_trip_and_reject_damage():
    src, dst = _secret("redsec_small_v2", 6), _secret("default128", 7, OTHER_SEED)
    seeded = src.rekey_to(dst, mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    assert (seeded.basebit, seeded.t) == (2, 8) and seeded.body.shape == (48,) and seeded.nbytes == 32 + 4 * 48
    assert np.array_equal(seeded.body, keygen.encrypt_seeded(dst.lwe_key, keygen.rekey_messages(src.lwe_key, 2, 8), MASK_SEED, NOISE_SEED,
                                                             0, client.PARAM_SETS["default128"][7]))
    rlwe = src.rekey_for(_secret("redsec_small_v2", 3, OTHER_SEED).rlwe_public_key(MASK_SEED, NOISE_SEED), rand_seed=RAND_SEED)
    hs = client._RS_HEADER.itemsize
    for key in (seeded, rlwe):
        f = io.BytesIO()
        client.write_rekey_key(f, key)
        raw = f.getvalue()
        assert raw[:4] == b"RSR1" and raw[hs:hs + 4] == b"RSR1" and len(raw) == 2 * hs + 12 + key.nbytes
        back = client.read_rekey_key(io.BytesIO(raw))
        assert (back.form, back.src_name, back.dst_name, back.n_src, back.n_dst, back.basebit, back.t) == \
               (key.form, key.src_name, key.dst_name, key.n_src, key.n_dst, key.basebit, key.t)
        assert back.mask_seed == key.mask_seed and np.array_equal(back.expand(), key.expand())
        digits = lambda *v: raw[:2 * hs] + np.array(v, "<i4").tobytes() + raw[2 * hs + 12:]
        other_form = 1 if key.form == "seeded" else 0
        for damaged in (raw[:-4], raw + b"\0\0\0\0", raw[:40], raw[:3], raw[:2 * hs + 8], b"RSK1" + raw[4:],
                        raw[:hs] + b"RSK1" + raw[hs + 4:], digits(9, 4, 0), digits(4, 9, 0), digits(key.basebit, key.t, 2),
                        digits(key.basebit, key.t, other_form)):
            with pytest.raises(ValueError):
                client.read_rekey_key(io.BytesIO(damaged))
        with pytest.raises(ValueError):
            client.read_packing_key(io.BytesIO(raw))                         # a re-keying key is not an RSK1 file


def test_equal_seeds_and_vanishing_default_deviations_are_refused():
    src, dst = _secret("redsec_small_v2", 4), _secret("redsec_small_v2", 5, OTHER_SEED)
    with pytest.raises(ValueError, match="equal"):
        src.rekey_to(dst, mask_seed=MASK_SEED, noise_seed=MASK_SEED)
    pk = dst.rlwe_public_key(MASK_SEED, NOISE_SEED)
    with pytest.raises(ValueError, match="equal"):
        src.rekey_for(pk, rand_seed=MASK_SEED)
    a, b = src.rekey_to(dst), src.rekey_to(dst)                              # fresh seeds by default
    assert a.mask_seed != b.mask_seed and not np.array_equal(a.body, b.body)
    assert not np.array_equal(src.rekey_for(pk).rlwe, src.rekey_for(pk).rlwe)
    for name in ("redsec_medium", "redsec_large"):
        big = _secret(name, 2, OTHER_SEED)
        with pytest.raises(ValueError, match="explicit stdev"):
            src.rekey_to(big, mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
        assert src.rekey_to(big, mask_seed=MASK_SEED, noise_seed=NOISE_SEED, stdev=2.0 ** -31).body.shape == (4 * 6,)
        with pytest.raises(ValueError, match="explicit stdev"):
            src.rekey_for(client.RlwePublicKey(name, MASK_SEED, np.zeros(big.N, np.int32)), rand_seed=RAND_SEED)
    for basebit, t in ((0, 4), (9, 2), (4, 0), (4, 9), (8, 5)):
        with pytest.raises(ValueError):
            src.rekey_to(dst, basebit, t, MASK_SEED, NOISE_SEED)
        with pytest.raises(ValueError):
            src.rekey_for(pk, basebit, t, RAND_SEED)


def test_symbol_prototype_and_formula_are_in_the_header_the_library_the_binding_the_recipe_and_the_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_rekey_dev\(rs_ctx\* ctx, int32_t\* out, const int32_t\* ct, size_t B, int32_t n_src,\s+"
                     r"const int32_t\* rekey_key, int32_t n_dst, int32_t basebit, int32_t t, void\* stream\);", header)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    formula = "sigma^2 = n_src t (2^basebit - 1)(2^(basebit+1) - 1)/6 sigma_row^2  +  (n_src/2) 2^(-2 t basebit)/12"
    assert formula in header and formula in integration and formula in (keygen.rekey_sigma.__doc__ or "")
    for line in ("out[r]   = (0, b_r) - sum_{i,j} d_ij(r) K[i][j]", "abar     = a + off,  off = 2^(31 - t basebit)  (0 when t basebit = 32)"):
        assert line in header and line in integration, line
    L = redsec_amd.load_library()
    assert "rs_rekey_dev" in redsec_amd.ABI_SYMBOLS and hasattr(L, "rs_rekey_dev")
    for f in ("rekey", "upload_rekey_key"):
        assert callable(getattr(redsec_amd.Backend, f))
    for f in ("rekey_to", "rekey_for", "phase", "decrypt_bits", "decrypt_ints"):
        assert callable(getattr(client.SecretKeySet, f))
    for f in ("rekey", "rekey_messages", "rekey_sigma", "rekey_default"):
        assert callable(getattr(keygen, f))
    for f in ("RekeyKey", "write_rekey_key", "read_rekey_key"):
        assert hasattr(client, f)
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_rekey", "rs_rekey.hip", [])' in build
    assert "## 21." in integration and "rs_rekey_dev" in integration and "rs_rekey_dev" in design
    assert "rs_rekey_dev" in open(os.path.join(ROOT, "README.md")).read()
    named = re.findall(r"profiles/r24/[\w./-]*\w", integration + design + open(os.path.join(ROOT, "profiles", "r24", "README.md")).read())
    assert named
    for path in named:
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_failure_without_a_context_matches_pack():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    rc = L.rs_pack_dev(None, p, p, 1, p, 4, 5, None)
    msg = L.rs_last_error()
    assert rc != 0
    assert L.rs_rekey_dev(None, p, p, 1, 1, p, 1, 4, 5, None) == rc and L.rs_last_error() == msg
    assert L.rs_rekey_dev(None, None, None, 0, 0, None, 0, 0, 0, None) == rc and L.rs_last_error() == msg


def test_new_kernels_hold_zero_scratch_and_no_static_lds():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    main = {n: k for n, k in ks.items() if "12rekey_kernel" in n}
    init = {n: k for n, k in ks.items() if "17rekey_init_kernel" in n}
    assert len(main) == 1 and len(init) == 1, (sorted(main), sorted(init))
    for k in main.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 72 and k["lds"] == 0, k    # the LDS is dynamic: (1,024 + 64 t) words, t <= 32
    for k in init.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 32 and k["lds"] == 0, k


def test_rekey_sources_are_integer_only():
    """As rs_pack.* and rs_audit.*: the sources name no floating type and include neither a transform nor the split-key product."""
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_rekey.h", "rs_rekey.hip"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\b(double|float|half|__fp16|_Float16)\b|rs_general\.h|rs_fft\.h|rs_ntt\.h", code), f
