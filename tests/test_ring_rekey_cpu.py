"""Ring re-keying without a GPU (rs_ring_rekey_dev): the exact identity of a noise-free key, the error of
noisy keys of both forms against ring_rekey_sigma (and what unsigned digits would do to the public-key form), the lane emulator of
the kernels against the numpy restatement, files, refusals, symbols and kernel budgets."""
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

MASK_SEED = bytes(range(150, 182))
NOISE_SEED = bytes(range(31, 63))
RAND_SEED = bytes(range(200, 232))
KEY_SEED = bytes(range(9, 41))
OTHER_SEED = bytes(range(90, 122))
SHAPES = [(1, 1), (8, 3), (4, 5), (2, 8), (5, 6), (1, 31)]


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _secret(name, seed=KEY_SEED):
    return client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, seed))


def _seeds(k):
    return [bytes((b + 41 * k + 13 * q) & 0xFF for b in range(32)) for q in range(6)]


def _emu():
    return emu_lib.lib()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _extreme(rng, R, N, basebit, t):
    """Random ciphertexts whose first mask coefficients are the extreme words and 2^32 - off, which wraps abar to 0."""
    rl = _words(rng, R, 2, N)
    off = 1 << (31 - t * basebit)
    ext = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, (1 << 32) - off, (1 << 32) - off - 1, off], np.uint64).astype(np.uint32)
    rl[:, 0, :ext.size] = ext.view(np.int32)
    rl[0, 0, -ext.size:] = ext.view(np.int32)
    return rl


@pytest.mark.parametrize("basebit,t", SHAPES)
def test_a_noise_free_key_moves_the_phase_by_the_rounding_alone(basebit, t):
    """phase_S'(out) - phase_S(in) = -((off - rho)(X) S) word for word, rho_k = abar_k mod 2^(32 - t basebit)."""
    N = 1024
    src, dst = _secret("redsec_small_v2"), _secret("redsec_small_v2", OTHER_SEED)
    key = src.ring_rekey_to(dst, basebit, t, MASK_SEED, NOISE_SEED, stdev=0.0)
    assert key.form == "seeded" and key.nbytes == 32 + 4 * N * (t + 1) and key.expand().shape == (t + 1, 2, N)
    rl = _extreme(np.random.default_rng(10 * basebit + t), 2, N, basebit, t)
    out = keygen.ring_rekey(rl, key.expand(), basebit, t)
    off = 1 << (31 - t * basebit)
    abar = (_u32(rl[:, 0]).astype(np.int64) + off) & 0xFFFFFFFF
    assert (abar[:, 4] == 0).all()                                           # 2^32 - off wrapped
    rho = abar % (1 << (32 - t * basebit))
    want = np.uint32(0) - keygen._times_binary(((off - rho) & 0xFFFFFFFF).astype(np.uint32), src.tlwe_key)
    got = _u32(keygen.rlwe_phase(out, dst.tlwe_key)) - _u32(keygen.rlwe_phase(rl, src.tlwe_key))
    assert np.array_equal(got, want)


def test_the_digits_are_odd_and_rebuild_the_rounded_word_with_the_constant():
    rng = np.random.default_rng(4)
    for basebit, t in SHAPES:
        a = _extreme(rng, 1, 1024, basebit, t)[0, 0]
        d = keygen.ring_rekey_digits(a, basebit, t)
        B1 = (1 << basebit) - 1
        assert d.shape == (t, 1024) and (d & 1).all() and np.abs(d).max() <= B1
        h = np.array([1 << (31 - (j + 1) * basebit) for j in range(t)], np.int64)
        abar = (_u32(a).astype(np.int64) + (1 << (31 - t * basebit))) & 0xFFFFFFFF
        top = abar >> (32 - t * basebit) << (32 - t * basebit)
        assert np.array_equal(((d * h[:, None]).sum(0) + B1 * h.sum()) & 0xFFFFFFFF, top)
    mu = keygen.ring_rekey_messages(np.array([1, 0, 1, 1], np.int32), 4, 2)
    c0 = 15 * ((1 << 27) + (1 << 23))
    assert mu.shape == (3, 4) and np.array_equal(mu[0], [1 << 27, 0, 1 << 27, 1 << 27])
    assert np.array_equal(_u32(mu[2]), (np.array([-1, -1, 1, 3], np.int64) * c0 & 0xFFFFFFFF).astype(np.uint32))


def _errors(form, basebit, t, stdev, pairs=8):
    """Re-keying errors per coefficient as reals, [pairs][2][N], of fresh key pairs and two ciphertexts each at N = 1024."""
    name, N = "redsec_small_v2", 1024
    errs = []
    for k in range(pairs):
        s = _seeds(k + (7 if form == "rlwe" else 0) + 100 * basebit)
        src, dst = _secret(name, s[0]), _secret(name, s[1])
        if form == "seeded":
            key = src.ring_rekey_to(dst, basebit, t, s[2], s[3], stdev=stdev)
        else:
            key = src.ring_rekey_for(dst.rlwe_public_key(s[2], s[3], stdev=stdev), basebit, t, rand_seed=s[4], stdev=stdev)
        rl = _words(np.random.default_rng(k), 2, 2, N)
        out = keygen.ring_rekey(rl, key.expand(), basebit, t)
        errs.append((_u32(keygen.rlwe_phase(out, dst.tlwe_key)) - _u32(keygen.rlwe_phase(rl, src.tlwe_key))).view(np.int32) / 2.0 ** 32)
    return np.array(errs)


@pytest.mark.parametrize("form", ["seeded", "rlwe"])
@pytest.mark.parametrize("basebit,t", [(4, 5), (2, 8)])
@pytest.mark.parametrize("log_alpha", [-25, -30])
def test_noisy_keys_meet_the_formula(form, basebit, t, log_alpha):
    """Eight key pairs x two ciphertexts, N = 1024: the rms of the error lies within 25 % of ring_rekey_sigma (the band of
    tests/test_rlwe_pubkey_cpu.py) and every error below 8 sigma."""
    stdev = 2.0 ** log_alpha
    sigma = keygen.ring_rekey_sigma(1024, basebit, t, stdev if form == "seeded" else stdev * np.sqrt(1025.0))
    e = _errors(form, basebit, t, stdev)
    rms = float(np.sqrt(np.mean(e * e)))
    print("%s (%d, %d) alpha 2^%d: rms / formula %.3f, largest %.2f sigma" % (form, basebit, t, log_alpha, rms / sigma, np.abs(e).max() / sigma))
    assert 0.75 < rms / sigma < 1.25
    assert np.abs(e).max() < 8 * sigma


def test_unsigned_digits_on_the_public_key_form_exceed_five_times_the_formula():
    """The finding behind the digit convention: rows made from one RLWE public key share its noise, and digit polynomials with a
    mean add the common part up along the coefficients. The convention of rs_pack_dev / rs_rekey_dev restated: unsigned digits,
    rows that encrypt 2^(32-(j+1) basebit) S (twice the message rows), no constant row. Eight key pairs x two ciphertexts, (4, 5),
    alpha = 2^-25: 20 times the formula pooled, no single key below 7."""
    name, N, basebit, t, stdev = "redsec_small_v2", 1024, 4, 5, 2.0 ** -25
    sigma = keygen.ring_rekey_sigma(N, basebit, t, stdev * np.sqrt(N + 1.0))
    errs = []
    for k in range(8):
        s = _seeds(k + 7 + 100 * basebit)
        src, dst = _secret(name, s[0]), _secret(name, s[1])
        mu = (_u32(keygen.ring_rekey_messages(src.tlwe_key, basebit, t)[:t]) * np.uint32(2)).view(np.int32)
        rows = keygen.rlwe_pk_encrypt(dst.rlwe_public_key(s[2], s[3], stdev=stdev).expand(), mu.ravel(), s[4], 0, stdev=stdev)
        key = np.concatenate([rows, np.zeros((1, 2, N), np.int32)])
        rl = _words(np.random.default_rng(k), 2, 2, N)
        out = keygen.ring_rekey(rl, key, basebit, t, unsigned=True)
        errs.append((_u32(keygen.rlwe_phase(out, dst.tlwe_key)) - _u32(keygen.rlwe_phase(rl, src.tlwe_key))).view(np.int32) / 2.0 ** 32)
    e = np.array(errs)
    print("unsigned digits, rlwe rows: rms / formula %.1f" % (np.sqrt(np.mean(e * e)) / sigma))
    assert np.sqrt(np.mean(e * e)) > 5 * sigma


@pytest.mark.parametrize("N,basebit,t,R", [(1024, 4, 5, 3), (1024, 1, 31, 1), (1024, 8, 3, 1), (1024, 5, 6, 1), (1024, 1, 1, 2),
                                           (2048, 2, 8, 2), (2048, 4, 5, 1)])
def test_the_emulated_ring_rekey_kernels_equal_numpy(N, basebit, t, R):
    """Every tile, both source blocks of N = 2048, every digit, every ciphertext: rs_emu_ring_rekey walks the kernel's workgroups."""
    E = _emu()
    E.rs_emu_ring_rekey_groups.restype = C.c_long
    assert E.rs_emu_ring_rekey_groups(C.c_long(R), N, t) == R * 2 * (N // 512) * (N // 1024) * t
    assert E.rs_emu_ring_rekey_tile() == 512 and E.rs_emu_ring_rekey_slots() == 1024
    rng = np.random.default_rng(N + 10 * basebit + t)
    rl, key = _extreme(rng, R, N, basebit, t), _words(rng, t + 1, 2, N)
    out = np.full((R + 1, 2, N), 0x5A5A5A5A, np.int32)
    E.rs_emu_ring_rekey(_p(rl), C.c_long(R), N, _p(key), basebit, t, _p(out))
    assert np.array_equal(out[:R], keygen.ring_rekey(rl, key, basebit, t)) and (out[R] == 0x5A5A5A5A).all()
    E.rs_emu_ring_rekey_offset.restype = E.rs_emu_ring_rekey_digit.restype = C.c_uint32
    assert E.rs_emu_ring_rekey_offset(basebit, t) == 1 << (31 - t * basebit)
    d = keygen.ring_rekey_digits(rl[0, 0, :8], basebit, t)
    for j in range(t):
        for k in range(8):
            abar = (int(_u32(rl)[0, 0, k]) + (1 << (31 - t * basebit))) & 0xFFFFFFFF
            assert E.rs_emu_ring_rekey_digit(C.c_uint32(abar), basebit, j) == int(d[j, k]) & 0xFFFFFFFF
    # every window stays inside ext = (-p, p)
    for k0 in range(0, N, 512):
        for c0 in range(0, N, 1024):
            wb = E.rs_emu_ring_rekey_window_base(N, k0, c0)
            assert 0 <= wb and wb + 1024 + 512 <= 2 * N


def test_key_files_round_trip_and_reject_damage():
    src, dst = _secret("redsec_small_v2"), _secret("redsec_small", OTHER_SEED)
    keys = [src.ring_rekey_to(dst, 4, 5, MASK_SEED, NOISE_SEED, stdev=2.0 ** -30),
            src.ring_rekey_for(dst.rlwe_public_key(MASK_SEED, NOISE_SEED, stdev=2.0 ** -30), 2, 3, rand_seed=RAND_SEED, stdev=2.0 ** -30)]
    hs = client._RS_HEADER.itemsize
    for key in keys:
        buf = io.BytesIO()
        client.write_ring_rekey_key(buf, key)
        raw = buf.getvalue()
        assert len(raw) == 2 * hs + 12 + key.nbytes
        back = client.read_ring_rekey_key(io.BytesIO(raw))
        assert (back.form, back.src_name, back.dst_name, back.basebit, back.t, back.N) == \
               (key.form, "redsec_small_v2", "redsec_small", key.basebit, key.t, 1024)
        assert back.mask_seed == key.mask_seed and np.array_equal(back.expand(), key.expand())
        digits = lambda *v: raw[:2 * hs] + np.array(v, "<i4").tobytes() + raw[2 * hs + 12:]
        other_form = 1 if key.form == "seeded" else 0
        medium = client._rs_header("RSX1", "redsec_medium", 3072)
        for damaged in (raw[:-4], raw + b"\0\0\0\0", raw[:40], raw[:3], raw[:2 * hs + 8], b"RSR1" + raw[4:],
                        raw[:hs] + b"RSK1" + raw[hs + 4:], digits(9, 3, 0), digits(4, 8, 0), digits(key.basebit, key.t, 2),
                        digits(key.basebit, key.t, other_form), digits(key.basebit, key.t + 1, 0 if key.form == "seeded" else 1),
                        raw[:hs] + medium + raw[2 * hs:]):
            with pytest.raises(ValueError):
                client.read_ring_rekey_key(io.BytesIO(damaged))
        with pytest.raises(ValueError):
            client.read_rekey_key(io.BytesIO(raw))                           # a ring re-keying key is not an RSR1 file
    assert client.RS_MAGIC["RSX1"] not in [v for k, v in client.RS_MAGIC.items() if k != "RSX1"]


def test_refusals_and_defaults():
    src, dst = _secret("redsec_small_v2"), _secret("redsec_small_v2", OTHER_SEED)
    with pytest.raises(ValueError, match="equal"):
        src.ring_rekey_to(dst, mask_seed=MASK_SEED, noise_seed=MASK_SEED)
    pk = dst.rlwe_public_key(MASK_SEED, NOISE_SEED)
    with pytest.raises(ValueError, match="equal"):
        src.ring_rekey_for(pk, rand_seed=MASK_SEED)
    a, b = src.ring_rekey_to(dst), src.ring_rekey_to(dst)                    # fresh seeds by default
    assert (a.basebit, a.t) == (4, 5) and a.mask_seed != b.mask_seed and not np.array_equal(a.body, b.body)
    r = src.ring_rekey_for(pk)
    assert (r.basebit, r.t) == keygen.ring_rekey_default("redsec_small_v2", "rlwe") == (2, 12) and r.rlwe.shape == (13, 2, 1024)
    assert not np.array_equal(r.rlwe, src.ring_rekey_for(pk).rlwe)
    with pytest.raises(ValueError, match="rings differ"):                    # crossing between rings is out of scope
        src.ring_rekey_to(_secret("redsec_medium", OTHER_SEED), stdev=2.0 ** -31)
    with pytest.raises(ValueError, match="rings differ"):
        src.ring_rekey_for(client.RlwePublicKey("redsec_large", MASK_SEED, np.zeros(8192, np.int32)), stdev=2.0 ** -31)
    small = _secret("redsec_small", OTHER_SEED)                              # bk_stdev 2^-36 truncates to zero
    with pytest.raises(ValueError, match="explicit stdev"):
        src.ring_rekey_to(small, mask_seed=MASK_SEED, noise_seed=NOISE_SEED)
    with pytest.raises(ValueError, match="explicit stdev"):
        src.ring_rekey_for(client.RlwePublicKey("redsec_small", MASK_SEED, np.zeros(1024, np.int32)), rand_seed=RAND_SEED)
    assert src.ring_rekey_to(small, mask_seed=MASK_SEED, noise_seed=NOISE_SEED, stdev=2.0 ** -31).body.shape == (6, 1024)
    for basebit, t in ((0, 4), (9, 2), (4, 0), (4, 8), (8, 4), (1, 32)):
        with pytest.raises(ValueError):
            src.ring_rekey_to(dst, basebit, t, MASK_SEED, NOISE_SEED)
        with pytest.raises(ValueError):
            src.ring_rekey_for(pk, basebit, t, RAND_SEED)
        with pytest.raises(ValueError):
            keygen.ring_rekey(np.zeros((1, 2, 1024), np.int32), np.zeros((t + 1, 2, 1024), np.int32), basebit, t)
    with pytest.raises(ValueError):
        keygen.ring_rekey_default("default128", "other")


def test_the_defaults_keep_eight_sigma_where_the_documents_say_so():
    """8 ring_rekey_sigma against 1/8 (default-128) or the half step 1/8192 (the networks' sets), rows at the set's bk_stdev or, where
    that truncates to zero, at the smallest deviation 2^-31; redsec_large in the rlwe form is the one listed as out of reach."""
    for name, (n, N, k, l, Bgbit, ks_t, ks_basebit, ks_stdev, bk_stdev) in client.PARAM_SETS.items():
        use = 1 / 8 if name == "default128" else 1 / 8192
        stdev = max(bk_stdev, keygen.MIN_STDEV)
        for form in ("seeded", "rlwe"):
            basebit, t = keygen.ring_rekey_default(name, form)
            sigma = keygen.ring_rekey_sigma(N, basebit, t, stdev if form == "seeded" else stdev * np.sqrt(N + 1.0))
            print("%s %s (%d, %d): sigma %.3g, margin %.1f sigma" % (name, form, basebit, t, sigma, use / sigma))
            assert (8 * sigma <= use) == ((name, form) != ("redsec_large", "rlwe")), (name, form, use / sigma)
    # no shape at all reaches it there
    best = max((1 / 8192) / keygen.ring_rekey_sigma(8192, b, t, 2.0 ** -31 * np.sqrt(8193.0)) for b in range(1, 9) for t in range(1, 32) if b * t <= 31)
    assert best < 8


def test_symbols_prototypes_and_formula_are_in_the_header_the_library_the_binding_the_recipe_and_the_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_ring_rekey_dev\(rs_ctx\* ctx, int32_t\* out, const int32_t\* rlwe, size_t R,\s+"
                     r"const int32_t\* ring_key, int32_t basebit, int32_t t, void\* stream\);", header)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    formula = "sigma^2 = (t N (4^basebit - 1)/3 + 1) sigma_row^2  +  (N/2) 2^(-2 t basebit)/12"
    assert formula in header and formula in integration and formula in (keygen.ring_rekey_sigma.__doc__ or "")
    for line in ("out[r]   = (0, b_r) - K[t] - sum_{j<t} D_j(X) K[j]", "abar_k   = a_k + off,  off = 2^(31 - t basebit)"):
        assert line in header and line in integration, line
    L = redsec_amd.load_library()
    assert "rs_ring_rekey_dev" in redsec_amd.ABI_SYMBOLS and hasattr(L, "rs_ring_rekey_dev")
    assert "rs_ring_rekey_dev" in integration and "rs_ring_rekey_dev" in design
    for f in ("ring_rekey", "upload_ring_rekey_key"):
        assert callable(getattr(redsec_amd.Backend, f))
    for f in ("ring_rekey_to", "ring_rekey_for"):
        assert callable(getattr(client.SecretKeySet, f))
    for f in ("ring_rekey", "ring_rekey_messages", "ring_rekey_key", "ring_rekey_sigma", "ring_rekey_default"):
        assert callable(getattr(keygen, f))
    for f in ("RingRekeyKey", "write_ring_rekey_key", "read_ring_rekey_key"):
        assert hasattr(client, f)
    assert (keygen.DOMAIN_RING_REKEY_MASK, keygen.DOMAIN_RING_REKEY_NOISE) == (16, 17) and "domain 16" in keygen.__doc__
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_ring_rekey", "rs_ring_rekey.hip", [])' in build and build.count('"rs_ring_rekey.h"') == 2
    assert "## 22." in integration and "rs_ring_rekey_dev" in open(os.path.join(ROOT, "README.md")).read()
    named = re.findall(r"profiles/r25/[\w./-]*\w", integration + design + open(os.path.join(ROOT, "profiles", "r25", "README.md")).read())
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
    assert L.rs_ring_rekey_dev(None, p, p, 1, p, 4, 5, None) == rc and L.rs_last_error() == msg
    assert L.rs_ring_rekey_dev(None, None, None, 0, None, 0, 0, None) == rc and L.rs_last_error() == msg


def test_new_kernels_hold_zero_scratch_and_no_static_lds():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    for pat, vgpr in (("17ring_rekey_kernel", 40), ("22ring_rekey_init_kernel", 16)):
        hit = {n: k for n, k in ks.items() if pat in n}
        assert len(hit) == 1, (pat, sorted(hit))
        for k in hit.values():
            assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= vgpr, (pat, k)   # the LDS is dynamic


def test_ring_rekey_sources_are_integer_only():
    """As rs_pack.* and rs_rekey.*: the sources name no floating type and include neither a transform nor the split-key product."""
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_ring_rekey.h", "rs_ring_rekey.hip", "rs_ring_sweep.h"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\b(double|float|half|__fp16|_Float16)\b|rs_general\.h|rs_fft\.h|rs_ntt\.h", code), f
