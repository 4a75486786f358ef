"""Circuit bootstrapping without a GPU (rs_ring_selector_dev, rs_circuit_bootstrap_dev): the numpy
restatement of the selector keyswitch against a brute-force sum, the lane emulator of the kernel against the numpy restatement,
selectors produced under real secrets from synthetic level samples against the formula, the noise of a CMUX under produced
selectors, files, refusals, defaults, symbols and kernel budgets."""
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

MASK_SEED = bytes(range(170, 202))
NOISE_SEED = bytes(range(51, 83))
KEY_SEED = bytes(range(19, 51))
NAME, N1, n1 = "redsec_small_v2", 1024, 350
KS_SHAPES = [(8, 4), (1, 1), (4, 6), (2, 12)]                  # (ks_basebit, ks_t); (8, 4) has off = 0
SIGMA_U = keygen.bootstrap_sigma(NAME)                         # the synthetic level samples: the set's bootstrap output noise, 2^-17.2


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _secret(seed=KEY_SEED, name=NAME):
    return client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, seed))


def _off(ks_basebit, ks_t):
    return 0 if ks_basebit * ks_t >= 32 else 1 << (31 - ks_basebit * ks_t)


def _extreme(rng, rows, n_src, basebit, l, ks_basebit, ks_t):
    """Random samples whose first and last coordinates x_i (the b word before its half step is added) are the extreme words and
    2^32 - off, which wraps x + off to 0."""
    ct = _words(rng, rows, n_src + 1)
    off = _off(ks_basebit, ks_t)
    ext = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, ((1 << 32) - off) & 0xFFFFFFFF], np.uint64).astype(np.uint32)
    for r in range(rows):
        half = 1 << (31 - (r % l + 1) * basebit)
        ct[r, 0] = ext[r % ext.size].view(np.int32)
        ct[r, n_src] = np.uint32((int(ext[(r + 2) % ext.size]) - half) & 0xFFFFFFFF).view(np.int32)
    return ct


def _brute(ct, basebit, l, key, ks_basebit, ks_t):
    """Python integers, one term at a time."""
    rows, n_src, N = ct.shape[0], ct.shape[1] - 1, key.shape[4]
    out = np.zeros((rows // l, 2 * l, 2, N), np.int64)
    for r in range(rows):
        k, j = divmod(r, l)
        for f in range(2):
            acc = [[0] * N, [0] * N]
            for i in range(n_src + 1):
                x = int(ct[r, i]) & 0xFFFFFFFF
                if i == n_src:
                    x += 1 << (31 - (j + 1) * basebit)
                x = (x + _off(ks_basebit, ks_t)) & 0xFFFFFFFF
                for q in range(ks_t):
                    d = (x >> (32 - (q + 1) * ks_basebit)) & ((1 << ks_basebit) - 1)
                    for p in range(2):
                        for c in range(N):
                            acc[p][c] -= d * (int(key[f, i, q, p, c]) & 0xFFFFFFFF)
            out[k, f * l + j] = np.array(acc, dtype=object) % (1 << 32)
    return out.astype(np.uint32).view(np.int32)


def test_the_numpy_selector_switch_equals_a_brute_force_sum():
    rng = np.random.default_rng(5)
    for (basebit, l), (ks_basebit, ks_t) in zip(((3, 2), (8, 3), (1, 31), (4, 1)), KS_SHAPES):
        rows = 2 * l if l < 8 else l
        ct = _extreme(rng, rows, 5, basebit, l, ks_basebit, ks_t)
        key = _words(rng, 2, 6, ks_t, 2, 8)
        assert np.array_equal(keygen.ring_selector_switch(ct, basebit, l, key, ks_basebit, ks_t), _brute(ct, basebit, l, key, ks_basebit, ks_t))


def _emu(ct, depth, basebit, l, n_src, N, key, ks_basebit, ks_t):
    E = emu_lib.lib()
    out = np.full((depth + 1, 2 * l, 2, N), 0x5A5A5A5A, np.int32)
    E.rs_emu_ring_selector(_p(ct), depth, basebit, l, n_src, N, _p(key), ks_basebit, ks_t, _p(out))
    assert (out[depth] == 0x5A5A5A5A).all()
    return out[:depth]


@pytest.mark.parametrize("n_src,depth,basebit,l,ks_basebit,ks_t",
                         [(6, 1, 4, 1, 4, 6), (7, 4, 4, 2, 8, 4), (8, 3, 3, 3, 1, 1), (21, 1, 7, 3, 2, 12), (13, 2, 1, 31, 4, 6)])
def test_the_emulated_selector_kernel_equals_numpy(n_src, depth, basebit, l, ks_basebit, ks_t):
    """N = 1024: both tiles, both polynomials, both families; coordinates one below, at and one past the chunk of eight and no
    multiple of it; rows 1, one register block of eight, one block + 1 and several blocks; the extreme words."""
    E = emu_lib.lib()
    E.rs_emu_ring_selector_groups.restype = C.c_long
    E.rs_emu_ring_selector_offset.restype = C.c_uint32
    assert (E.rs_emu_ring_selector_chunk(), E.rs_emu_ring_selector_rows()) == (8, 8)
    rows = depth * l
    assert E.rs_emu_ring_selector_groups(C.c_long(rows), N1, n_src) == -(-rows // 8) * 4 * (N1 // 512) * -(-(n_src + 1) // 8)
    assert E.rs_emu_ring_selector_offset(ks_basebit, ks_t) == _off(ks_basebit, ks_t)
    rng = np.random.default_rng(n_src + 100 * depth + 7 * ks_t)
    ct = _extreme(rng, rows, n_src, basebit, l, ks_basebit, ks_t)
    key = _words(rng, 2, n_src + 1, ks_t, 2, N1)
    want = keygen.ring_selector_switch(ct, basebit, l, key, ks_basebit, ks_t)
    assert want.shape == (depth, 2 * l, 2, N1)
    assert np.array_equal(_emu(ct, depth, basebit, l, n_src, N1, key, ks_basebit, ks_t), want)


def _level_samples(sk, bits, basebit, l, rng, sigma_u):
    """Synthetic bootstraps: row k l + j encrypts +-h_j/2 (+ for a bit of 1) under the LWE key with Gaussian noise of sigma_u."""
    s = np.asarray(sk.lwe_key, np.int64)
    rows = len(bits) * l
    a = _words(rng, rows, s.size)
    half = np.array([1 << (31 - (j + 1) * basebit) for j in range(l)], np.int64)[np.arange(rows) % l]
    sign = np.repeat(2 * np.asarray(bits, np.int64) - 1, l)
    e = np.rint(rng.normal(0.0, sigma_u, rows) * 2.0 ** 32).astype(np.int64)
    b = (a.astype(np.int64) @ s + sign * half + e) & 0xFFFFFFFF
    return np.concatenate([a, b.astype(np.uint32).view(np.int32)[:, None]], axis=1)


def _phase(rows, S):
    """b - a*S of ring samples [..., 2, N] -> int64 centred words [..., N]"""
    flat = np.ascontiguousarray(rows, np.int32).reshape(-1, 2, rows.shape[-1])
    ph = (_u32(flat[:, 1]) - keygen._times_binary(np.ascontiguousarray(_u32(flat[:, 0])), S)).view(np.int32).astype(np.int64)
    return ph.reshape(rows.shape[:-2] + (rows.shape[-1],))


@pytest.fixture(scope="module")
def made():
    """one secret, its selector key at (7, 3), and selectors produced from synthetic level samples of eight bits at (4, 3)"""
    sk = _secret()
    key = sk.selector_key(7, 3, MASK_SEED, NOISE_SEED)
    rng = np.random.default_rng(77)
    bits = [1, 0, 1, 1, 0, 0, 1, 0]
    ct = _level_samples(sk, bits, 4, 3, rng, SIGMA_U)
    sel = keygen.ring_selector_switch(ct, 4, 3, key.expand(), 7, 3)
    return sk, key, bits, sel


def test_a_produced_selector_decrypts_to_the_gadget_rows(made):
    """rows l + j: m h_j at coefficient 0; rows j < l: -m h_j S; every coefficient within 8 sigma of the formula"""
    sk, key, bits, sel = made
    basebit, l = 4, 3
    S = np.asarray(sk.tlwe_key, np.int64)
    sw, skey = keygen.selector_row_sigma(n1, 7, 3, SIGMA_U, keygen.ring_selector_default_stdev(NAME))
    ph = _phase(sel, S)                                            # [depth][2l][N]
    worst = 0.0
    for k, m in enumerate(bits):
        for j in range(l):
            h = 1 << (32 - (j + 1) * basebit)
            want0 = (-m * h * S) & 0xFFFFFFFF
            want1 = np.zeros(N1, np.int64)
            want1[0] = m * h
            for row, want, where in ((ph[k, j], want0, S == 1), (ph[k, l + j], want1, np.arange(N1) == 0)):
                err = ((row - want + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
                sigma = np.sqrt(np.where(where, sw * sw, 0.0) + skey * skey) * 2.0 ** 32
                worst = max(worst, float(np.abs(err / sigma).max()))
    print("worst |error| / sigma over the produced rows: %.2f" % worst)
    assert worst <= 8.0


def test_a_lookup_under_produced_selectors_returns_the_entry(made):
    sk, key, bits, sel = made
    rng = np.random.default_rng(3)
    table = keygen.ring_trivial((rng.integers(0, 16, (8, N1)) << 28).astype(np.uint32).view(np.int32))
    index = bits[0] + 2 * bits[1] + 4 * bits[2]
    out = keygen.ring_lookup(table, sel[:3], 4, 3)
    err = _phase(out, np.asarray(sk.tlwe_key, np.int64)) - table[index, 1].astype(np.int64)
    err = ((err + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    sigma = keygen.circuit_bootstrap_sigma(N1, n1, 4, 3, 7, 3, SIGMA_U, keygen.ring_selector_default_stdev(NAME), depth=3,
                                           coefficient=np.arange(N1))
    print("worst |error| / sigma_c of the lookup: %.2f" % np.abs(err / (sigma * 2.0 ** 32)).max())
    assert (np.abs(err) <= 8 * sigma * 2.0 ** 32).all() and np.abs(err).max() < 1 << 27


SECRETS, BITS = 3, 8


def test_the_noise_of_a_cmux_under_produced_selectors_follows_the_formula():
    """SECRETS fresh secrets, BITS produced selectors each at (4, 3) over keys at (7, 3), one CMUX of two noise-free ring ciphertexts
    with random masks per selector; the squared error of every coefficient over the formula's variance for that coefficient and
    the selector's bit (circuit_bootstrap_sigma; bit = 0 leaves the CMUX rounding out). The error of a level is its ONE sample
    error w_j times a digit polynomial, so the independent draws are the SECRETS BITS l = 72 values w_j, not the coefficients: the
    mean of the ratio has relative deviation sqrt(2 / 72) = 0.17, and the accepted band is four of them either side, 0.33 .. 1.67
    in variance. Measured: see INTEGRATION.md section 24. Without the digits' mean (the first form of the formula) the ratio was
    2.45."""
    basebit, l, ks_basebit, ks_t = 4, 3, 7, 3
    stdev = keygen.ring_selector_default_stdev(NAME)
    rng = np.random.default_rng(2024)
    ratios = []
    for q in range(SECRETS):
        sk = _secret(bytes((b + 31 * q + 5) & 0xFF for b in range(32)))
        S = np.asarray(sk.tlwe_key, np.int64)
        key = sk.selector_key(ks_basebit, ks_t, bytes((b + q) & 0xFF for b in MASK_SEED), bytes((b + q) & 0xFF for b in NOISE_SEED)).expand()
        bits = [int(v) for v in rng.integers(0, 2, BITS)]
        sel = keygen.ring_selector_switch(_level_samples(sk, bits, basebit, l, rng, SIGMA_U), basebit, l, key, ks_basebit, ks_t)
        for k, m in enumerate(bits):
            mu = (rng.integers(0, 16, (2, N1)) << 28).astype(np.uint32)
            a = _u32(_words(rng, 2, N1))
            d = np.stack([a, keygen._times_binary(np.ascontiguousarray(a), S) + mu], axis=1).view(np.int32)    # [2][2][N]
            out = keygen.ring_cmux(d[1:2], d[0:1], sel[k], basebit, l)
            err = _phase(out, S)[0] - mu[m].astype(np.int64)
            err = (((err + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)) / 2.0 ** 32
            sigma = keygen.circuit_bootstrap_sigma(N1, n1, basebit, l, ks_basebit, ks_t, SIGMA_U, stdev, bit=m, coefficient=np.arange(N1))
            ratios.append(float(np.mean(err * err / sigma ** 2)))
    ratio = float(np.mean(ratios))
    band = 4 * np.sqrt(2.0 / (SECRETS * BITS * l))
    print("variance / formula = %.3f (rms / formula %.3f), band %.2f .. %.2f" % (ratio, np.sqrt(ratio), 1 - band, 1 + band))
    assert 1 - band <= ratio <= 1 + band


def test_key_rows_and_file_round_trip(made):
    sk, key, _, _ = made
    assert key.body.shape == (2, n1 + 1, 3, N1) and key.expand().shape == (2, n1 + 1, 3, 2, N1) and key.nbytes == 32 + 4 * N1 * 2 * (n1 + 1) * 3
    assert np.array_equal(key.expand()[:, :, :, 1], key.body)
    rows = 2 * (n1 + 1) * 3
    assert np.array_equal(key.expand()[:, :, :, 0].reshape(rows, N1), keygen.selector_key_mask(MASK_SEED, N1, np.arange(rows)))
    # the rows under the secret: family 1 sg_i g_q at coefficient 0, family 0 -sg_i g_q S, within the Gaussian bound
    S, s = np.asarray(sk.tlwe_key, np.int64), np.asarray(sk.lwe_key, np.int64)
    ph = _phase(key.expand(), S)
    sg = np.concatenate([s, [-1]])
    bound = keygen.GAUSS_BOUND * keygen.ring_selector_default_stdev(NAME) * 2.0 ** 32 + 1
    for q in range(3):
        g = sg << (32 - (q + 1) * 7)
        want1 = np.zeros((n1 + 1, N1), np.int64)
        want1[:, 0] = g
        for f, want in ((1, want1), (0, -g[:, None] * S[None, :])):
            err = ((ph[f, :, q] - want + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
            assert np.abs(err).max() <= bound and np.abs(err).max() > 0
    buf = io.BytesIO()
    client.write_selector_key(buf, key)
    raw = buf.getvalue()
    hs = client._RS_HEADER.itemsize
    assert len(raw) == hs + 8 + key.nbytes and raw[:4] == b"RSB1"
    back = client.read_selector_key(io.BytesIO(raw))
    assert (back.name, back.n, back.N, back.ks_basebit, back.ks_t, back.mask_seed) == (NAME, n1, N1, 7, 3, MASK_SEED)
    assert np.array_equal(back.body, key.body)
    digits = lambda *v: raw[:hs] + np.array(v, "<i4").tobytes() + raw[hs + 8:]
    bad_shape = np.frombuffer(raw[:hs], client._RS_HEADER).copy()
    bad_shape["N"] = 512
    for damaged in (raw[:-4], raw + b"\0\0\0\0", raw[:40], raw[:3], b"", raw[:hs + 4], b"RSG1" + raw[4:], digits(9, 3), digits(0, 3),
                    digits(7, 0), digits(7, 5), digits(7, 2), digits(8, 5), digits(7, 4), bad_shape.tobytes() + raw[hs:],
                    client._rs_header("RSB1", NAME, n1 + 1) + raw[hs:], client._rs_header("RSB1", NAME, 0) + raw[hs:]):
        with pytest.raises(ValueError):
            client.read_selector_key(io.BytesIO(damaged))
    with pytest.raises(ValueError):
        client.read_ring_selector(io.BytesIO(raw))                         # a selector key is not an RSG1 file
    assert client.RS_MAGIC["RSB1"] not in [v for k, v in client.RS_MAGIC.items() if k != "RSB1"]


def test_refusals():
    sk = _secret()
    with pytest.raises(ValueError, match="equal"):
        sk.selector_key(7, 3, MASK_SEED, MASK_SEED)
    z = np.zeros((1, 4), np.int32)
    for ks_basebit, ks_t in ((0, 4), (9, 2), (4, 0), (4, 9), (8, 5), (1, 33)):
        with pytest.raises(ValueError):
            sk.selector_key(ks_basebit, ks_t, MASK_SEED, NOISE_SEED)
        with pytest.raises(ValueError):
            keygen.ring_selector_switch(z, 4, 1, np.zeros((2, 4, max(ks_t, 1), 2, 16), np.int32), ks_basebit, ks_t)
        with pytest.raises(ValueError):
            keygen.circuit_bootstrap_sigma(1024, 350, 4, 3, ks_basebit, ks_t, 0.0, 0.0)
    for basebit, l in ((0, 4), (9, 2), (4, 0), (4, 8), (1, 32)):
        with pytest.raises(ValueError):
            keygen.ring_selector_switch(z, basebit, l, np.zeros((2, 4, 3, 2, 16), np.int32), 7, 3)
    with pytest.raises(ValueError, match="default128"):
        _secret(name="default128").selector_key(mask_seed=MASK_SEED, noise_seed=NOISE_SEED)


def test_failure_without_a_context_matches_pack():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    rc = L.rs_pack_dev(None, p, p, 1, p, 4, 5, None)
    msg = L.rs_last_error()
    assert rc != 0
    assert L.rs_ring_selector_dev(None, p, p, 1, 4, 3, 5, p, 7, 3, None) == rc and L.rs_last_error() == msg
    assert L.rs_ring_selector_dev(None, None, None, 0, 0, 0, 0, None, 0, 0, None) == rc and L.rs_last_error() == msg
    assert L.rs_circuit_bootstrap_dev(None, p, p, 1, 4, 3, p, 7, 3, p, None) == rc and L.rs_last_error() == msg
    assert L.rs_circuit_bootstrap_dev(None, None, None, 0, 0, 0, None, 0, 0, None, None) == rc and L.rs_last_error() == msg


# (set, depth, payload step) -> the default shape; INTEGRATION.md section 24 has the table
REACHED = {(NAME, 1, 1 / 16): (4, 3, 7, 3), (NAME, 3, 1 / 8): (4, 3, 7, 3), (NAME, 2, 1 / 8): (6, 2, 6, 4), (NAME, 10, 1 / 4): (6, 2, 5, 5),
           ("redsec_small", 1, 1 / 4): (5, 2, 7, 3)}
UNREACHED = [(NAME, 2, 1 / 16), (NAME, 3, 1 / 16), (NAME, 10, 1 / 8), (NAME, 1, 1 / 4096), ("redsec_small", 1, 1 / 8), ("redsec_small", 2, 1 / 4)] + \
            [(name, depth, step) for name in ("default128", "redsec_medium", "redsec_large") for depth in (1, 10) for step in (1 / 16, 1 / 4)]


def test_the_default_table():
    """8 circuit_bootstrap_sigma of the worst coefficient inside half of the payload step, for the smallest l and then the smallest
    ks_t that reach it; ValueError where no shape does: every step on default-128, whose bootstrap output noise (2^-8.2) no shape can
    absorb, and on the two large rings; on redsec_small_v2 steps of 1/16 past depth 1."""
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert keygen.bootstrap_sigma(NAME) == pytest.approx(2.0 ** -17.23, rel=0.02)
    assert keygen.bootstrap_sigma("default128") == pytest.approx(2.0 ** -8.15, rel=0.02)
    assert keygen.circuit_bootstrap_default(NAME) == REACHED[(NAME, 1, 1 / 16)]
    for (name, depth, step), shape in REACHED.items():
        v = client.PARAM_SETS[name]
        su, sk = keygen.bootstrap_sigma(name), keygen.ring_selector_default_stdev(name)
        b, l, kb, kt = keygen.circuit_bootstrap_default(name, depth, step)
        sigma = keygen.circuit_bootstrap_sigma(v[1], v[0], b, l, kb, kt, su, sk, depth)
        print("%s depth %d step %g (%d, %d, %d, %d): sigma 2^%.2f" % (name, depth, step, b, l, kb, kt, np.log2(sigma)))
        assert (b, l, kb, kt) == shape and 8 * sigma <= step / 2 and l * b <= 31 and kb * kt <= 32
        # the worst coefficient is the first, and no smaller l reaches the step
        assert sigma == keygen.circuit_bootstrap_sigma(v[1], v[0], b, l, kb, kt, su, sk, depth, coefficient=np.arange(v[1])).max()
        assert all(8 * keygen.circuit_bootstrap_sigma(v[1], v[0], bb, l - 1, kk, t, su, sk, depth) > step / 2
                   for bb in range(1, 9) if l > 1 and bb * (l - 1) <= 31 for t in range(1, 33) for kk in range(1, 9) if kk * t <= 32)
    for name, depth, step in UNREACHED:
        with pytest.raises(ValueError, match="no shape"):
            keygen.circuit_bootstrap_default(name, depth, step)
    assert "default-128" in integration and "## 24." in integration


def test_symbols_prototypes_and_formula_are_in_the_header_the_library_the_binding_the_recipe_and_the_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert re.search(r"int rs_ring_selector_dev\(rs_ctx\* ctx, int32_t\* sel, const int32_t\* ct, int32_t depth, int32_t basebit, int32_t l,\s+"
                     r"int32_t n_src, const int32_t\* sel_key, int32_t ks_basebit, int32_t ks_t, void\* stream\);", header)
    assert re.search(r"int rs_circuit_bootstrap_dev\(rs_ctx\* ctx, int32_t\* sel, const int32_t\* bits, int32_t depth, int32_t basebit, int32_t l,\s+"
                     r"const int32_t\* sel_key, int32_t ks_basebit, int32_t ks_t, int32_t\* scratch, void\* stream\);", header)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert len(design.splitlines()) <= 250
    formula = ("sigma^2 = depth (l sigma_w^2 ((1 + N/2)(B^2 - 1)/12 + ((1 - t_c)^2 + N/4)/4)  +  2 l N (B^2 + 2)/12 sigma_key^2  +  "
               "(1 + N/2) 2^(-2 l basebit)/12)")
    assert formula in integration and formula in (keygen.circuit_bootstrap_sigma.__doc__ or "")
    line = "sel[k][f l + j] = - sum_{i <= n_src, q < ks_t} d_iq K[f][i][q]"
    assert line in header and line in integration
    L = redsec_amd.load_library()
    for sym in ("rs_ring_selector_dev", "rs_circuit_bootstrap_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and hasattr(L, sym)
        assert sym in integration and sym in design and sym in readme
    for f in ("ring_selector", "circuit_bootstrap", "upload_selector_key"):
        assert callable(getattr(redsec_amd.Backend, f))
    from redsec_amd import arith
    assert callable(arith.lookup) and callable(client.SecretKeySet.selector_key)
    for f in ("selector_key", "selector_key_expand", "ring_selector_switch", "circuit_bootstrap_sigma", "circuit_bootstrap_default",
              "bootstrap_sigma", "selector_row_sigma"):
        assert callable(getattr(keygen, f))
    for f in ("SelectorKey", "write_selector_key", "read_selector_key"):
        assert hasattr(client, f)
    assert (keygen.DOMAIN_SELECTOR_KEY_MASK, keygen.DOMAIN_SELECTOR_KEY_NOISE) == (20, 21) and "domain 20" in keygen.__doc__
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_ring_selector", "rs_ring_selector.hip", [])' in build and build.count('"rs_ring_selector.h"') == 2
    named = re.findall(r"profiles/r27/[\w./-]*\w", integration + design + open(os.path.join(ROOT, "profiles", "r27", "README.md")).read())
    assert named
    for path in named:
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_new_kernels_hold_zero_scratch():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    for pat, vgpr, lds in (("20ring_selector_kernel", 128, 256), ("25ring_selector_init_kernel", 16, 0), ("22circuit_prepare_kernel", 16, 0)):
        hit = {n: k for n, k in ks.items() if pat in n}
        assert len(hit) == 1, (pat, sorted(hit))
        for k in hit.values():
            assert k["scratch"] == 0 and k["lds"] == lds and k["vgpr"] <= vgpr, (pat, k)


def test_ring_selector_sources_are_integer_only():
    """As rs_pack.*, rs_rekey.*, rs_ring_rekey.* and rs_ring_cmux.*: the sources name no floating type and include neither a
    transform nor the split-key product."""
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_ring_selector.h", "rs_ring_selector.hip"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\b(double|float|half|__fp16|_Float16)\b|rs_general\.h|rs_fft\.h|rs_ntt\.h", code), f
