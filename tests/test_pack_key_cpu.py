"""The packing key on the device, without a GPU (include/redsec_hip.h rs_pack_keygen_dev, rs_pack_expand_dev, rs_audit_pack_key_dev;
INTEGRATION.md section 19): the emulated generator (its own tile / window-block / chunk-and-carry walk, compiled into the lane
emulator) equals keygen.pack_key word for word under directed ring secrets, the emulated expansion equals pack_key_mask beside the
body, the emulated audit (a sparse sweep over the listed bits of S, another loop than the generator's) equals keygen.pack_key_noise
and returns exactly the generator's domain-15 words, corrupted words move exactly the predicted noise words, and the three symbols
are everywhere they belong."""
import ctypes as C
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
KEY_SEED = bytes(range(9, 41))
_i32p = C.POINTER(C.c_int32)
RING_SET = {1024: "redsec_small_v2", 4096: "redsec_medium", 8192: "redsec_large"}
# (N, n, basebit, t): the three digit extremes at N = 1024 ((1, 32): g_j = 1 at 32 bits; (8, 4): the widest digit), then the large rings
SHAPES = [(1024, 3, 4, 5), (1024, 2, 1, 32), (1024, 2, 8, 4), (4096, 2, 4, 5), (8192, 2, 4, 5)]
SECRETS = ["zero", "ones", "bit0", "bitlast", "random"]
STDEV = 2.0 ** -25


def _p(a):
    return a.ctypes.data_as(_i32p)


def _emu():
    L = emu_lib.lib()
    L.rs_emu_pack_keygen_row.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint64, _i32p, C.c_int, _i32p, C.c_double, _i32p]
    L.rs_emu_pack_keygen_row.restype = None
    L.rs_emu_pack_expand_row.argtypes = [C.c_char_p, C.c_int, C.c_uint64, _i32p, _i32p]
    L.rs_emu_pack_expand_row.restype = None
    L.rs_emu_audit_pack_row.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint64, _i32p, _i32p, C.c_int, _i32p, _i32p]
    L.rs_emu_audit_pack_row.restype = None
    L.rs_emu_audit_reduce.argtypes = [_i32p, C.c_long, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    return L


def lwe_secret(n):
    """Both a 1 and a 0, so that rows with and without the gadget word are met."""
    return (np.arange(n) % 2 == 0).astype(np.int32)


def ring_secret(kind, N):
    """The directed ring secrets: nothing to add; every rotation (each window word of each tile is read, the wrap sign of every term);
    only X^0 (the window's upper end); only X^(N-1) (its lower end: all but one coefficient wrapped and negated); random."""
    S = np.zeros(N, np.int32)
    if kind == "ones":
        S[:] = 1
    elif kind == "bit0":
        S[0] = 1
    elif kind == "bitlast":
        S[N - 1] = 1
    elif kind == "random":
        S[:] = np.random.default_rng(N).integers(0, 2, N)
    else:
        assert kind == "zero"
    return S


def pack_gauss(seed, rows, N, stdev):
    """The generator's domain-15 noise words of the rows."""
    return keygen.noise32(keygen.chacha20_words(seed, keygen.DOMAIN_PACK_NOISE, np.asarray(rows, np.uint64), 4 * N), stdev).reshape(len(rows), N)


def _emu_keygen_row(L, N, n, basebit, t, row, lwe, S, stdev):
    out = np.full(N, 7, np.int32)
    L.rs_emu_pack_keygen_row(MASK_SEED, NOISE_SEED, N, basebit, t, int(row), _p(lwe), n, _p(S), float(stdev), _p(out))
    return out


def _emu_audit_row(L, N, n, basebit, t, row, stored, lwe, S, mask_seed=None):
    out = np.full(N, 7, np.int32)
    stored = np.ascontiguousarray(stored, np.int32)
    L.rs_emu_audit_pack_row(0 if mask_seed is None else 1, mask_seed, N, t, basebit, int(row), _p(stored), _p(lwe), n, _p(S), _p(out))
    return out


def _add(word, delta):
    return np.int32((int(word) + delta + (1 << 31)) % (1 << 32) - (1 << 31))


@pytest.mark.parametrize("stdev", [0.0, STDEV])
@pytest.mark.parametrize("kind", SECRETS)
@pytest.mark.parametrize("N,n,basebit,t", SHAPES)
def test_emulated_generator_equals_numpy_on_every_row(N, n, basebit, t, kind, stdev):
    L = _emu()
    lwe, S = lwe_secret(n), ring_secret(kind, N)
    want = keygen.pack_key(RING_SET[N], lwe, S, MASK_SEED, NOISE_SEED, basebit, t, stdev).reshape(n * t, N)
    for row in range(n * t):
        got = _emu_keygen_row(L, N, n, basebit, t, row, lwe, S, stdev)
        assert np.array_equal(got, want[row]), (row, np.flatnonzero(got != want[row])[:4].tolist())
    assert np.array_equal(want[[0, n * t - 1]], keygen.pack_key(RING_SET[N], lwe, S, MASK_SEED, NOISE_SEED, basebit, t, stdev, rows=[0, n * t - 1]))
    if kind == "zero":
        # b = e + s_i g_j X^0: the gadget word lands on coefficient 0 (tile 0) and nowhere else, and g_j = 1 at (1, 32), j = 31
        e = pack_gauss(NOISE_SEED, np.arange(n * t), N, stdev).view(np.uint32)
        g = (lwe[np.arange(n * t) // t].astype(np.uint32) << (32 - (np.arange(n * t) % t + 1) * basebit).astype(np.uint32))
        diff = want.view(np.uint32) - e
        assert np.array_equal(diff[:, 0], g) and not diff[:, 1:].any() and g.any() and not g.all()
        assert (basebit, t) != (1, 32) or g[31] == 1


@pytest.mark.parametrize("N,n,basebit,t", SHAPES)
def test_emulated_expansion_and_audit_rows_equal_numpy(N, n, basebit, t):
    L = _emu()
    name = RING_SET[N]
    lwe, S = lwe_secret(n), ring_secret("random", N)
    rows = np.arange(n * t)
    body = keygen.pack_key(name, lwe, S, MASK_SEED, NOISE_SEED, basebit, t, STDEV).reshape(n * t, N)
    mask = keygen.pack_key_mask(MASK_SEED, N, rows)
    full = np.stack([mask, body], axis=1)
    assert np.array_equal(full.reshape(n, t, 2, N), client.PackingKey(name, n, basebit, t, MASK_SEED, body).expand())
    want = pack_gauss(NOISE_SEED, rows, N, STDEV)
    assert want.any()
    assert np.array_equal(keygen.pack_key_noise(name, lwe, S, full, basebit, t), want)
    assert np.array_equal(keygen.pack_key_noise(name, lwe, S, body, basebit, t, mask_seed=MASK_SEED), want)
    assert np.array_equal(keygen.pack_key_noise(name, lwe, S, body[[n * t - 1, 1]], basebit, t, mask_seed=MASK_SEED, rows=[n * t - 1, 1]), want[[n * t - 1, 1]])
    clean = keygen.pack_key(name, lwe, S, MASK_SEED, NOISE_SEED, basebit, t, 0.0).reshape(n * t, N)
    for row in rows:
        out = np.full((2, N), 7, np.int32)
        L.rs_emu_pack_expand_row(MASK_SEED, N, int(row), _p(np.ascontiguousarray(body[row])), _p(out))
        assert np.array_equal(out, full[row]), row
        assert np.array_equal(_emu_audit_row(L, N, n, basebit, t, row, full[row], lwe, S), want[row]), ("full", row)
        assert np.array_equal(_emu_audit_row(L, N, n, basebit, t, row, body[row], lwe, S, MASK_SEED), want[row]), ("seeded", row)
        assert not _emu_audit_row(L, N, n, basebit, t, row, clean[row], lwe, S, MASK_SEED).any(), ("noise-free", row)
    assert not keygen.pack_key_noise(name, lwe, S, clean, basebit, t, mask_seed=MASK_SEED).any()


@pytest.mark.parametrize("N", [1024, 8192])
def test_corrupted_words_change_exactly_the_predicted_noise_words(N):
    L = _emu()
    name, n, basebit, t = RING_SET[N], 2, 4, 5
    lwe, S = lwe_secret(n), ring_secret("random", N)
    body = keygen.pack_key(name, lwe, S, MASK_SEED, NOISE_SEED, basebit, t, STDEV).reshape(n * t, N)
    set_bits = np.flatnonzero(S)
    delta, pos = 12345, N - 3
    for row in (1, n * t - 1):
        full = np.stack([keygen.pack_key_mask(MASK_SEED, N, [row])[0], body[row]])
        clean = _emu_audit_row(L, N, n, basebit, t, row, full, lwe, S)
        bad = full.copy()
        bad[1, 77] = _add(bad[1, 77], 1 << 20)
        for got in (_emu_audit_row(L, N, n, basebit, t, row, bad, lwe, S), _emu_audit_row(L, N, n, basebit, t, row, bad[1], lwe, S, MASK_SEED),
                    keygen.pack_key_noise(name, lwe, S, bad[1], basebit, t, mask_seed=MASK_SEED, rows=[row])[0]):
            diff = (got.astype(np.int64) - clean) % (1 << 32)
            assert np.flatnonzero(diff).tolist() == [77] and diff[77] == 1 << 20
        bad = full.copy()
        bad[0, pos] = _add(bad[0, pos], delta)
        diff = (_emu_audit_row(L, N, n, basebit, t, row, bad, lwe, S).astype(np.int64) - clean) % (1 << 32)
        want = np.zeros(N, np.int64)
        for m in set_bits:                         # X^m a: a[pos] lands at pos + m, negated once it wraps; the noise is b - a*S
            want[(pos + m) % N] = (-delta if pos + m < N else delta) % (1 << 32)
        assert np.array_equal(diff, want) and np.count_nonzero(diff) == len(set_bits)
        assert np.array_equal((keygen.pack_key_noise(name, lwe, S, bad[None], basebit, t, rows=[row])[0].astype(np.int64) - clean) % (1 << 32), want)


def test_a_key_of_another_secret_fails_the_audit():
    """Under another random S the noise words are uniform: with the limit of sigma = 2^-25 (about 1.1e3 in 2^32) all but 5e-7 of
    them exceed it, so well over half must."""
    L = _emu()
    N, n, basebit, t = 1024, 3, 4, 5
    name = RING_SET[N]
    lwe, S = lwe_secret(n), ring_secret("random", N)
    other = np.random.default_rng(77).integers(0, 2, N).astype(np.int32)
    assert 0 < (other != S).sum()
    body = keygen.pack_key(name, lwe, S, MASK_SEED, NOISE_SEED, basebit, t, STDEV).reshape(n * t, N)
    limit = keygen.pack_noise_limit(STDEV)
    assert limit == int(np.floor(8.58 * STDEV * 2.0 ** 32)) + 1 and 1000 < limit < 1200
    for secret, bad in ((S, False), (other, True)):
        e = np.stack([_emu_audit_row(L, N, n, basebit, t, row, body[row], lwe, secret, MASK_SEED) for row in range(n * t)])
        assert np.array_equal(e, keygen.pack_key_noise(name, lwe, secret, body, basebit, t, mask_seed=MASK_SEED))
        mag = np.abs(e.astype(np.int64))
        for parts in (1, 256):
            mx, over = C.c_uint32(), C.c_uint64()
            L.rs_emu_audit_reduce(_p(np.ascontiguousarray(e)), e.size, limit, parts, C.byref(mx), C.byref(over))
            assert (mx.value, over.value) == (mag.max(), (mag > limit).sum())
        assert (over.value > e.size // 2) if bad else (over.value == 0 and 0 < mx.value <= limit)
    # a wrong LWE bit moves coefficient 0 of that bit's rows by the gadget word, nothing else
    flipped = lwe.copy()
    flipped[1] ^= 1
    e = keygen.pack_key_noise(name, flipped, S, body, basebit, t, mask_seed=MASK_SEED)
    assert (np.abs(e.astype(np.int64)) > limit).sum() == t and (np.abs(e[t:2 * t, 0].astype(np.int64)) > limit).all()


def test_symbols_are_in_the_header_the_library_the_binding_the_recipe_and_the_documents():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    protos = [
        r"int rs_pack_keygen_dev\(rs_ctx\* ctx, int32_t\* body, const int32_t\* lwe_key, const int32_t\* tlwe_key,\s+const uint8_t\* mask_seed, "
        r"const uint8_t\* noise_seed, int32_t basebit, int32_t t, double stdev\);",
        r"int rs_pack_expand_dev\(rs_ctx\* ctx, int32_t\* pack_key, const uint8_t\* mask_seed, const int32_t\* body, int32_t t, void\* stream\);",
        r"int rs_audit_pack_key_dev\(rs_ctx\* ctx, rs_pack_key_audit\* report, int32_t\* noise, const int32_t\* key, const uint8_t\* mask_seed,\s+"
        r"const int32_t\* lwe_key, const int32_t\* tlwe_key, int32_t basebit, int32_t t, uint32_t limit\);",
        r"typedef struct rs_pack_key_audit \{\s+uint32_t max_abs;[^}]*uint64_t over;[^}]*uint64_t words;[^}]*\} rs_pack_key_audit;",
    ]
    for proto in protos:
        assert re.search(proto, header), proto
    L = redsec_amd.load_library()
    docs = {f: open(os.path.join(ROOT, f)).read() for f in ("INTEGRATION.md", "README.md", "DESIGN.md")}
    for sym in ("rs_pack_keygen_dev", "rs_pack_expand_dev", "rs_audit_pack_key_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS and hasattr(L, sym), sym
        assert sym in docs["INTEGRATION.md"] and sym in (keygen.__doc__ or ""), sym
    assert "rs_pack_keygen_dev" in docs["README.md"] and "rs_pack_keygen_dev" in docs["DESIGN.md"]
    assert re.search(r"^#+ 19\.", docs["INTEGRATION.md"], re.M)
    for f in ("pack_keygen", "expand_packing_key", "audit_packing_key", "upload_packing_key"):
        assert callable(getattr(redsec_amd.Backend, f)), f
    assert callable(client.SecretKeySet.audit_packing_key) and callable(keygen.pack_key_noise) and callable(keygen.pack_noise_limit)
    import inspect
    assert "backend" in inspect.signature(client.SecretKeySet.packing_key).parameters
    build = open(os.path.join(ROOT, "redsec_amd", "build.py")).read()
    assert '("rs_packkey", "rs_packkey.hip", [])' in build and '("rs_pack", "rs_pack.hip", [])' in build
    for stale in ("no device code for them", "pack_key; no device code", "device-side expansion is not part of this section"):
        for f in ("include/redsec_hip.h", "redsec_amd/csrc/rs_pack.h", "INTEGRATION.md"):
            assert stale not in open(os.path.join(ROOT, f)).read(), (stale, f)
    for path in re.findall(r"profiles/r21/[\w./-]*\w", "".join(docs.values()) + open(os.path.join(ROOT, "MEASUREMENTS.md")).read()):
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_failure_without_a_context_matches_pack():
    L = redsec_amd.load_library()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    rc = L.rs_pack_dev(None, p, p, 1, p, 4, 5, None)
    msg = L.rs_last_error()
    assert rc != 0
    key = (C.c_int32 * 8)()
    rep = redsec_amd.backend.RsPackKeyAudit()
    assert L.rs_pack_keygen_dev(None, p, key, key, MASK_SEED, NOISE_SEED, 4, 5, 0.0) == rc and L.rs_last_error() == msg
    assert L.rs_pack_keygen_dev(None, None, None, None, None, None, 0, 0, -1.0) == rc and L.rs_last_error() == msg
    assert L.rs_pack_expand_dev(None, p, MASK_SEED, p, 5, None) == rc and L.rs_last_error() == msg
    assert L.rs_pack_expand_dev(None, None, None, None, 0, None) == rc and L.rs_last_error() == msg
    assert L.rs_audit_pack_key_dev(None, C.byref(rep), None, p, None, key, key, 4, 5, 0) == rc and L.rs_last_error() == msg
    assert L.rs_audit_pack_key_dev(None, None, None, None, None, None, None, 0, 0, 0) == rc and L.rs_last_error() == msg


def test_new_kernels_hold_zero_scratch_and_no_static_lds():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    gen = {n: k for n, k in ks.items() if "18pack_keygen_kernel" in n}
    exp = {n: k for n, k in ks.items() if "18pack_expand_kernel" in n}
    aud = {n: k for n, k in ks.items() if re.search(r"17audit_pack_kernelILb[01]E", n)}
    assert len(gen) == 1 and len(exp) == 1 and len(aud) == 2, (sorted(gen), sorted(exp), sorted(aud))
    for k in gen.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 96 and k["lds"] == 0, k     # the LDS is dynamic: (N + 512 + N / 32) words
    for k in exp.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 32 and k["lds"] == 0, k
    for k in aud.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 64 and k["lds"] == 0, k     # dynamic, as audit_bk_kernel's
    # the bk audit kernels are still the two they were
    assert len([n for n in ks if re.search(r"15audit_bk_kernelILb[01]E", n)]) == 2


def test_generator_sources_include_no_transform_and_the_audit_stays_integer_only():
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    strip = lambda f: "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
    for f in ("rs_packkey.h", "rs_packkey.hip"):
        assert not re.search(r"rs_general\.h|rs_fft\.h|rs_bootstrap\.h|#include \"rs_ntt\.h\"", strip(f)), f
    for f in ("rs_audit.h", "rs_audit.hip"):
        assert not re.search(r"\b(double|float)\b|rs_general\.h|rs_fft\.h|#include \"rs_ntt\.h\"|rs_packkey\.h", strip(f)), f
    assert "audit_pack_kernel" in strip("rs_audit.hip") and "pack_keygen_kernel" in strip("rs_packkey.hip")
    for f in ("rs_pack.h", "rs_pack.hip"):                                    # the generator did not move in with the packing kernels
        assert "keygen_kernel" not in strip(f) and "rs_packkey.h" not in strip(f), f
