"""Compressed evaluation keys without a GPU (include/redsec_hip.h, rs_keygen_compressed_dev / rs_expand_keys_dev; INTEGRATION.md
section 11): the numpy restatement against keygen.restate, a compressed toy key on the CPU oracle, the expansion of the device
functions (compiled into the lane emulator) against numpy, the RSZ1 file between client.py and the TFHE shim, the shim's own
compressed key generation, and the scratch budget of the new kernels."""
import ctypes as C
import io
import os
import re
import struct

import numpy as np
import pytest

import cppbuild
import emu_lib
from redsec_amd import client, keygen

SETS = ("default128", "redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large")
MASK_SEED = bytes(range(40, 72))
NOISE_SEED = bytes(range(200, 232))


def _stdevs(name):
    (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    return bk_stdev, ks_stdev


def _gadget(name, lwe, rows):
    s = keygen._shape(name, len(lwe))
    l, Bgbit = s["l"], s["Bgbit"]
    p = rows % (2 * l)
    c, j = p // l, p % l
    return c, np.asarray(lwe, np.uint32)[rows // (2 * l)] * (np.uint32(1) << (32 - (j + 1) * Bgbit).astype(np.uint32))


@pytest.mark.parametrize("name,n", [("redsec_small_v2", 20), ("default128", None)])
def test_numpy_compressed_key_relates_to_the_full_restatement(name, n):
    """Same seed for masks and noise at the numpy level: the ksk is equal word for word, c = 1 bk rows are equal, c = 0 rows
    differ by exactly -s_i g_j (1, S), and every row has the same phase."""
    bk_stdev, ks_stdev = _stdevs(name)
    seed = NOISE_SEED
    lwe, tlwe = keygen.secret_keys(name, seed, n=n)
    full_bk, full_ksk = keygen.restate(name, seed, lwe, tlwe, bk_stdev, ks_stdev)
    bk_body, ksk_body = keygen.restate_compressed(name, seed, seed, lwe, tlwe, bk_stdev, ks_stdev)
    bk, ksk = keygen.expand(name, seed, bk_body, ksk_body)
    assert bk.shape == full_bk.shape and ksk.shape == full_ksk.shape
    assert np.array_equal(ksk, full_ksk)
    rows_e, rows_f = bk.reshape(-1, 2, bk.shape[-1]).view(np.uint32), full_bk.reshape(-1, 2, bk.shape[-1]).view(np.uint32)
    r = np.arange(rows_e.shape[0])
    c, g = _gadget(name, lwe, r)
    assert np.array_equal(rows_e[c == 1], rows_f[c == 1])
    with np.errstate(over="ignore"):
        diff = rows_e[c == 0] - rows_f[c == 0]
        want = np.zeros_like(diff)
        want[:, 0, 0] = -g[c == 0]
        want[:, 1, :] = -(g[c == 0, None] * np.asarray(tlwe, np.uint32)[None, :])
        assert np.array_equal(diff, want)
        ph_e = rows_e[:, 1] - keygen._times_binary(np.ascontiguousarray(rows_e[:, 0]), tlwe)
        ph_f = rows_f[:, 1] - keygen._times_binary(np.ascontiguousarray(rows_f[:, 0]), tlwe)
    assert np.array_equal(ph_e, ph_f)
    assert np.mean(g[c == 0] != 0) > 0.3                          # the relation is not vacuous
    # sampled rows restate the same words as the whole key
    br, kr = np.array([0, 7, len(r) - 1]), np.array([1, 5, ksk_body.size - 1])
    sb, sk = keygen.restate_compressed(name, seed, seed, lwe, tlwe, bk_stdev, ks_stdev, rows=(br, kr))
    assert np.array_equal(sb, bk_body.reshape(-1, bk.shape[-1])[br]) and np.array_equal(sk, ksk_body.ravel()[kr])
    eb, ek = keygen.expand(name, seed, sb, sk, n=len(lwe), rows=(br, kr))
    assert np.array_equal(eb, bk.reshape(-1, 2, bk.shape[-1])[br]) and np.array_equal(ek, ksk.reshape(-1, len(lwe) + 1)[kr])


def test_compressed_masks_come_from_the_mask_seed_and_noise_from_the_noise_seed():
    name = "redsec_small_v2"
    bk_stdev, ks_stdev = _stdevs(name)
    lwe, tlwe = keygen.secret_keys(name, NOISE_SEED, n=12)
    b1, k1 = keygen.restate_compressed(name, MASK_SEED, NOISE_SEED, lwe, tlwe, bk_stdev, ks_stdev)
    b0, k0 = keygen.restate_compressed(name, MASK_SEED, NOISE_SEED, lwe, tlwe, 0.0, 0.0)
    b2, _ = keygen.restate_compressed(name, MASK_SEED, bytes(32), lwe, tlwe, bk_stdev, ks_stdev)
    b3, _ = keygen.restate_compressed(name, bytes(32), NOISE_SEED, lwe, tlwe, bk_stdev, ks_stdev)
    e = (b1.astype(np.int64) - b0) % (1 << 32)
    e = np.where(e >= 1 << 31, e - (1 << 32), e)
    assert 0 < np.abs(e).max() < 64 * bk_stdev * 2 ** 32            # noise only
    assert not np.array_equal(b1, b2) and np.abs(((b1.astype(np.int64) - b2) + (1 << 31)) % (1 << 32) - (1 << 31)).max() < 128 * bk_stdev * 2 ** 32
    assert np.mean(b3 == b1) < 1e-2                                   # another mask: another body
    ck = keygen.CompressedKey(name, 12, MASK_SEED, b1, k1)
    s = keygen._shape(name, 12)
    assert ck.nbytes == 32 + 4 * (b1.size + k1.size) == 32 + 4 * (12 * 2 * s["l"] * s["N"] + s["N"] * s["t"] * (1 << s["basebit"]))


def test_full_size_byte_counts_of_the_issue_table():
    mb = lambda name: (keygen.full_nbytes(name) / 1e6, keygen.CompressedKey(name, keygen._shape(name)["n"], bytes(32), None, None).nbytes / 1e6)
    assert [round(x, 1) for x in mb("default128")] == [113.7, 15.6]
    assert [round(x, 1) for x in mb("redsec_small_v2")] == [160.9, 29.0]
    assert round(mb("redsec_large")[0] / mb("redsec_large")[1], 1) == 8.0


@pytest.mark.parametrize("name,toy", [("default128", "toy"), ("redsec_small_v2", "toy_redsec")])
def test_compressed_toy_key_runs_all_gates_on_the_cpu_oracle(name, toy):
    import oracle_lib as ol
    p = ol.params(toy)
    lwe, tlwe = keygen.secret_keys(name, NOISE_SEED, n=p.n)
    bk_stdev, ks_stdev = _stdevs(name)
    bk_body, ksk_body = keygen.restate_compressed(name, MASK_SEED, NOISE_SEED, lwe, tlwe, bk_stdev, ks_stdev)
    bk, ksk = keygen.expand(name, MASK_SEED, bk_body, ksk_body)

    class K:
        pass
    ks = K()
    ks.p, ks.bk, ks.ksk = p, np.ascontiguousarray(bk).ravel(), np.ascontiguousarray(ksk).ravel()
    ctx = ol.Ctx(ks)
    sk = client.SecretKeySet.from_secret(name, lwe, tlwe)
    rng = np.random.default_rng(8)
    a, b, c = (rng.integers(0, 2, 24) for _ in range(3))
    ca, cb, cc = sk.encrypt_bits(a, seed=1), sk.encrypt_bits(b, seed=2), sk.encrypt_bits(c, seed=3)
    truth = {"NAND": lambda a, b: 1 - (a & b), "OR": lambda a, b: a | b, "AND": lambda a, b: a & b, "NOR": lambda a, b: 1 - (a | b),
             "XOR": lambda a, b: a ^ b, "XNOR": lambda a, b: 1 - (a ^ b), "ANDNY": lambda a, b: (1 - a) & b,
             "ANDYN": lambda a, b: a & (1 - b), "ORNY": lambda a, b: (1 - a) | b, "ORYN": lambda a, b: a | (1 - b)}
    for op, f in truth.items():
        assert np.array_equal(sk.decrypt_bits(ctx.gate_batch(op, ca, cb)), f(a, b)), op
    assert np.array_equal(sk.decrypt_bits(ctx.mux_batch(ca, cb, cc)), np.where(a == 1, b, c))
    ctx.close()


def _emu():
    L = emu_lib.lib()
    i32p = C.POINTER(C.c_int32)
    L.rs_emu_expand_bk_row.argtypes = [C.c_char_p, C.c_int, C.c_uint64, i32p, i32p]
    L.rs_emu_expand_ksk_sample.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_int32, i32p]
    return L, i32p


@pytest.mark.parametrize("name", SETS)
def test_emulated_device_expansion_equals_numpy(name):
    """rows spread over the whole index range of the full-size set, its last bk row and last ksk sample included."""
    L, i32p = _emu()
    s = keygen._shape(name)
    n, N = s["n"], s["N"]
    rows_bk = n * 2 * s["l"]
    samples = N * s["t"] * (1 << s["basebit"])
    rng = np.random.default_rng(len(name))
    br = np.unique(np.concatenate([[0, 1, rows_bk // 2, rows_bk - 1], rng.integers(0, rows_bk, 4)]))
    kr = np.unique(np.concatenate([[0, 1, 2, (1 << s["basebit"]) + 1, samples // 2 + 1, samples - 1], rng.integers(0, samples, 6)]))
    bodies = rng.integers(-(1 << 31), 1 << 31, (len(br), N), dtype=np.int64).astype(np.int32)
    kbodies = rng.integers(-(1 << 31), 1 << 31, len(kr), dtype=np.int64).astype(np.int32)
    want_bk, want_ksk = keygen.expand(name, MASK_SEED, bodies, kbodies, rows=(br, kr))
    for k, r in enumerate(br):
        out = np.zeros(2 * N, np.int32)
        L.rs_emu_expand_bk_row(MASK_SEED, N, int(r), np.ascontiguousarray(bodies[k]).ctypes.data_as(i32p), out.ctypes.data_as(i32p))
        assert np.array_equal(out.reshape(2, N), want_bk[k]), (name, int(r))
    for k, r in enumerate(kr):
        out = np.full(n + 1, 7, np.int32)
        L.rs_emu_expand_ksk_sample(MASK_SEED, n, s["basebit"], int(r), int(kbodies[k]), out.ctypes.data_as(i32p))
        assert np.array_equal(out, want_ksk[k]), (name, int(r))
    assert np.all(want_ksk[kr % (1 << s["basebit"]) == 0] == 0)


HEADER = struct.Struct("<I7i4d")   # redsec_amd/host/tfhe_shim.cpp ParamHeader


def _read_rss1(path):
    with open(path, "rb") as f:
        magic, n, N, k, l, bg, t, bb, *_ = HEADER.unpack(f.read(HEADER.size))
        assert magic == client.RS_MAGIC["RSS1"]
        rd = lambda count: np.frombuffer(f.read(4 * count), np.int32)
        lwe, tlwe = rd(n).copy(), rd(N).copy()
        bk = rd(n * 2 * l * 2 * N).reshape(n, 2 * l, 2, N)
        ksk = rd(N * t * (1 << bb) * (n + 1)).reshape(N, t, 1 << bb, n + 1)
        assert f.read(1) == b""
    return lwe, tlwe, bk, ksk


@pytest.fixture(scope="module")
def keyio():
    e = cppbuild.build("keyio_roundtrip")
    if e is None:
        pytest.skip("no host compiler")
    return e


def test_rsz1_roundtrips_between_client_and_shim(keyio, tmp_path):
    name = "redsec_small_v2"
    sk = client.SecretKeySet(name, seed=5, n=12)
    bk_stdev, ks_stdev = _stdevs(name)
    bk_body, ksk_body = keygen.restate_compressed(name, MASK_SEED, NOISE_SEED, sk.lwe_key, sk.tlwe_key, bk_stdev, ks_stdev)
    ck = keygen.CompressedKey(name, 12, MASK_SEED, bk_body, ksk_body)
    s_in, c_in, s_out, c_out = (str(tmp_path / n) for n in ("s.in", "c.in", "s.out", "c.out"))
    with open(s_in, "wb") as f:
        client.write_tfhe_keyset(f, sk, True, ks_stdev, bk_stdev)
    with open(c_in, "wb") as f:
        client.write_compressed_cloud_key(f, ck)
    raw = open(c_in, "rb").read()
    assert raw[:4] == b"RSZ1" and len(raw) == HEADER.size + ck.nbytes
    r = cppbuild.run(keyio, s_in, c_in, s_out, c_out)
    assert r.returncode == 0, r.stderr
    assert "n=12 N=1024 l=10 Bgbit=3 t=9 basebit=3" in r.stdout
    assert open(c_out, "rb").read() == raw                          # read as RSZ1, written back as RSZ1, byte for byte
    back = client.read_compressed_cloud_key(open(c_out, "rb"))
    assert back.name == name and back.n == 12 and back.mask_seed == MASK_SEED
    assert np.array_equal(back.bk_body, bk_body) and np.array_equal(back.ksk_body, ksk_body)
    with pytest.raises(AssertionError):
        client.read_compressed_cloud_key(io.BytesIO(raw + b"\0"))


@pytest.fixture(scope="module")
def shim_keygen():
    e = cppbuild.build("compressed_keygen")
    if e is None:
        pytest.skip("no host compiler")
    return e


@pytest.mark.parametrize("name,n", [("redsec_small_v2", 16), ("default128", 10)])
def test_shim_keygen_writes_a_compressed_cloud_key(shim_keygen, tmp_path, name, n):
    """REDSEC_KEY_FORMAT=compressed: the cloud key is header + 32 + body bytes; its expansion is the secret file's full key,
    and that key decrypts under the secret: every bk row and ksk sample has its message's phase up to the set's noise."""
    (_, N, _, l, Bgbit, t, basebit, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    sec, cloud = str(tmp_path / "secret.key"), str(tmp_path / "cloud.key")
    args = [str(v) for v in (n, N, l, Bgbit, t, basebit, repr(ks_stdev), repr(bk_stdev))] + [sec, cloud]
    r = cppbuild.run(shim_keygen, *args, env={"REDSEC_KEY_FORMAT": "compressed"})
    assert r.returncode == 0, r.stderr
    ck = client.read_compressed_cloud_key(open(cloud, "rb"))
    assert os.path.getsize(cloud) == HEADER.size + 32 + 4 * (n * 2 * l * N + N * t * (1 << basebit)) == HEADER.size + ck.nbytes
    lwe, tlwe, full_bk, full_ksk = _read_rss1(sec)
    bk, ksk = keygen.expand(name, ck.mask_seed, ck.bk_body, ck.ksk_body)
    assert np.array_equal(bk, full_bk) and np.array_equal(ksk, full_ksk)
    # bk: phase = b - a*S = e + s_i g_j X^0 (c = 1) or e - s_i g_j S (c = 0)
    rows = bk.reshape(-1, 2, N).view(np.uint32)
    c, g = _gadget(name, lwe, np.arange(rows.shape[0]))
    with np.errstate(over="ignore"):
        e = rows[:, 1] - keygen._times_binary(np.ascontiguousarray(rows[:, 0]), tlwe)
        e[c == 1, 0] -= g[c == 1]
        e[c == 0] += g[c == 0, None] * tlwe.astype(np.uint32)[None, :]
    e = e.view(np.int32).astype(np.int64)
    assert np.abs(e).max() <= 8 * bk_stdev * 2 ** 32 + 1 and np.abs(e).max() > 0
    # ksk: phase = message + e
    kk = ksk.reshape(-1, n + 1)
    srow = np.arange(kk.shape[0])
    live = srow % (1 << basebit) != 0
    ij = srow >> basebit
    mess = (tlwe[ij // t].astype(np.uint64) * (srow % (1 << basebit)).astype(np.uint64)) << (32 - ((ij % t) + 1) * basebit).astype(np.uint64)
    ph = (kk[:, n].view(np.uint32).astype(np.uint64) - (kk[:, :n].view(np.uint32).astype(np.uint64) * lwe.astype(np.uint64)).sum(axis=1) - mess) & np.uint64(0xFFFFFFFF)
    ph = ph.astype(np.uint32).view(np.int32).astype(np.int64)
    assert np.abs(ph[live]).max() <= 8 * ks_stdev * 2 ** 32 + 1 and np.all(kk[~live] == 0)
    # a second key gets a fresh mask seed
    cloud2 = str(tmp_path / "cloud2.key")
    assert cppbuild.run(shim_keygen, *(args[:-1] + [cloud2]), env={"REDSEC_KEY_FORMAT": "compressed"}).returncode == 0
    assert client.read_compressed_cloud_key(open(cloud2, "rb")).mask_seed != ck.mask_seed


def test_new_kernels_hold_zero_scratch():
    import test_kernel_budgets as kb
    ks = kb._kernels()
    hits = {n: k for n, k in ks.items() if re.search(r"16expand_bk_kernelILi1[0-3]E|17expand_ksk_kernel|20gen_keygen_bk_kernelILi1[0-3]E|17keygen_ksk_kernel", n)}
    assert len(hits) == 10, sorted(hits)
    for n, k in hits.items():
        assert k["scratch"] == 0, (n, k)


def test_compressed_bindings_exist():
    import redsec_amd
    for sym in ("rs_keygen_compressed_dev", "rs_expand_keys_dev", "rs_load_compressed_keys", "rs_load_compressed_keys_dev"):
        assert sym in redsec_amd.ABI_SYMBOLS
    for f in ("keygen_compressed", "expand_keys", "load_compressed_keys"):
        assert callable(getattr(redsec_amd.Backend, f))
    assert callable(keygen.generate_compressed)
