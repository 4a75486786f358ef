"""Evaluation keys generated on the device (rs_keygen_dev, redsec_amd/keygen.py): word for word against the numpy restatement,
noise statistics, and real keys end to end on all five parameter sets at full size -- the first decrypted evidence for
redsec_params_medium (N = 4096) and redsec_params_large (N = 8192)."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

SETS = ("default128", "redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large")
SEED = bytes(range(7, 39))


def _backend(name, n=None):
    import redsec_amd
    return redsec_amd.Backend(redsec_amd.params(name, n=n), device=0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _stdevs(name):
    (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    return bk_stdev, ks_stdev


def _free(*objs):
    import torch
    for o in objs:
        if hasattr(o, "close"):
            o.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,n", [("default128", None), ("redsec_small_v2", None), ("redsec_medium", 16), ("redsec_large", 16)])
def test_noiseless_key_equals_the_numpy_restatement_word_for_word(name, n):
    be = _backend(name, n)
    lwe, tlwe = keygen.secret_keys(name, SEED, n=be.p.n)
    bk, ksk = be.keygen(lwe, tlwe, SEED, 0.0, 0.0)
    want_bk, want_ksk = keygen.restate(name, SEED, lwe, tlwe, 0.0, 0.0)
    got_bk = bk.cpu().numpy()
    assert got_bk.shape == want_bk.shape
    bad = np.argwhere(got_bk != want_bk)
    assert len(bad) == 0, (len(bad), bad[:4].tolist())
    got_ksk = ksk.cpu().numpy()
    assert np.array_equal(got_ksk, want_ksk), np.argwhere(got_ksk != want_ksk)[:4].tolist()
    _free(be)


def _bk_errors(name, lwe, tlwe, bk):
    """e = b - a*S - gadget of every bk row (a with its own gadget term removed first)."""
    s = keygen._shape(name, len(lwe))
    l, Bgbit = s["l"], s["Bgbit"]
    rows = bk.reshape(-1, 2, bk.shape[-1]).view(np.uint32).copy()
    r = np.arange(rows.shape[0])
    p = r % (2 * l)
    c, j = p // l, p % l
    gadget = np.asarray(lwe, np.uint32)[r // (2 * l)] * (np.uint32(1) << (32 - (j + 1) * Bgbit).astype(np.uint32))
    with np.errstate(over="ignore"):
        rows[c == 0, 0, 0] -= gadget[c == 0]
        rows[c == 1, 1, 0] -= gadget[c == 1]
        e = rows[:, 1] - keygen._times_binary(np.ascontiguousarray(rows[:, 0]), tlwe)
    return e.view(np.int32).astype(np.int64)


def _ksk_errors(name, lwe, tlwe, ksk):
    s = keygen._shape(name, len(lwe))
    t, basebit, n = s["t"], s["basebit"], s["n"]
    base = 1 << basebit
    rows = ksk.reshape(-1, n + 1)
    r = np.arange(rows.shape[0])
    live = r % base != 0
    rows, r = rows[live], r[live]
    ij = r >> basebit
    i, j = ij // t, ij % t
    dot = (rows[:, :n].view(np.uint32).astype(np.uint64) * np.asarray(lwe, np.uint64)).sum(axis=-1)
    mess = (np.asarray(tlwe, np.uint64)[i] * (r % base).astype(np.uint64)) << (32 - (j + 1) * basebit).astype(np.uint64)
    e = (rows[:, n].view(np.uint32).astype(np.uint64) - dot - mess) & np.uint64(0xFFFFFFFF)
    return e.astype(np.uint32).view(np.int32).astype(np.int64)


def _truncated_std(scale):
    """Standard deviation of trunc(scale z), z ~ N(0, 1): TFHE's noise word for sigma = scale 2^-32."""
    z = np.linspace(-12.0, 12.0, 2_400_001)
    w = np.exp(-0.5 * z * z)
    v = np.trunc(scale * z)
    return float(np.sqrt((w * v * v).sum() / w.sum()))


@pytest.mark.parametrize("name", ["default128", "redsec_small_v2"])
def test_noise_of_the_whole_key_has_the_set_deviation(name):
    bk_stdev, ks_stdev = _stdevs(name)
    be = _backend(name)
    lwe, tlwe = keygen.secret_keys(name, SEED)
    bk0, ksk0 = (x.cpu().numpy() for x in be.keygen(lwe, tlwe, SEED, 0.0, 0.0))
    bk, ksk = (x.cpu().numpy() for x in be.keygen(lwe, tlwe, SEED, bk_stdev, ks_stdev))
    assert np.array_equal(bk[:, :, 0], bk0[:, :, 0])                 # the masks are those of the noiseless key
    assert np.array_equal(ksk[..., :-1], ksk0[..., :-1])
    for e, sigma, tol in ((_bk_errors(name, lwe, tlwe, bk), bk_stdev, 0.01), (_ksk_errors(name, lwe, tlwe, ksk), ks_stdev, 0.02)):
        scale = sigma * 2.0 ** 32
        want = _truncated_std(scale)                                  # = scale up to TFHE's truncation (4 -> 3.6 for small_v2 bk)
        assert abs(e.mean()) <= 4 * want / np.sqrt(e.size), (e.mean(), want, e.size)
        assert abs(e.std() / want - 1) <= tol, (e.std(), want, scale)
        assert np.abs(e).max() <= 7 * scale, (np.abs(e).max(), scale)
    # noise words agree with the host restatement except within a last-bit change of z
    rows = np.arange(0, bk.shape[0] * bk.shape[1], 97)
    want_bk, _ = keygen.restate(name, SEED, lwe, tlwe, bk_stdev, ks_stdev, rows=(rows, None))
    got = bk.reshape(-1, 2, bk.shape[-1])[rows]
    assert np.array_equal(got[:, 0], want_bk[:, 0]) and np.abs(got[:, 1].astype(np.int64) - want_bk[:, 1]).max() <= 1
    # same seed: same key; another seed: other masks
    bk2 = be.keygen(lwe, tlwe, SEED, bk_stdev, ks_stdev)[0].cpu().numpy()
    assert np.array_equal(bk2, bk)
    bk3 = be.keygen(lwe, tlwe, bytes(32), bk_stdev, ks_stdev)[0].cpu().numpy()
    assert np.mean(bk3[:, :, 0] == bk[:, :, 0]) < 1e-3
    _free(be)


@pytest.mark.parametrize("name", ["redsec_medium", "redsec_large"])
def test_noise_truncates_to_zero_on_the_large_rings(name):
    """sigma 2^32 < 2^-7 for both keys of these sets: TFHE's dtot32 truncation makes every noise word 0, so sampled rows of the full-size
    key equal the noiseless restatement exactly."""
    bk_stdev, ks_stdev = _stdevs(name)
    assert bk_stdev * 2 ** 32 < 2 ** -7 and ks_stdev * 2 ** 32 < 2 ** -7
    be = _backend(name)
    lwe, tlwe = keygen.secret_keys(name, SEED)
    bk, ksk = be.keygen(lwe, tlwe, SEED, bk_stdev, ks_stdev)
    p = be.p
    brows = np.array([0, 1, 5, p.n * 2 * p.bk_l // 2 + 3, p.n * 2 * p.bk_l - 1])
    krows = np.array([1, 3, 1001, p.N * p.ks_t * (1 << p.ks_basebit) - 1, p.N * p.ks_t * (1 << p.ks_basebit) // 2 + 1])
    want_bk, want_ksk = keygen.restate(name, SEED, lwe, tlwe, 0.0, 0.0, rows=(brows, krows))
    got_bk = bk.view(-1, 2, p.N)[brows.tolist()].cpu().numpy()
    got_ksk = ksk.view(-1, p.n + 1)[krows.tolist()].cpu().numpy()
    assert np.array_equal(got_bk, want_bk) and np.array_equal(got_ksk, want_ksk)
    del bk, ksk
    _free(be)


GATE_TRUTH = {"NAND": lambda a, b: 1 - (a & b), "OR": lambda a, b: a | b, "AND": lambda a, b: a & b, "NOR": lambda a, b: 1 - (a | b),
              "XOR": lambda a, b: a ^ b, "XNOR": lambda a, b: 1 - (a ^ b), "ANDNY": lambda a, b: (1 - a) & b, "ANDYN": lambda a, b: a & (1 - b),
              "ORNY": lambda a, b: (1 - a) | b, "ORYN": lambda a, b: a | (1 - b)}


@pytest.mark.parametrize("name", SETS)
def test_real_device_key_end_to_end_at_full_size(name):
    """keygen.generate at the set's full size; fresh host encryptions under the secret; all ten gates, MUX and a 4-level
    programmable bootstrap decrypt correctly for every sample."""
    import torch
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=SEED)
    del bk, ksk
    torch.cuda.empty_cache()
    B = 256 if be.p.N == 1024 else 64
    rng = np.random.default_rng(17)
    a, b, c = (rng.integers(0, 2, B) for _ in range(3))
    ca, cb, cc = (_dev(sk.encrypt_bits(x, seed=s)) for x, s in ((a, 1), (b, 2), (c, 3)))
    for op, f in GATE_TRUTH.items():
        got = sk.decrypt_bits(be.gate(op, ca, cb).cpu().numpy())
        assert np.array_equal(got, f(a, b)), (name, op, int(np.sum(got != f(a, b))))
    assert np.array_equal(sk.decrypt_bits(be.mux(ca, cb, cc).cpu().numpy()), np.where(a == 1, b, c))
    # 4 message levels m in [0, 4) at phase (2m + 1)/16 (the positive half of the torus), LUT m -> 3 - m at msize 16
    N = be.p.N
    m = rng.integers(0, 4, B)
    x = _dev(sk.encrypt_torus(client.modswitch_to_torus32(2 * m + 1, 16).astype(np.int64), seed=4))
    lut = np.zeros(N, np.int32)
    for level in range(4):
        lut[level * N // 4:(level + 1) * N // 4] = client.modswitch_to_torus32([2 * (3 - level) + 1], 16)[0]
    out = be.bootstrap_lut(x, _dev(lut[None]))
    ph = sk.phase(out.cpu().numpy()).view(np.uint32).astype(np.int64)
    assert np.array_equal(ph >> 29, 3 - m), (name, int(np.sum((ph >> 29) != 3 - m)))
    be.sync()
    _free(be)


def test_oracle_parity_and_both_load_paths_on_a_generated_key():
    import oracle_lib as ol
    name = "default128"
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=SEED, load=False)
    bk_h, ksk_h = bk.cpu().numpy(), ksk.cpu().numpy()
    be.load_keys_dev(bk, ksk)
    assert np.array_equal(bk.cpu().numpy(), bk_h) and np.array_equal(ksk.cpu().numpy(), ksk_h)   # inputs not modified
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 2, 8), rng.integers(0, 2, 8)
    ca, cb = sk.encrypt_bits(a, seed=5), sk.encrypt_bits(b, seed=6)
    mu = ol.to_torus(1, 8)
    dev_boot = be.bootstrap(_dev(ca), mu).cpu().numpy()
    dev_nand = be.gate("NAND", _dev(ca), _dev(cb)).cpu().numpy()
    be2 = _backend(name)
    be2.load_keys(bk_h, ksk_h)
    assert np.array_equal(be2.bootstrap(_dev(ca), mu).cpu().numpy(), dev_boot)
    assert np.array_equal(be2.gate("NAND", _dev(ca), _dev(cb)).cpu().numpy(), dev_nand)

    class K:
        pass
    ks = K()
    ks.p, ks.bk, ks.ksk = ol.params(name), bk_h.ravel(), ksk_h.ravel()
    ctx = ol.Ctx(ks)
    assert np.array_equal(ctx.bootstrap_batch(ca, mu), dev_boot)
    assert np.array_equal(ctx.gate_batch("NAND", ca, cb), dev_nand)
    assert np.array_equal(sk.decrypt_bits(dev_nand), 1 - (a & b))
    ctx.close()
    _free(be, be2)


def _w(s, z):
    return np.where(z == 1, 0, np.where(s == 1, 1, -1)).astype(np.int64)


@pytest.mark.parametrize("name", ["redsec_small_v2", "redsec_medium"])
def test_mnist_sign1024x1_under_a_device_generated_key(name):
    """One image of nets/mnist/sign1024x1 with the layer-wise assertions of test_gpu_mnist.py, under a key generated on the device.
    The tolerances on bootstrapped values widen by the set's own keyswitch rounding: t basebit = 18 bits at N = 4096 (medium) leave
    each coefficient's digits 2^-19 short at most, sum_i S_i delta_i of std sqrt(N / 24) 2^-18 = 0.20 / 4096 per output -- the
    parameter set's noise, present under any key (27 bits at the REDsec set: 2e-4 / 4096)."""
    import torch
    import plain_model as pm
    from redsec_amd import nets
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=SEED)
    del bk, ksk
    torch.cuda.empty_cache()
    p = be.p
    ks_round = np.sqrt(p.N / 24.0) * 2.0 ** -(p.ks_t * p.ks_basebit) * 4096   # std per bootstrapped output, in 1/4096
    net = pm.load_net("sign1024x1")
    enc = nets.EncryptedMnist(be, net)
    labels, pixels = pm.load_images()
    ct = torch.from_numpy(sk.encrypt_image(pixels[0], seed=100)).cuda()
    taps, ptaps = {}, {}
    out = enc.run(ct, taps)
    pm.forward(net, pixels[0], ptaps)
    assert out.shape == (10, be.W)
    pre0 = sk.decrypt_ints(taps["pre0"].cpu().numpy())
    assert np.abs(pre0 - ptaps["pre0"]).max() <= 2
    bits0 = np.where(sk.phase(taps["bits0"].cpu().numpy()) > 0, 1, -1)
    strong = np.abs(ptaps["pre0"]) >= 32
    assert np.array_equal(bits0[strong], ptaps["bits0"][strong])
    s, z, b = net.fc[0]
    W1 = _w(s, z)
    expect1 = bits0 @ W1 + b
    pre1 = sk.decrypt_ints(taps["pre1"].cpu().numpy())
    assert np.abs(pre1 - expect1).max() <= 2 + 6 * ks_round * np.sqrt(np.abs(W1).sum(axis=0).max())
    bits1 = np.where(sk.phase(taps["bits1"].cpu().numpy()) > 0, 1, -1)
    strong = np.abs(expect1) >= 32
    assert np.array_equal(bits1[strong], np.where(expect1 >= 0, 1, -1)[strong])
    ph = sk.phase(taps["bits1"].cpu().numpy()).astype(np.float64) / (1 << 20)
    assert np.all(np.abs(np.abs(ph) - 1.0) < max(0.25, 6 * ks_round))
    s, z, b = net.final
    W2 = _w(s, z)
    logits = sk.decrypt_ints(out.cpu().numpy())
    assert np.abs(logits - (bits1 @ W2 + b)).max() <= 3 + 6 * ks_round * np.sqrt(np.abs(W2).sum(axis=0).max())
    _free(be)


def test_invalid_arguments_and_isolation_of_the_loaded_key():
    import torch
    import oracle_lib as ol
    name = "redsec_small_v2"
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=SEED)
    ct = _dev(sk.encrypt_bits(np.arange(16) & 1, seed=9))
    mu = ol.to_torus(1, 8)
    before = be.bootstrap(ct, mu).cpu().numpy()
    lwe, tlwe = sk.lwe_key, sk.tlwe_key
    L = be.L
    vp = C.c_void_p
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    pbk, pksk = vp(bk.data_ptr()), vp(ksk.data_ptr())

    def call(bkp=pbk, kskp=pksk, lw=lwe, tl=tlwe, seed=SEED, s1=0.0, s2=0.0):
        return L.rs_keygen_dev(be.h, bkp, kskp, None if lw is None else i32(lw), None if tl is None else i32(tl), seed, s1, s2)
    assert call(bkp=None) == -1 and call(kskp=None) == -1 and call(lw=None) == -1 and call(tl=None) == -1 and call(seed=None) == -1
    bad = lwe.copy(); bad[3] = 2
    assert call(lw=bad) == -1 and b"lwe_key" in L.rs_last_error()
    bad = tlwe.copy(); bad[7] = -1
    assert call(tl=bad) == -1 and b"tlwe_key" in L.rs_last_error()
    for s1, s2 in ((-1e-9, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("inf"))):
        assert call(s1=s1, s2=s2) == -1, (s1, s2)
    assert L.rs_load_keys_dev(be.h, None, pksk) == -1
    # a key generated into other buffers (another seed) leaves the loaded one alone
    be.keygen(lwe, tlwe, bytes(32), 2.0 ** -30, 2.0 ** -25)
    assert call() == 0                      # also over the very tensors that were loaded: the context holds its own copy
    assert np.array_equal(be.bootstrap(ct, mu).cpu().numpy(), before)
    del bk, ksk
    torch.cuda.empty_cache()
    _free(be)
