"""Compressed evaluation keys on the device (rs_keygen_compressed_dev, rs_expand_keys_dev, rs_load_compressed_keys[_dev]): word for
word against the numpy restatement, the relation to rs_keygen_dev's key, three load paths against each other and the CPU oracle,
full-size end to end on all five sets from host bodies, MNIST, the unmodified reference tools with a compressed cloud.key, and
invalid input."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

SETS = ("default128", "redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large")
MASK_SEED = bytes(range(40, 72))
NOISE_SEED = bytes(range(7, 39))


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


def _sample_rows(p):
    rows_bk, samples = p.n * 2 * p.bk_l, p.N * p.ks_t * (1 << p.ks_basebit)
    br = np.array([0, 1, 2, 5, rows_bk // 2 + 3, rows_bk - 2, rows_bk - 1])
    kr = np.array([0, 1, 3, 1001, samples // 2 + 1, samples - 2, samples - 1])
    return br, kr


@pytest.mark.parametrize("name", SETS)
def test_compressed_bodies_and_expansion_equal_numpy(name):
    """Noiseless bodies equal the restatement word for word (whole keys at N = 1024, sampled rows at full size for medium / large);
    the device expansion of those bodies equals the numpy expansion."""
    import torch
    be = _backend(name)
    p = be.p
    lwe, tlwe = keygen.secret_keys(name, NOISE_SEED)
    bk_body, ksk_body = be.keygen_compressed(lwe, tlwe, MASK_SEED, NOISE_SEED, 0.0, 0.0)
    bk, ksk = be.expand_keys(MASK_SEED, bk_body, ksk_body)
    if p.N == 1024:
        want_b, want_k = keygen.restate_compressed(name, MASK_SEED, NOISE_SEED, lwe, tlwe, 0.0, 0.0)
        hb, hk = bk_body.cpu().numpy(), ksk_body.cpu().numpy()
        assert np.array_equal(hb, want_b), np.argwhere(hb != want_b)[:4].tolist()
        assert np.array_equal(hk, want_k)
        eb, ek = keygen.expand(name, MASK_SEED, hb, hk)
        assert np.array_equal(bk.cpu().numpy(), eb) and np.array_equal(ksk.cpu().numpy(), ek)
    else:
        br, kr = _sample_rows(p)
        want_b, want_k = keygen.restate_compressed(name, MASK_SEED, NOISE_SEED, lwe, tlwe, 0.0, 0.0, rows=(br, kr))
        hb = bk_body.view(-1, p.N)[br.tolist()].cpu().numpy()
        hk = ksk_body.view(-1)[kr.tolist()].cpu().numpy()
        assert np.array_equal(hb, want_b) and np.array_equal(hk, want_k)
        eb, ek = keygen.expand(name, MASK_SEED, hb, hk, rows=(br, kr))
        assert np.array_equal(bk.view(-1, 2, p.N)[br.tolist()].cpu().numpy(), eb)
        assert np.array_equal(ksk.view(-1, p.n + 1)[kr.tolist()].cpu().numpy(), ek)
    del bk, ksk, bk_body, ksk_body
    torch.cuda.empty_cache()
    _free(be)


@pytest.mark.parametrize("name", ["default128", "redsec_small_v2"])
def test_noisy_bodies_match_numpy_and_relate_to_the_full_device_key(name):
    bk_stdev, ks_stdev = _stdevs(name)
    be = _backend(name)
    lwe, tlwe = keygen.secret_keys(name, NOISE_SEED)
    bk_body, ksk_body = (x.cpu().numpy() for x in be.keygen_compressed(lwe, tlwe, MASK_SEED, NOISE_SEED, bk_stdev, ks_stdev))
    want_b, want_k = keygen.restate_compressed(name, MASK_SEED, NOISE_SEED, lwe, tlwe, bk_stdev, ks_stdev)
    assert np.abs(bk_body.astype(np.int64) - want_b).max() <= 1 and np.mean(bk_body == want_b) >= 0.999
    assert np.abs(ksk_body.astype(np.int64) - want_k).max() <= 1 and np.mean(ksk_body == want_k) >= 0.999
    # noiseless: the expanded key against rs_keygen_dev's key of the same secret and masks (seed = the mask seed)
    b0, k0 = be.keygen_compressed(lwe, tlwe, MASK_SEED, NOISE_SEED, 0.0, 0.0)
    ebk, eksk = (x.cpu().numpy() for x in be.expand_keys(MASK_SEED, b0, k0))
    fbk, fksk = (x.cpu().numpy() for x in be.keygen(lwe, tlwe, MASK_SEED, 0.0, 0.0))
    assert np.array_equal(eksk, fksk)
    re_, rf = ebk.reshape(-1, 2, be.p.N).view(np.uint32), fbk.reshape(-1, 2, be.p.N).view(np.uint32)
    r = np.arange(re_.shape[0])
    s = keygen._shape(name)
    pp = r % (2 * s["l"])
    c, j = pp // s["l"], pp % s["l"]
    g = lwe.astype(np.uint32)[r // (2 * s["l"])] * (np.uint32(1) << (32 - (j + 1) * s["Bgbit"]).astype(np.uint32))
    assert np.array_equal(re_[c == 1], rf[c == 1])
    with np.errstate(over="ignore"):
        d = re_[c == 0] - rf[c == 0]
        want = np.zeros_like(d)
        want[:, 0, 0] = -g[c == 0]
        want[:, 1, :] = -(g[c == 0, None] * tlwe.astype(np.uint32)[None, :])
    assert np.array_equal(d, want)
    _free(be)


def test_three_load_paths_agree_with_each_other_and_the_oracle():
    import oracle_lib as ol
    for name in ("default128", "redsec_small_v2"):
        be = _backend(name)
        sk, ck = keygen.generate_compressed(be, noise_seed=NOISE_SEED, mask_seed=MASK_SEED, load=False)
        host = ck.numpy()
        rng = np.random.default_rng(2)
        a, b = rng.integers(0, 2, 8), rng.integers(0, 2, 8)
        ca, cb = sk.encrypt_bits(a, seed=5), sk.encrypt_bits(b, seed=6)
        mu = ol.to_torus(1, 8)
        outs = []
        bk, ksk = be.expand_keys(ck.mask_seed, ck.bk_body, ck.ksk_body)
        for load in (lambda: be.load_compressed_keys(host.mask_seed, host.bk_body, host.ksk_body),
                     lambda: be.load_compressed_keys(ck.mask_seed, ck.bk_body, ck.ksk_body),
                     lambda: be.load_keys_dev(bk, ksk)):
            load()
            outs.append((be.bootstrap(_dev(ca), mu).cpu().numpy(), be.gate("NAND", _dev(ca), _dev(cb)).cpu().numpy()))
        for o in outs[1:]:
            assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]), name
        assert np.array_equal(ck.bk_body.cpu().numpy(), host.bk_body)            # the bodies were not modified

        class K:
            pass
        ks = K()
        ks.p, ks.bk, ks.ksk = ol.params(name), bk.cpu().numpy().ravel(), ksk.cpu().numpy().ravel()
        ctx = ol.Ctx(ks)
        assert np.array_equal(ctx.bootstrap_batch(ca, mu), outs[0][0])
        assert np.array_equal(ctx.gate_batch("NAND", ca, cb), outs[0][1])
        assert np.array_equal(sk.decrypt_bits(outs[0][1]), 1 - (a & b))
        ctx.close()
        del bk, ksk, ck
        _free(be)


GATE_TRUTH = {"NAND": lambda a, b: 1 - (a & b), "OR": lambda a, b: a | b, "AND": lambda a, b: a & b, "NOR": lambda a, b: 1 - (a | b),
              "XOR": lambda a, b: a ^ b, "XNOR": lambda a, b: 1 - (a ^ b), "ANDNY": lambda a, b: (1 - a) & b, "ANDYN": lambda a, b: a & (1 - b),
              "ORNY": lambda a, b: (1 - a) | b, "ORYN": lambda a, b: a | (1 - b)}


@pytest.mark.parametrize("name", SETS)
def test_compressed_key_from_host_bodies_end_to_end_at_full_size(name):
    """generate_compressed at full size, the bodies moved to the host and loaded from there (rs_load_compressed_keys); all ten
    gates, MUX and a 4-level programmable bootstrap decrypt correctly."""
    import torch
    be = _backend(name)
    sk, ck = keygen.generate_compressed(be, noise_seed=NOISE_SEED, mask_seed=MASK_SEED, load=False)
    host = ck.numpy()
    del ck
    torch.cuda.empty_cache()
    be.load_compressed_keys(host.mask_seed, host.bk_body, host.ksk_body)
    B = 256 if be.p.N == 1024 else 64
    rng = np.random.default_rng(17)
    a, b, c = (rng.integers(0, 2, B) for _ in range(3))
    ca, cb, cc = (_dev(sk.encrypt_bits(x, seed=s)) for x, s in ((a, 1), (b, 2), (c, 3)))
    for op, f in GATE_TRUTH.items():
        got = sk.decrypt_bits(be.gate(op, ca, cb).cpu().numpy())
        assert np.array_equal(got, f(a, b)), (name, op, int(np.sum(got != f(a, b))))
    assert np.array_equal(sk.decrypt_bits(be.mux(ca, cb, cc).cpu().numpy()), np.where(a == 1, b, c))
    N = be.p.N
    m = rng.integers(0, 4, B)
    x = _dev(sk.encrypt_torus(client.modswitch_to_torus32(2 * m + 1, 16).astype(np.int64), seed=4))
    lut = np.zeros(N, np.int32)
    for level in range(4):
        lut[level * N // 4:(level + 1) * N // 4] = client.modswitch_to_torus32([2 * (3 - level) + 1], 16)[0]
    ph = sk.phase(be.bootstrap_lut(x, _dev(lut[None])).cpu().numpy()).view(np.uint32).astype(np.int64)
    assert np.array_equal(ph >> 29, 3 - m), (name, int(np.sum((ph >> 29) != 3 - m)))
    be.sync()
    _free(be)


def test_mnist_sign1024x1_classifies_alike_under_compressed_and_full_keys():
    import torch
    import plain_model as pm
    from redsec_amd import nets
    name = "redsec_small_v2"
    net = pm.load_net("sign1024x1")
    labels, pixels = pm.load_images()
    preds = []
    for compressed in (True, False):
        be = _backend(name)
        if compressed:
            sk, _ = keygen.generate_compressed(be, noise_seed=NOISE_SEED, mask_seed=MASK_SEED)
        else:
            sk, bk, ksk = keygen.generate(be, seed=NOISE_SEED)
            del bk, ksk
        torch.cuda.empty_cache()
        enc = nets.EncryptedMnist(be, net)
        got = []
        for i in (1, 3, 8):
            out = enc.run(torch.from_numpy(sk.encrypt_image(pixels[i], seed=100 + i)).cuda(), {})
            got.append(int(np.argmax(sk.decrypt_ints(out.cpu().numpy()))))
        preds.append(got)
        _free(be)
    assert preds[0] == preds[1], preds
    assert sum(int(p == labels[i]) for p, i in zip(preds[0], (1, 3, 8))) >= 2


def test_unmodified_reference_tools_with_a_compressed_cloud_key(tmp_path, monkeypatch):
    import plain_model as pm
    import refdrivers as rd
    if not rd.available():
        pytest.skip("oracle/_ref/refnets not shipped")
    cdir, netdir = rd.make_tree(str(tmp_path))
    monkeypatch.setenv("REDSEC_KEY_FORMAT", "compressed")
    r = rd.run("client_gen_secure_keyset.out", cdir)
    assert r.returncode == 0, r.stderr
    keys = {f: open(os.path.join(cdir, f), "rb").read(4) for f in os.listdir(cdir) if f.endswith(".key")}
    assert sorted(keys.values()) == [b"RSS1", b"RSZ1"], keys
    monkeypatch.delenv("REDSEC_KEY_FORMAT")
    labels, pixels = pm.load_images()
    _, lwe_key = rd.read_secret_key(os.path.join(cdir, "secret.key"))
    ok = 0
    for i in (1, 3, 8):
        rd.write_image_csv(os.path.join(cdir, "img.csv"), labels[i], pixels[i])
        assert rd.run("client_encrypt_image.out", cdir, "img.csv").returncode == 0
        r = rd.run("mnist_sign1024x1_enc.out", netdir)
        assert r.returncode == 0 and "Result ctxts loaded" in r.stdout, r.stdout + r.stderr
        logits_ct = rd.read_ciphertexts(os.path.join(cdir, "network_output.ctxt"), 350, 10)
        r = rd.run("client_decrypt_image.out", cdir, "MNIST")
        m = re.search(r"Classification Result: (\d)", r.stdout)
        assert r.returncode == 0 and m, r.stdout + r.stderr
        phase = (logits_ct[:, 350].astype(np.int64) - (logits_ct[:, :350].astype(np.int64) * lwe_key).sum(axis=1)) & 0xFFFFFFFF
        dec = ((phase + (1 << 19)) >> 20) & 0xFFF
        dec = np.where(dec > 2048, dec - 4096, dec)
        assert int(np.argmax(dec)) == int(m.group(1))
        ok += int(int(m.group(1)) == labels[i])
    assert ok >= 2


def test_invalid_arguments_and_failed_loads():
    import torch
    import oracle_lib as ol
    name = "redsec_small_v2"
    be = _backend(name)
    sk, ck = keygen.generate_compressed(be, noise_seed=NOISE_SEED, mask_seed=MASK_SEED)
    L, vp = be.L, C.c_void_p
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    lwe, tlwe = sk.lwe_key, sk.tlwe_key
    pb, pk = vp(ck.bk_body.data_ptr()), vp(ck.ksk_body.data_ptr())

    def kg(b=pb, k=pk, lw=lwe, tl=tlwe, ms=MASK_SEED, ns=NOISE_SEED):
        return L.rs_keygen_compressed_dev(be.h, b, k, None if lw is None else i32(lw), None if tl is None else i32(tl), ms, ns, 0.0, 0.0)
    assert kg(b=None) == -1 and kg(k=None) == -1 and kg(lw=None) == -1 and kg(tl=None) == -1 and kg(ms=None) == -1 and kg(ns=None) == -1
    assert kg(ns=MASK_SEED) == -1 and b"equal" in L.rs_last_error()
    assert kg(b=vp(ck.bk_body.data_ptr() + 4)) == -1
    bad = lwe.copy(); bad[3] = 2
    assert kg(lw=bad) == -1 and b"lwe_key" in L.rs_last_error()
    bad = tlwe.copy(); bad[7] = -1
    assert kg(tl=bad) == -1 and b"tlwe_key" in L.rs_last_error()
    full_bk, full_ksk = be.empty(*be._key_sizes()[:1]), be.empty(*be._key_sizes()[1:])
    pfb, pfk = vp(full_bk.data_ptr()), vp(full_ksk.data_ptr())
    assert L.rs_expand_keys_dev(be.h, vp(full_bk.data_ptr() + 4), pfk, MASK_SEED, pb, pk) == -1
    for args in ((None, pfk, MASK_SEED, pb, pk), (pfb, None, MASK_SEED, pb, pk), (pfb, pfk, None, pb, pk), (pfb, pfk, MASK_SEED, None, pk),
                 (pfb, pfk, MASK_SEED, pb, None)):
        assert L.rs_expand_keys_dev(be.h, *args) == -1
    # a failed load leaves no key; the next load succeeds
    ct = _dev(sk.encrypt_bits(np.arange(16) & 1, seed=9))
    mu = ol.to_torus(1, 8)
    before = be.bootstrap(ct, mu).cpu().numpy()
    assert L.rs_load_compressed_keys_dev(be.h, MASK_SEED, pb, None) == -1
    with pytest.raises(Exception):
        be.bootstrap(ct, mu)
    host = ck.numpy()
    assert L.rs_load_compressed_keys(be.h, None, i32(host.bk_body), i32(host.ksk_body)) == -1
    be.load_compressed_keys(MASK_SEED, host.bk_body, host.ksk_body)
    assert np.array_equal(be.bootstrap(ct, mu).cpu().numpy(), before)
    del full_bk, full_ksk, ck
    torch.cuda.empty_cache()
    _free(be)
