"""Seeded LWE ciphertexts on the device (rs_encrypt_seeded_dev, rs_expand_ciphertexts_dev): bodies and
full samples word for word against the numpy restatement on all five sets, the expansion of device bodies, stream ordering against
a gate on the same stream, MNIST from 784 uploaded bodies, the unmodified reference tools with an RSC1 image, and invalid input."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

SETS = ("default128", "redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large")
MASK_SEED = bytes(range(90, 122))
NOISE_SEED = bytes(range(11, 43))
KEY_SEED = bytes(range(7, 39))


def _backend(name, n=None):
    import redsec_amd
    return redsec_amd.Backend(redsec_amd.params(name, n=n), device=0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _free(*objs):
    import torch
    for o in objs:
        if hasattr(o, "close"):
            o.close()
    torch.cuda.empty_cache()


def _want_rows(lwe, mu, first, idx, stdev):
    """numpy bodies and full samples of the ciphertexts at positions idx of a call starting at row `first`."""
    n = len(lwe)
    body = np.empty(len(idx), np.int32)
    ct = np.empty((len(idx), n + 1), np.int32)
    for k, i in enumerate(idx):
        body[k] = keygen.encrypt_seeded(lwe, mu[i:i + 1], MASK_SEED, NOISE_SEED, first + int(i), stdev)[0]
        ct[k] = keygen.expand_ciphertexts(MASK_SEED, body[k:k + 1], n, first + int(i))[0]
    return body, ct


@pytest.mark.parametrize("name", SETS)
def test_device_encryption_and_expansion_equal_numpy(name):
    """B in {1, 37, 4097}, first in {0, 2^32 - 3, 2^64 - B}, stdev 0 and SECALPHA: the bodies, the optional full ct and the
    expansion of the device bodies equal numpy word for word (every row at N <= 2048, sampled rows for medium / large); the phase of
    the expansion minus mu is numpy's noise."""
    import torch
    be = _backend(name)
    n = be.p.n
    lwe, _ = keygen.secret_keys(name, KEY_SEED)
    rng = np.random.default_rng(n)
    for B in (1, 37, 4097):
        mu = rng.integers(-(1 << 31), 1 << 31, B, dtype=np.int64).astype(np.int32)
        d_mu = _dev(mu)
        for first in (0, (1 << 32) - 3, (1 << 64) - B):
            for stdev in (0.0, client.SECALPHA):
                body, ct = be.encrypt_seeded(lwe, d_mu, MASK_SEED, NOISE_SEED, first, stdev, full=True)
                body_only = be.encrypt_seeded(lwe, d_mu, MASK_SEED, NOISE_SEED, first, stdev)
                exp = be.expand_ciphertexts(MASK_SEED, body, first)
                torch.cuda.synchronize()
                hb, hc, he = body.cpu().numpy(), ct.cpu().numpy(), exp.cpu().numpy()
                assert np.array_equal(body_only.cpu().numpy(), hb)
                assert np.array_equal(hc, he)
                if n <= 630:
                    want_b = keygen.encrypt_seeded(lwe, mu, MASK_SEED, NOISE_SEED, first, stdev)
                    assert np.array_equal(hb, want_b), (name, B, first, stdev, np.flatnonzero(hb != want_b)[:4].tolist())
                    want_c = keygen.expand_ciphertexts(MASK_SEED, want_b, n, first)
                    assert np.array_equal(hc, want_c), (name, B, first, stdev)
                    noise = keygen.ct_noise(NOISE_SEED, first, B, stdev)
                else:
                    idx = np.unique(np.array([0, B // 2, B - 1] + ([1, 2, 1000, 4095] if B > 4000 else [])))
                    want_b, want_c = _want_rows(lwe, mu, first, idx, stdev)
                    assert np.array_equal(hb[idx], want_b), (name, B, first, stdev)
                    assert np.array_equal(hc[idx], want_c), (name, B, first, stdev)
                    he = he[idx]
                    noise = np.array([keygen.ct_noise(NOISE_SEED, first + int(i), 1, stdev)[0] for i in idx], np.int32)
                sk = client.SecretKeySet.from_secret(name, lwe, keygen.secret_keys(name, KEY_SEED)[1])
                m = mu if n <= 630 else mu[idx]
                ph = (sk.phase(he).astype(np.int64) - m) & 0xFFFFFFFF
                assert np.array_equal(ph.astype(np.uint32).view(np.int32), noise), (name, B, first, stdev)
                if stdev:
                    assert np.any(noise != 0)
                del body, ct, body_only, exp
    _free(be)


def test_stream_ordering_expand_then_gate_on_a_side_stream():
    """default-128, B = 2 #CUs + 1 (crosses a form boundary): bodies uploaded, expanded and NANDed on one non-default stream with no
    synchronisation in between; the gate outputs equal the CPU oracle's on the numpy expansion."""
    import torch
    import oracle_lib as ol
    name = "default128"
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * cus + 1
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 2, B), rng.integers(0, 2, B)
    sa = sk.encrypt_bits_seeded(a, mask_seed=MASK_SEED, noise_seed=NOISE_SEED, first=0)
    sb = sk.encrypt_bits_seeded(b, mask_seed=MASK_SEED, noise_seed=NOISE_SEED, first=B)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ba, bb = _dev(sa.body), _dev(sb.body)
        ca = be.expand_ciphertexts(MASK_SEED, ba, 0)
        cb = be.expand_ciphertexts(MASK_SEED, bb, B)
        out = be.gate("NAND", ca, cb)
    s.synchronize()
    got = out.cpu().numpy()

    class K:
        pass
    ks = K()
    ks.p, ks.bk, ks.ksk = ol.params(name), bk.cpu().numpy().ravel(), ksk.cpu().numpy().ravel()
    ctx = ol.Ctx(ks)
    ref = ctx.gate_batch("NAND", sa.expand(), sb.expand())
    ctx.close()
    assert np.array_equal(got, ref)
    assert np.array_equal(sk.decrypt_bits(got), 1 - (a & b))
    del bk, ksk, ca, cb, out
    _free(be)


def test_mnist_from_seeded_bodies_expanded_on_the_device():
    """sign1024x1 on real redsec_small_v2 keys: 784 bodies (4 bytes each) uploaded and expanded on the device give logits
    word-identical to the same image expanded in numpy and uploaded in full."""
    import torch
    import plain_model as pm
    from redsec_amd import nets
    name = "redsec_small_v2"
    net = pm.load_net("sign1024x1")
    labels, pixels = pm.load_images()
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    torch.cuda.empty_cache()
    enc = nets.EncryptedMnist(be, net)
    ok = 0
    for i in (1, 3):
        sc = sk.encrypt_image_seeded(pixels[i], mask_seed=MASK_SEED, noise_seed=NOISE_SEED, first=784 * i)
        d_body = _dev(sc.body)
        assert d_body.numel() * d_body.element_size() == 784 * 4 and sc.expand().nbytes == 784 * 351 * 4
        seeded = enc.run(be.expand_ciphertexts(MASK_SEED, d_body, sc.first), {}).cpu().numpy()
        full = enc.run(_dev(sc.expand()), {}).cpu().numpy()
        assert np.array_equal(seeded, full), i
        ok += int(sk.classify(seeded) == labels[i])
    assert ok >= 1
    _free(be)


def test_unmodified_reference_tools_with_a_seeded_image(tmp_path, monkeypatch):
    """client_encrypt_image under REDSEC_CT_FORMAT=seeded writes RSC1; mnist_sign1024x1_enc reads it. Its output's a and b words
    equal those it writes from a TFHE-format image.ctxt holding the numpy expansion of the same RSC1 file; the class matches."""
    import plain_model as pm
    import refdrivers as rd
    if not rd.available():
        pytest.skip("oracle/_ref/refnets not shipped")
    cdir, netdir = rd.make_tree(str(tmp_path))
    r = rd.run("client_gen_secure_keyset.out", cdir)
    assert r.returncode == 0, r.stderr
    labels, pixels = pm.load_images()
    _, lwe_key = rd.read_secret_key(os.path.join(cdir, "secret.key"))
    i = 3
    rd.write_image_csv(os.path.join(cdir, "img.csv"), labels[i], pixels[i])
    monkeypatch.setenv("REDSEC_CT_FORMAT", "seeded")
    assert rd.run("client_encrypt_image.out", cdir, "img.csv").returncode == 0
    monkeypatch.delenv("REDSEC_CT_FORMAT")
    image = os.path.join(cdir, "image.ctxt")
    raw = open(image, "rb").read()
    assert raw[:4] == b"RSC1" and len(raw) == client._RS_HEADER.itemsize + 40 + 784 * 4
    sc = client.read_seeded_ciphertexts(open(image, "rb"), n=350)
    outs = []
    for form in ("seeded", "tfhe"):
        if form == "tfhe":
            with open(image, "wb") as f:
                client.write_ciphertexts(f, sc.expand())
        r = rd.run("mnist_sign1024x1_enc.out", netdir)
        assert r.returncode == 0 and "Result ctxts loaded" in r.stdout, r.stdout + r.stderr
        outs.append(rd.read_ciphertexts(os.path.join(cdir, "network_output.ctxt"), 350, 10))
        r = rd.run("client_decrypt_image.out", cdir, "MNIST")
        m = re.search(r"Classification Result: (\d)", r.stdout)
        assert r.returncode == 0 and m, r.stdout + r.stderr
        outs.append(int(m.group(1)))
    assert np.array_equal(outs[0], outs[2]), "the a and b words of the two runs differ"
    assert outs[1] == outs[3]
    sk = client.SecretKeySet.from_secret("redsec_small_v2", lwe_key, np.zeros(1024, np.int32))
    assert sk.classify(outs[0]) == outs[1]


def test_invalid_arguments_zero_batch_and_the_secret_copy_is_freed():
    import torch
    name = "redsec_small_v2"
    be = _backend(name)
    n = be.p.n
    lwe, _ = keygen.secret_keys(name, KEY_SEED)
    L, vp = be.L, C.c_void_p
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    B = 64
    mu = _dev(np.arange(B) << 20)
    body, ct = be.empty(B), be.empty(B, n + 1)
    pb, pc, pm = vp(body.data_ptr()), vp(ct.data_ptr()), vp(mu.data_ptr())
    torch.cuda.synchronize()

    def enc(b=pb, c=pc, m=pm, count=B, lw=lwe, ms=MASK_SEED, ns=NOISE_SEED, first=0, sd=client.SECALPHA):
        return L.rs_encrypt_seeded_dev(be.h, b, c, m, count, None if lw is None else i32(lw), ms, ns, first, sd)

    def exp(c=pc, ms=MASK_SEED, first=0, b=pb, count=B):
        return L.rs_expand_ciphertexts_dev(be.h, c, ms, first, b, count, None)
    assert enc(b=None) == -1 and enc(m=None) == -1 and enc(lw=None) == -1 and enc(ms=None) == -1 and enc(ns=None) == -1
    assert enc(ns=MASK_SEED) == -1 and b"equal" in L.rs_last_error()
    bad = lwe.copy(); bad[5] = 3
    assert enc(lw=bad) == -1 and b"lwe_key" in L.rs_last_error()
    for sd in (-1e-3, float("nan"), float("inf")):
        assert enc(sd=sd) == -1
    assert enc(first=(1 << 64) - B + 1) == -1 and b"2^64" in L.rs_last_error()
    assert exp(first=(1 << 64) - 1, count=2) == -1
    assert exp(c=None) == -1 and exp(ms=None) == -1 and exp(b=None) == -1
    # B = 0 is a no-op, the context stays usable
    ct.fill_(7)
    assert enc(count=0) == 0 and exp(count=0) == 0 and exp(count=0, first=(1 << 64) - 1) == 0
    torch.cuda.synchronize()
    assert bool((ct == 7).all())
    assert enc(first=(1 << 64) - B) == 0 and enc(c=None) == 0
    torch.cuda.synchronize()
    want = keygen.encrypt_seeded(lwe, np.arange(B) << 20, MASK_SEED, NOISE_SEED, 0, client.SECALPHA)
    assert np.array_equal(body.cpu().numpy(), want)
    # the secret's device copy is freed: device memory returns to within 1 MB after many encryptions
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(50):
        assert enc() == 0
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free0 - free1) <= 1 << 20, (free0, free1)
    del body, ct, mu
    _free(be)
