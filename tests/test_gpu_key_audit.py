"""Device decryption and the exact noise audit of evaluation keys on the device (rs_phase_dev, rs_audit_keys_dev,
rs_audit_compressed_keys_dev): phases against numpy on all five sets, the audit of whole keys against the
numpy restatement and against the difference of a noisy and a noiseless key, the compressed audit against the audit of the expanded
key, every word of the full-size keys of the large rings, deterministic detection of corrupted words, and invalid input. Every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from redsec_amd import client, keygen

pytestmark = pytest.mark.gpu

SETS = ("default128", "redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large")
KEY_SEED = bytes(range(21, 53))
MASK_SEED = bytes(range(150, 182))
REPORT = ("bk_max_abs", "ksk_max_abs", "bk_over", "ksk_over", "ksk_zero_bad", "bk_words", "ksk_words")
BIG = (2.0 ** -20, 2.0 ** -15)       # deviations whose noise words are non-zero on every ring


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


def _words(p):
    return p.n * 2 * p.bk_l * p.N, p.N * p.ks_t * ((1 << p.ks_basebit) - 1)


def _np_phase(ct, key):
    dim = len(key)
    ct = np.asarray(ct, np.int32).reshape(-1, dim + 1)
    dot = (ct[:, :dim].view(np.uint32).astype(np.uint64) * np.asarray(key).astype(np.uint64)).sum(axis=-1)
    return ((ct[:, dim].view(np.uint32).astype(np.uint64) - dot) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("name", SETS)
def test_phase_equals_numpy(name):
    """B in {1, 257, 4096} (and 65,536 for default-128) samples of random words under the LWE key of the full dimension: rs_phase_dev
    equals SecretKeySet.phase word for word; so does decryption through backend=."""
    be = _backend(name)
    n = be.p.n
    lwe, tlwe = keygen.secret_keys(name, KEY_SEED)
    sk = client.SecretKeySet.from_secret(name, lwe, tlwe)
    rng = np.random.default_rng(n)
    for B in (1, 257, 4096) + ((65536,) if name == "default128" else ()):
        ct = rng.integers(-(1 << 31), 1 << 31, (B, n + 1), dtype=np.int64).astype(np.int32)
        d_ct = _dev(ct)
        got = be.phase(d_ct, lwe).cpu().numpy()
        want = sk.phase(ct)
        assert np.array_equal(got, want), (name, B, np.flatnonzero(got != want)[:4].tolist())
        if B == 257:
            assert np.array_equal(sk.decrypt_bits(d_ct, backend=be), sk.decrypt_bits(ct))
            assert np.array_equal(sk.decrypt_ints(d_ct, backend=be), sk.decrypt_ints(ct))
        del d_ct
    _free(be)


@pytest.mark.parametrize("name", ["default128", "redsec_medium"])
def test_phase_of_bootstrap_outputs_with_the_ring_key_and_from_a_side_stream(name):
    """dim = N on the output of bootstrap_wo_ks against numpy with the ring key (the noise of a bootstrap, measured for the first
    time); a gate's output produced on a side stream and passed on without any synchronisation."""
    import torch
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    B = 300
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 2, B), rng.integers(0, 2, B)
    ca, cb = _dev(sk.encrypt_bits(a)), _dev(sk.encrypt_bits(b))
    x = be.lincomb(ca, -1, cb, -1, bconst=1 << 29)
    u = be.bootstrap_wo_ks(x, 1 << 29)
    got = be.phase(u, sk.tlwe_key).cpu().numpy()
    assert np.array_equal(got, _np_phase(u.cpu().numpy(), sk.tlwe_key))
    want = np.where(1 - (a & b), 1 << 29, -(1 << 29))
    assert np.abs(got.astype(np.int64) - want).max() < 1 << 27          # NAND, well inside its eighth of the torus
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = be.gate("NAND", ca, cb)
        for _ in range(3):                                              # more work behind it on the same side stream
            out = be.gate("NAND", out, cb)
    ph = be.phase(out, sk.lwe_key)                                      # no synchronisation of any kind in between
    s.synchronize()
    assert np.array_equal(ph.cpu().numpy(), sk.phase(out.cpu().numpy()))
    del bk, ksk, ca, cb, x, u, out, ph
    _free(be)


def _assert_report(got, want):
    assert {f: got[f] for f in REPORT} == {f: int(want[f]) for f in REPORT}


@pytest.mark.parametrize("name", ["default128", "redsec_small_v2"])
def test_full_audit_of_a_whole_noisy_key_equals_numpy(name):
    """Set deviations: the noise arrays and every report field equal keygen.audit of the downloaded key, under the default limits
    and under limits low enough that words exceed them."""
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED, load=False)
    hb, hk = bk.cpu().numpy().reshape(-1, 2, be.p.N), ksk.cpu().numpy().reshape(-1, be.p.n + 1)
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, ksk, noise=True)
    want = keygen.audit(name, sk.lwe_key, sk.tlwe_key, hb, hk)
    _assert_report(got, want)
    assert got["bk_over"] == got["ksk_over"] == got["ksk_zero_bad"] == 0 and got["bk_max_abs"] > 0 and got["ksk_max_abs"] > 0
    assert (got["bk_words"], got["ksk_words"]) == _words(be.p)
    assert np.array_equal(got["bk_noise"].cpu().numpy().reshape(-1, be.p.N), want["bk_noise"])
    assert np.array_equal(got["ksk_noise"].cpu().numpy().ravel(), want["ksk_noise"])
    low = (want["bk_max_abs"] // 3, want["ksk_max_abs"] // 3)
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, ksk, limits=low)
    _assert_report(got, keygen.audit(name, sk.lwe_key, sk.tlwe_key, hb, hk, limits=low))
    assert got["bk_over"] > 0 and got["ksk_over"] > 0 and "bk_noise" not in got
    # one half at a time
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk=bk)
    assert (got["bk_max_abs"], got["bk_words"], got["ksk_words"], got["ksk_max_abs"]) == (want["bk_max_abs"], want["bk_words"], 0, 0)
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, ksk=ksk)
    assert (got["ksk_max_abs"], got["ksk_words"], got["bk_words"], got["bk_max_abs"]) == (want["ksk_max_abs"], want["ksk_words"], 0, 0)
    del bk, ksk
    _free(be)


@pytest.mark.parametrize("name", ["default128", "redsec_small_v2"])
def test_audited_noise_is_the_difference_of_the_noisy_and_the_noiseless_key(name):
    """Independent of numpy's libm: with one seed, (b of the noisy device key) - (b of the noiseless device key) is the audited
    noise word for word, bk and ksk; the noiseless key audits to all zeros."""
    import torch
    be = _backend(name)
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED, load=False)
    _, bk0, ksk0 = keygen.generate(be, seed=KEY_SEED, bk_stdev=0.0, ks_stdev=0.0, load=False)
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, ksk, noise=True)
    assert torch.equal(bk[:, :, 0], bk0[:, :, 0]) and torch.equal(ksk[..., :-1], ksk0[..., :-1])
    assert torch.equal(got["bk_noise"], bk[:, :, 1] - bk0[:, :, 1]) and bool(got["bk_noise"].any())
    assert torch.equal(got["ksk_noise"], ksk[..., -1] - ksk0[..., -1]) and bool(got["ksk_noise"].any())
    zero = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk0, ksk0, noise=True)
    assert not bool(zero["bk_noise"].any()) and not bool(zero["ksk_noise"].any())
    assert (zero["bk_max_abs"], zero["ksk_max_abs"], zero["bk_over"], zero["ksk_over"], zero["ksk_zero_bad"]) == (0, 0, 0, 0, 0)
    del bk, ksk, bk0, ksk0, got, zero
    _free(be)


@pytest.mark.parametrize("name", SETS)
def test_compressed_audit_equals_the_audit_of_the_expanded_key(name):
    """All five sets at full size, deviations that leave non-zero noise on every ring: the compressed audit (masks regenerated from
    the mask seed) equals the full audit of expand_keys of the same bodies, and the full audit of the key rs_keygen_dev writes from
    seed = the compressed key's noise seed (other masks, the same domain-4 / 6 noise words). Arrays compared on the device."""
    import torch
    be = _backend(name)
    sk, ck = keygen.generate_compressed(be, noise_seed=KEY_SEED, mask_seed=MASK_SEED, bk_stdev=BIG[0], ks_stdev=BIG[1], load=False)
    limits = (int(3 * BIG[0] * 2 ** 32), int(3 * BIG[1] * 2 ** 32))      # some words of an honest key exceed 3 sigma
    comp = be.audit_compressed_keys(sk.lwe_key, sk.tlwe_key, MASK_SEED, ck.bk_body, ck.ksk_body, limits=limits, noise=True)
    assert (comp["bk_words"], comp["ksk_words"]) == _words(be.p) and comp["bk_over"] > 0 and comp["ksk_zero_bad"] == 0
    assert 0 < comp["bk_max_abs"] < 8.58 * BIG[0] * 2 ** 32 and 0 < comp["ksk_max_abs"] < 8.58 * BIG[1] * 2 ** 32
    bk, ksk = be.expand_keys(MASK_SEED, ck.bk_body, ck.ksk_body)
    full = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, ksk, limits=limits, noise=True)
    _assert_report(comp, full)
    assert torch.equal(comp["bk_noise"], full["bk_noise"]) and torch.equal(comp["ksk_noise"], full["ksk_noise"])
    del full
    be.keygen(sk.lwe_key, sk.tlwe_key, KEY_SEED, BIG[0], BIG[1], bk=bk, ksk=ksk)
    other = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, ksk, limits=limits, noise=True)
    _assert_report(comp, other)
    assert torch.equal(comp["bk_noise"], other["bk_noise"]) and torch.equal(comp["ksk_noise"], other["ksk_noise"])
    del bk, ksk, other, comp, ck
    _free(be)


@pytest.mark.parametrize("name", ["redsec_medium", "redsec_large"])
def test_every_word_of_the_full_size_keys_of_the_large_rings(name):
    """The set's deviations truncate to zero noise words: every one of the n 2l N + N t (2^basebit - 1) noise words of the key
    rs_keygen_dev writes is 0 and every v = 0 sample is all zero. With larger deviations, sampled rows against numpy."""
    be = _backend(name)
    p = be.p
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED, load=False)
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, ksk)
    assert (got["bk_max_abs"], got["ksk_max_abs"], got["ksk_zero_bad"], got["bk_over"], got["ksk_over"]) == (0, 0, 0, 0, 0)
    assert (got["bk_words"], got["ksk_words"]) == _words(p)
    be.keygen(sk.lwe_key, sk.tlwe_key, KEY_SEED, BIG[0], BIG[1], bk=bk, ksk=ksk)
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, ksk, noise=True)
    base, rows_bk = 1 << p.ks_basebit, p.n * 2 * p.bk_l
    bk_rows = np.array([0, 1, p.bk_l, rows_bk // 2 + 2, rows_bk - 1])
    ksk_rows = np.array([0, 1, base * p.ks_t * 7 + base - 1, (p.N * p.ks_t - 1) * base, p.N * p.ks_t * base - 1])
    hb = bk.reshape(-1, 2, p.N)[_dev(bk_rows).long()].cpu().numpy()
    hk = ksk.reshape(-1, p.n + 1)[_dev(ksk_rows).long()].cpu().numpy()
    want = keygen.audit(name, sk.lwe_key, sk.tlwe_key, hb, hk, bk_rows=bk_rows, ksk_rows=ksk_rows)
    assert np.array_equal(got["bk_noise"].reshape(-1, p.N)[_dev(bk_rows).long()].cpu().numpy(), want["bk_noise"]) and want["bk_noise"].any()
    assert np.array_equal(got["ksk_noise"].ravel()[_dev(ksk_rows).long()].cpu().numpy(), want["ksk_noise"]) and want["ksk_noise"].any()
    assert 0 < got["bk_max_abs"] < 8.58 * BIG[0] * 2 ** 32 and 0 < got["ksk_max_abs"] < 8.58 * BIG[1] * 2 ** 32 and got["ksk_zero_bad"] == 0
    del bk, ksk, got
    _free(be)


def test_corrupted_words_and_a_wrong_secret_are_detected_exactly():
    import torch
    name = "default128"
    be = _backend(name)
    p = be.p
    n, N, l, Bgbit, base = p.n, p.N, p.bk_l, p.bk_Bgbit, 1 << p.ks_basebit
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED, load=False)
    clean = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, ksk, noise=True)
    # one body word + 2^20
    bad = bk.clone()
    bad[17, 4, 1, 300] += 1 << 20
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, bad, ksk, noise=True)
    diff = (got["bk_noise"] - clean["bk_noise"]).cpu().numpy()
    assert np.argwhere(diff).tolist() == [[17, 4, 300]] and diff[17, 4, 300] == 1 << 20
    assert got["bk_over"] == clean["bk_over"] + 1 == 1 and torch.equal(got["ksk_noise"], clean["ksk_noise"])
    del bad
    # a non-zero word in a v = 0 sample
    badk = ksk.clone()
    badk[9, 2, 0, 5] = 1
    got = be.audit_keys(sk.lwe_key, sk.tlwe_key, bk, badk, noise=True)
    assert got["ksk_zero_bad"] == 1 and torch.equal(got["ksk_noise"], clean["ksk_noise"]) and got["ksk_max_abs"] == clean["ksk_max_abs"]
    del badk
    # one bit of the LWE key flipped
    i = 123
    wrong = sk.lwe_key.copy()
    wrong[i] ^= 1
    ds = int(sk.lwe_key[i]) - int(wrong[i])                                 # s - s'
    got = be.audit_keys(wrong, sk.tlwe_key, bk, ksk, noise=True)
    diff = (got["bk_noise"] - clean["bk_noise"]).cpu().numpy().view(np.uint32)
    assert np.unique(np.argwhere(diff)[:, 0]).tolist() == [i]
    S = sk.tlwe_key.astype(np.int64)
    for c in (0, 1):
        for j in range(l):
            g = 1 << (32 - (j + 1) * Bgbit)
            want = np.zeros(N, np.int64)
            if c == 1:
                want[0] = ds * g
            else:
                want = -ds * g * S
            assert np.array_equal(diff[i, c * l + j], (want % (1 << 32)).astype(np.uint32)), (c, j)
    a_i = ksk[..., i].cpu().numpy().view(np.uint32).astype(np.int64)
    live = np.broadcast_to(np.arange(base) != 0, a_i.shape)
    dk = (got["ksk_noise"] - clean["ksk_noise"]).cpu().numpy().view(np.uint32)
    assert np.array_equal(dk, np.where(live, (ds * a_i) % (1 << 32), 0).astype(np.uint32))
    del bk, ksk, clean, got
    _free(be)


def test_invalid_arguments_zero_batch_the_secret_copy_is_freed_and_the_loaded_key_stays():
    import torch
    name = "redsec_small_v2"
    be = _backend(name)
    p = be.p
    n, N = p.n, p.N
    sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)                        # loaded
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 2, 200), rng.integers(0, 2, 200)
    ca, cb = _dev(sk.encrypt_bits(a)), _dev(sk.encrypt_bits(b))
    before = be.gate("NAND", ca, cb).cpu().numpy()
    L, vp = be.L, C.c_void_p
    i32 = lambda x: None if x is None else np.ascontiguousarray(x, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    B = 64
    ct = _dev(rng.integers(-(1 << 31), 1 << 31, (B, n + 1), dtype=np.int64))
    ph = be.empty(B)
    ph.fill_(7)
    torch.cuda.synchronize()
    pp, pc = vp(ph.data_ptr()), vp(ct.data_ptr())

    def phase(out=pp, c=pc, count=B, key=sk.lwe_key, dim=n):
        return L.rs_phase_dev(be.h, out, c, count, i32(key), dim)
    assert phase(out=None) == -1 and phase(c=None) == -1 and phase(key=None) == -1
    for dim in (0, -1, n - 1, n + 1, 2 * N):
        assert phase(dim=dim, key=np.zeros(2 * N, np.int32)) == -1 and b"dim" in L.rs_last_error()
    two = sk.lwe_key.copy(); two[n - 1] = 2
    assert phase(key=two) == -1 and b"not 0 or 1" in L.rs_last_error()
    assert phase(count=0) == 0
    torch.cuda.synchronize()
    assert bool((ph == 7).all())
    assert phase() == 0 and np.array_equal(ph.cpu().numpy(), sk.phase(ct.cpu().numpy()))
    assert phase(c=vp(be.empty(B, N + 1).fill_(0).data_ptr()), key=sk.tlwe_key, dim=N) == 0 and not bool(ph.any())

    import redsec_amd.backend as rb
    rep = rb.RsKeyAudit()
    pbk, pksk = vp(bk.data_ptr()), vp(ksk.data_ptr())

    def audit(r=C.byref(rep), k=pbk, s=pksk, lw=sk.lwe_key, tl=sk.tlwe_key):
        return L.rs_audit_keys_dev(be.h, r, None, None, k, s, i32(lw), i32(tl), 1, 1)
    assert audit(r=None) == -1 and audit(lw=None) == -1 and audit(tl=None) == -1
    assert audit(k=None, s=None) == -1 and b"both halves" in L.rs_last_error()
    assert audit(lw=two) == -1 and b"lwe_key" in L.rs_last_error()
    twoN = sk.tlwe_key.copy(); twoN[0] = -1
    assert audit(tl=twoN) == -1 and b"tlwe_key" in L.rs_last_error()
    assert L.rs_audit_compressed_keys_dev(be.h, C.byref(rep), None, None, None, pbk, pksk, i32(sk.lwe_key), i32(sk.tlwe_key), 1, 1) == -1
    assert L.rs_audit_compressed_keys_dev(be.h, C.byref(rep), None, None, MASK_SEED, None, None, i32(sk.lwe_key), i32(sk.tlwe_key), 1, 1) == -1
    assert audit() == 0 and rep.bk_over > 0 and rep.ksk_over > 0 and rep.ksk_zero_bad == 0          # limits of 1
    # the secrets' device copies are freed: device memory returns to within 1 MB after many calls
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        assert phase() == 0 and audit() == 0
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free0 - free1) <= 1 << 20, (free0, free1)
    # the key loaded before all this still evaluates the same words
    assert np.array_equal(be.gate("NAND", ca, cb).cpu().numpy(), before)
    assert np.array_equal(sk.decrypt_bits(before), 1 - (a & b))
    del bk, ksk, ca, cb, ct, ph
    _free(be)
