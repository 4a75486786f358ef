"""GPU parity of the sparse bootstraps (include/redsec_hip.h rs_bootstrap_sparse_dev): every word equal
to the dense call rs_bootstrap_dev on the same batch, and sampled rows equal to the CPU oracle. default-128 at its full size on a
synthetic key (generated on the device; the oracle restates the generator), one case on redsec_params_medium's ring, and the
networks with skip_dead=True against skip_dead=False. Oracle results are computed once and shared by the arithmetic modes."""
import numpy as np
import pytest

import oracle_lib as ol
import sparse_ref as sr

pytestmark = pytest.mark.gpu

SEED = 0x5ba75e
E8 = 1 << 29
MU_SIGN = 1 << 20
_STATE = {}
_REF = {}


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()


@pytest.fixture(scope="module")
def be():
    import torch
    import redsec_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    b = redsec_amd.Backend(redsec_amd.params("default128"), device=0)
    b.load_synthetic_keys(SEED)
    yield b
    b.close()
    if "ctx" in _STATE:
        _STATE.pop("ctx").close()
    _REF.clear()


def _oracle():
    """the oracle on the same synthetic key words, built on first use"""
    if "ctx" not in _STATE:
        p = ol.params("default128")

        class K:
            pass
        ks = K()
        ks.p = p
        ks.bk = ol.synthetic_key_words(SEED, p.n * 2 * p.bk_l * 2 * p.N)
        ks.ksk = ol.synthetic_key_words(SEED ^ 0x6b73, p.N * p.ks_t * (1 << p.ks_basebit) * (p.n + 1))
        _STATE["ctx"] = ol.Ctx(ks)
    return _STATE["ctx"]


def _batch(B, live, seed, N=1024, n=630):
    """B rows: random words at the live rows, trivial samples that cycle through the directed b words everywhere else"""
    rng = np.random.default_rng(seed)
    b = sr.directed_b(N)
    x = sr.trivial_rows(np.resize(b, B), n)
    x[live] = rng.integers(-2**31, 2**31, (len(live), n + 1)).astype(np.int32)
    return x


def _scattered(B, count, seed):
    """`count` distinct rows scattered through [0, B), row 0 and row B - 1 among them, in no particular order"""
    rng = np.random.default_rng(seed)
    rows = np.r_[0, B - 1, 1 + rng.choice(B - 2, size=count - 2, replace=False)]
    return rng.permutation(rows).astype(np.int32)


# ---- the mixed batch ----
@pytest.mark.parametrize("mode", ["fft", "exact", "split"])
def test_mixed_batch_equals_the_dense_call_and_the_oracle(be, mode):
    """B = 2 #CUs + 3 with 13 live rows scattered through it (row 0 and row B - 1 among them); the dead rows are trivial samples
    over the directed b words. Every word equals rs_bootstrap_dev on the whole batch; every live row and eight dead rows equal
    ro_bootstrap."""
    import torch
    cus = be.info()["num_cus"]
    B = 2 * cus + 3
    live = _scattered(B, 13, 1)
    x = _batch(B, live, 2)
    dead8 = np.setdiff1d(np.arange(B), live)[[0, 1, 2, 7, 11, 19, 23, 28]]
    be.set_mode(mode)
    try:
        d = _dev(x)
        dense = be.bootstrap(d, E8)
        got = be.bootstrap_sparse(d, E8, _dev(live))
        assert torch.equal(got, dense)
        assert torch.equal(d, _dev(x))                       # the input is not written
    finally:
        be.set_mode("fft")
    got = got.cpu().numpy()
    sample = np.r_[live, dead8]
    if "mixed" not in _REF:
        _REF["mixed"] = _oracle().bootstrap_batch(x[sample], E8)
    assert np.array_equal(got[sample], _REF["mixed"])
    dead = np.setdiff1d(np.arange(B), live)
    assert np.array_equal(got[dead], sr.fill(x[dead], E8, 1024)) and {E8, -E8} == set(np.unique(got[dead, -1]))


def test_launch_form_is_that_of_the_compact_batch(be):
    cus = be.info()["num_cus"]
    B = 2 * cus + 3
    live = _scattered(B, 13, 3)
    d = _dev(_batch(B, live, 4))
    be.bootstrap(d, E8)
    form_B = be.last_launch()
    be.bootstrap(d[:13], E8)
    form_13 = be.last_launch()
    assert form_13 != form_B
    be.bootstrap(d, E8)
    be.bootstrap_sparse(d, E8, _dev(live))
    assert be.last_launch() == form_13


# ---- edge sizes, each against the dense call ----
def test_no_live_row_launches_no_rotation(be):
    import torch
    import redsec_amd
    B = 70
    x = _batch(B, np.zeros(0, np.int64), 5)
    d = _dev(x)
    dense = be.bootstrap(d, MU_SIGN)
    assert be.last_launch()["form"]                           # a rotation is on record ...
    got = be.bootstrap_sparse(d, MU_SIGN, torch.empty(0, dtype=torch.int32, device="cuda"))
    assert torch.equal(got, dense)
    with pytest.raises(redsec_amd.RedsecHipError, match="no blind rotation launched"):
        be.last_launch()                                      # ... and the sparse call without live rows launched none
    assert np.array_equal(got.cpu().numpy(), sr.fill(x, MU_SIGN, 1024))


def test_identity_list_gives_the_dense_words(be):
    import torch
    B = 37
    x = _batch(B, np.arange(0, B, 2), 6)
    d = _dev(x)
    assert torch.equal(be.bootstrap_sparse(d, E8, _dev(np.arange(B))), be.bootstrap(d, E8))


def test_compact_batch_crosses_a_form_boundary(be):
    """#CUs + 1 live rows inside B = 8 #CUs + 3: the dense call takes the throughput form, the compact batch another one."""
    import torch
    cus = be.info()["num_cus"]
    B, n_live = 8 * cus + 3, cus + 1
    live = _scattered(B, n_live, 7)
    d = _dev(_batch(B, live, 8))
    be.bootstrap(d[:n_live], E8)
    form_live = be.last_launch()
    dense = be.bootstrap(d, E8)
    form_B = be.last_launch()
    assert form_B != form_live
    got = be.bootstrap_sparse(d, E8, _dev(live))
    assert be.last_launch() == form_live
    assert torch.equal(got, dense)


def test_in_place_and_unusual_entries(be):
    """out == in; and a list with a repeated entry and entries outside [0, B), which the device ignores."""
    import torch
    B = 45
    live = _scattered(B, 9, 9)
    x = _batch(B, live, 10)
    dense = be.bootstrap(_dev(x), MU_SIGN)
    d = _dev(x)
    assert be.bootstrap_sparse(d, MU_SIGN, _dev(live), out=d) is d
    assert torch.equal(d, dense)
    odd = np.r_[live[:4], -1, B, live[4:], live[2], 2**31 - 1, -2**31, B + 64].astype(np.int64).astype(np.int32)
    guard = _dev(np.full((B + 2, x.shape[1]), 0x5a5a5a5a, np.int32))     # the rows around the batch stay as they are
    out = guard[1:B + 1]
    be.bootstrap_sparse(_dev(x), MU_SIGN, _dev(odd), out=out)
    assert torch.equal(out, dense)
    assert bool((guard[0] == 0x5a5a5a5a).all()) and bool((guard[B + 1] == 0x5a5a5a5a).all())


def test_empty_batch_and_refused_arguments(be):
    import torch
    import redsec_amd
    empty = torch.empty(0, be.W, dtype=torch.int32, device="cuda")
    none = torch.empty(0, dtype=torch.int32, device="cuda")
    assert tuple(be.bootstrap_sparse(empty, E8, none).shape) == (0, be.W)
    d = _dev(_batch(4, np.array([1]), 11))
    with pytest.raises(redsec_amd.RedsecHipError, match="error -1"):
        be.bootstrap_sparse(empty, E8, _dev(np.array([0])))                    # n_live > B = 0
    with pytest.raises(redsec_amd.RedsecHipError, match="error -1"):
        be.bootstrap_sparse(d, E8, _dev(np.arange(5)))                         # n_live > B
    L, vp = be.L, lambda t: t.data_ptr()
    assert L.rs_bootstrap_sparse_dev(be.h, None, vp(d), E8, 4, vp(d), 1, None) == -1
    assert L.rs_bootstrap_sparse_dev(be.h, vp(d), None, E8, 4, vp(d), 1, None) == -1
    assert L.rs_bootstrap_sparse_dev(be.h, vp(d), vp(d), E8, 4, None, 1, None) == -1
    assert L.rs_bootstrap_sparse_dev(be.h, vp(d), vp(d), E8, 2**61, vp(d), 1, None) == -1
    be.sync()


# ---- a ring above 1024 ----
def test_redsec_medium_ring_on_a_synthetic_key():
    """redsec_params_medium (N = 4096, the general kernels) at its full size on a synthetic key: B = 8, 3 live rows."""
    import torch
    import redsec_amd
    p = redsec_amd.params("redsec_medium")
    b = redsec_amd.Backend(p, device=0)
    try:
        b.load_synthetic_keys(SEED + 1)
        mu = MU_SIGN
        live = np.array([6, 0, 3], np.int32)
        x = _batch(8, live, 12, N=p.N, n=p.n)
        d = _dev(x)
        dense = b.bootstrap(d, mu)
        got = b.bootstrap_sparse(d, mu, _dev(live))
        assert b.last_launch()["form"] == "general"
        assert torch.equal(got, dense)
        dead = np.setdiff1d(np.arange(8), live)
        assert np.array_equal(got.cpu().numpy()[dead], sr.fill(x[dead], mu, p.N))
    finally:
        b.close()
        torch.cuda.empty_cache()


# ---- the networks ----
class _Net:
    pass


def _cifar_net(rng):
    """EncryptedCifar's layout with 4 output channels per conv: channels 1 and 3 of conv2, conv5 and conv6 and two neurons of fc1
    are dead, the weights are otherwise random."""
    net = _Net()
    net.bias0 = rng.integers(-100, 100, 3).astype(np.int32)
    net.convs, cin = [], 3
    for li in range(6):
        zero = (rng.integers(0, 3, (3, 3, cin, 4)) == 0).astype(np.uint8)
        zero[0, 0, 0, :] = 0                               # every channel starts with a live tap ...
        if li in (1, 4, 5):
            zero[..., [1, 3]] = 1                          # ... except the dead ones
        net.convs.append((rng.integers(0, 2, zero.shape).astype(np.uint8), zero, rng.integers(-9, 9, 4).astype(np.int32)))
        cin = 4
    net.fcs, k = [], 4 * 4 * 4
    for m in (8, 8, 10):
        zero = (rng.integers(0, 3, (k, m)) == 0).astype(np.uint8)
        zero[0, :] = 0
        net.fcs.append((rng.integers(0, 2, zero.shape).astype(np.uint8), zero, rng.integers(-9, 9, m).astype(np.int32)))
        k = m
    net.fcs[0][1][:, [2, 5]] = 1
    return net


def test_synthetic_cifar_net_with_and_without_skip_dead(be):
    import torch
    from redsec_amd import nets
    rng = np.random.default_rng(21)
    net = _cifar_net(rng)
    image = _dev(rng.integers(-2**31, 2**31, (32 * 32 * 3, be.W)).astype(np.int32))
    dense_taps, sparse_taps = [], []
    dense = nets.EncryptedCifar(be, net).run(image, taps=dense_taps)
    enc = nets.EncryptedCifar(be, net, skip_dead=True)
    assert sorted(enc.live) == ["conv2", "conv5", "conv6", "fc1", "maxpool2", "maxpool6"]
    calls = []
    sparse_call = be.bootstrap_sparse
    be.bootstrap_sparse = lambda rows, mu, live, out=None: calls.append(int(live.numel())) or sparse_call(rows, mu, live, out)
    try:
        sparse = enc.run(image, taps=sparse_taps)
    finally:
        del be.bootstrap_sparse
    assert calls == [2048, 512, 128, 128, 32, 6]            # conv2, maxpool2, conv5, conv6, maxpool6, fc1: half the rows, 6 of 8
    assert torch.equal(sparse, dense) and tuple(sparse.shape) == (10, be.W)
    assert [t["name"] for t in sparse_taps] == [t["name"] for t in dense_taps] and len(dense_taps) == 12
    for a, b in zip(sparse_taps, dense_taps):
        assert (a["kind"], a["mu"]) == (b["kind"], b["mu"]) and torch.equal(a["out"], b["out"]), a["name"]
        assert torch.equal(a["inputs"][0], b["inputs"][0]), a["name"]
    # the dead rows really are trivial samples, and both signs occur among them
    conv6 = [t for t in sparse_taps if t["name"] == "conv6"][0]
    rows = conv6["out"].view(8 * 8, 4, be.W)[:, [1, 3]]
    assert not bool(rows[..., :-1].any()) and bool((rows[..., -1].abs() == (1 << 28)).all())


def test_mnist_sign1024x1_with_100_dead_neurons(be):
    import torch
    import plain_model as pm
    from redsec_amd import nets
    rng = np.random.default_rng(22)
    net = pm.load_net("sign1024x1")
    sign, zero, bias = net.fc[0]
    zero = zero.copy()
    dead = rng.choice(1024, size=100, replace=False)
    zero[:, dead] = 1
    net.fc[0] = (sign, zero, bias)
    image = _dev(rng.integers(-2**31, 2**31, (784, be.W)).astype(np.int32))
    dense_taps, sparse_taps = {}, {}
    dense = nets.EncryptedMnist(be, net).run(image, taps=dense_taps)
    enc = nets.EncryptedMnist(be, net, skip_dead=True)
    n_dead = int(nets.dead_outputs(zero).sum())
    assert n_dead >= 100 and enc.live[0].numel() == 1024 - n_dead
    sparse = enc.run(image, taps=sparse_taps)
    assert torch.equal(sparse, dense) and sorted(sparse_taps) == sorted(dense_taps) == ["bits0", "bits1", "pre0", "pre1"]
    for k in dense_taps:
        assert torch.equal(sparse_taps[k], dense_taps[k]), k
    bits = sparse_taps["bits1"][torch.from_numpy(np.sort(dead)).cuda()]
    assert not bool(bits[:, :-1].any()) and bool((bits[:, -1].abs() == MU_SIGN).all())
