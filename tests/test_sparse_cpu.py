"""Sparse bootstraps without a GPU (include/redsec_hip.h rs_bootstrap_sparse_dev): the kernels' own row
functions and the host validation of csrc/rs_sparse.h (compiled into the lane emulator) against the numpy restatement
(tests/sparse_ref.py), the trivial result against the CPU oracle's bootstrap of trivial samples, nets.dead_outputs on the bundled
binarynet weights, and the exports. Nothing here bootstraps on the library's side: there is no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import sparse_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i32p = C.POINTER(C.c_int32)
MU_SIGN = 1 << 20


@pytest.fixture(scope="module")
def emu():
    from redsec_amd import build
    L = C.CDLL(build.build_emulator())
    L.rs_emu_sparse_trivial.argtypes = [C.c_int32, C.c_int32, C.c_int]
    L.rs_emu_sparse_trivial.restype = C.c_int32
    L.rs_emu_sparse_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]
    L.rs_emu_sparse_gather.argtypes = [_i32p, _i32p, C.c_long, C.c_long, C.c_int, _i32p]
    L.rs_emu_sparse_fill.argtypes = [_i32p, _i32p, C.c_long, C.c_int, C.c_int32, C.c_int]
    L.rs_emu_sparse_scatter.argtypes = [_i32p, _i32p, _i32p, C.c_long, C.c_long, C.c_int]
    return L


def _p(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_i32p)


def _live_list(rng, B):
    """rows scattered through the batch with row 0 and row B - 1, a repeated entry, and entries outside [0, B) on both sides"""
    live = list(rng.choice(B, size=max(1, B // 3), replace=False)) + [0, B - 1, B - 1]
    live += [-1, B, B + 5, 2**31 - 1, -2**31]
    return np.array(rng.permutation(live), np.int64).astype(np.int32)


# ---- the row functions ----
@pytest.mark.parametrize("W", [5, 64, 65, 351])
def test_row_functions_equal_the_numpy_restatement(emu, W):
    """Random words; W below, at and just past one lane step, and REDsec's 351 (five steps and a partial one). The live list holds
    out-of-range and repeated entries; the fill runs out of place and with out == in."""
    rng = np.random.default_rng(W)
    B, N, logn, mu = 37, 1024, 10, MU_SIGN
    inp = rng.integers(-2**31, 2**31, (B, W)).astype(np.int32)
    directed = sr.directed_b(N)
    inp[:len(directed), -1] = directed
    live = _live_list(rng, B)
    n_live = len(live)
    assert n_live <= B
    # gather
    rows = np.full((n_live, W), 0x5a5a5a5a, np.int32)
    assert emu.rs_emu_sparse_gather(_p(inp), _p(live), n_live, B, W, _p(rows)) == 0
    assert np.array_equal(rows, sr.gather(inp, live))
    # fill, out of place: every word of every row is written
    out = np.full((B, W), 0x5a5a5a5a, np.int32)
    keep = inp.copy()
    assert emu.rs_emu_sparse_fill(_p(inp), _p(out), B, W, mu, logn) == 0
    want = sr.fill(keep, mu, N)
    assert np.array_equal(out, want) and np.array_equal(inp, keep)
    assert not out[:, :-1].any() and set(np.unique(out[:, -1])) == {mu, -mu}
    # fill in place
    same = keep.copy()
    assert emu.rs_emu_sparse_fill(_p(same), _p(same), B, W, mu, logn) == 0
    assert np.array_equal(same, want)
    # scatter over the filled rows: unlisted rows keep the fill, ignored entries write nothing
    boot = rng.integers(-2**31, 2**31, (n_live, W)).astype(np.int32)
    assert emu.rs_emu_sparse_scatter(_p(out), _p(boot), _p(live), n_live, B, W) == 0
    assert np.array_equal(out, sr.scatter(want, boot, live))
    listed = np.zeros(B, bool)
    listed[live[(live >= 0) & (live < B)]] = True
    assert np.array_equal(out[~listed], want[~listed]) and (~listed).any()


def test_an_empty_and_an_identity_live_list(emu):
    rng = np.random.default_rng(2)
    B, W = 7, 65
    inp = rng.integers(-2**31, 2**31, (B, W)).astype(np.int32)
    rows = np.zeros((B, W), np.int32)
    ident = np.arange(B, dtype=np.int32)
    assert emu.rs_emu_sparse_gather(_p(inp), _p(ident), B, B, W, _p(rows)) == 0 and np.array_equal(rows, inp)
    assert emu.rs_emu_sparse_gather(_p(inp), None, 0, B, W, _p(rows)) == 0
    out = np.zeros((B, W), np.int32)
    assert emu.rs_emu_sparse_scatter(_p(out), _p(inp), _p(ident), B, B, W) == 0 and np.array_equal(out, inp)
    assert emu.rs_emu_sparse_scatter(_p(out), _p(rows), None, 0, B, W) == 0 and np.array_equal(out, inp)


# ---- the trivial result against the oracle ----
def _synthetic_ctx(name, seed, n=None):
    p = ol.params(name)
    if n is not None:
        p.n = n

    class K:
        pass
    ks = K()
    ks.p = p
    ks.bk = ol.synthetic_key_words(seed, p.n * 2 * p.bk_l * 2 * p.N)
    ks.ksk = ol.synthetic_key_words(seed ^ 0x6b73, p.N * p.ks_t * (1 << p.ks_basebit) * (p.n + 1))
    return p, ol.Ctx(ks)


@pytest.mark.parametrize("name,n", [("default128", None), ("redsec_medium", 10)])
def test_trivial_samples_bootstrap_to_the_trivial_result_on_the_oracle(emu, name, n):
    """ro_bootstrap of (0, ..., 0, b) over the directed b words on a synthetic key (pseudo-random words: any key word that took part
    would show): exactly (0, ..., 0, +-mu), and the emulator's fill gives the same words. default-128 at its full size, and
    redsec_params_medium's ring N = 4096 (LWE dimension cut to 10 so that the keyswitch key stays small)."""
    p, ctx = _synthetic_ctx(name, 0x5ba75e, n)
    logn = p.N.bit_length() - 1
    b = sr.directed_b(p.N)
    x = sr.trivial_rows(b, p.n)
    for mu in (1 << 29, MU_SIGN, -(1 << 28), 12345):
        ref = ctx.bootstrap_batch(x, mu)
        assert not ref[:, :-1].any()
        assert set(np.unique(ref[:, -1])) == {mu, -mu}
        got = np.full_like(x, 0x5a5a5a5a)
        assert emu.rs_emu_sparse_fill(_p(x), _p(got), len(b), p.n + 1, mu, logn) == 0
        assert np.array_equal(got, ref), mu
        assert np.array_equal(sr.fill(x, mu, p.N), ref)
        assert [emu.rs_emu_sparse_trivial(int(v), mu, logn) for v in b] == ref[:, -1].tolist()
    ctx.close()


# ---- dead outputs of the bundled binarynet ----
def test_dead_outputs_of_the_bundled_binarynet():
    """conv6 of nets/cifar/binarynet: 356 of its 512 output channels (89 of every 128) have only zero weights. Over the 8 x 8
    positions of conv6 and the 4 x 4 of maxpool6 that is 22,784 of 32,768 and 5,696 of 8,192 rows: the trivial_inputs counts the
    benchmark's sign_agreement leg reports for these stages."""
    import plain_model as pm
    from redsec_amd import nets
    net = pm.CifarNet("binarynet")
    dead = [nets.dead_outputs(zero) for _, zero, _ in net.convs]
    assert [d.shape for d in dead] == [(128,), (128,), (256,), (256,), (512,), (512,)] and all(d.dtype == bool for d in dead)
    assert [int(d.sum()) for d in dead] == [0, 0, 0, 0, 0, 356] and 356 * 128 == 89 * 512
    conv6, pool6 = nets.live_rows(dead[5], 8 * 8), nets.live_rows(dead[5], 4 * 4)
    assert conv6.dtype == np.int32 and len(conv6) == 32768 - 22784 and len(pool6) == 8192 - 5696
    assert np.array_equal(conv6 % 512, np.tile(np.flatnonzero(~dead[5]), 64)) and (np.diff(conv6) > 0).all()
    assert nets.live_rows(dead[0], 32 * 32) is None
    # an FC layer: [K][M] -> [M]
    fc = [nets.dead_outputs(zero) for _, zero, _ in net.fcs]
    assert [d.shape for d in fc] == [(1024,), (1024,), (10,)] and [int(d.sum()) for d in fc] == [1, 0, 0]
    # a channel with one live tap is live
    z = np.ones((3, 3, 2, 3), np.uint8)
    z[1, 2, 1, 2] = 0
    assert nets.dead_outputs(z).tolist() == [True, True, False]


class _StubBackend:
    device = 0
    W = 3


def test_live_lists_are_built_once_per_stage(monkeypatch):
    """EncryptedCifar(skip_dead=True): one list per conv, fused max-pool and FC sign stage with a dead output, rows (h, w, c) of the
    live channels; none without skip_dead; maxpool="chain" is refused together with it."""
    import torch
    from redsec_amd import nets
    monkeypatch.setattr(torch, "from_numpy", lambda a: _Host(a))
    rng = np.random.default_rng(4)

    class Net:
        pass
    net = Net()
    net.bias0 = np.zeros(3, np.int32)
    net.convs, cin = [], 3
    for li in range(6):
        zero = rng.integers(0, 2, (3, 3, cin, 4)).astype(np.uint8)
        if li in (1, 4, 5):
            zero[..., [1, 3]] = 1
        net.convs.append((np.ones_like(zero), zero, np.zeros(4, np.int32)))
        cin = 4
    net.fcs, k = [], 64
    for m in (8, 8, 10):
        zero = rng.integers(0, 2, (k, m)).astype(np.uint8)
        net.fcs.append((np.ones_like(zero), zero, np.zeros(m, np.int32)))
        k = m
    net.fcs[0][1][:, [2, 5]] = 1
    net.fcs[2][1][:, 0] = 1                      # the logits layer is not bootstrapped: no list
    enc = nets.EncryptedCifar(_StubBackend(), net, skip_dead=True)
    assert sorted(enc.live) == ["conv2", "conv5", "conv6", "fc1", "maxpool2", "maxpool6"]
    sizes = {"conv2": 32 * 32, "maxpool2": 16 * 16, "conv5": 8 * 8, "conv6": 8 * 8, "maxpool6": 4 * 4}
    for name, positions in sizes.items():
        rows = enc.live[name].a
        assert rows.dtype == np.int32 and np.array_equal(rows, np.flatnonzero(np.tile([True, False, True, False], positions)))
    assert enc.live["fc1"].a.tolist() == [0, 1, 3, 4, 6, 7]
    assert nets.EncryptedCifar(_StubBackend(), net).live == {}
    with pytest.raises(ValueError):
        nets.EncryptedCifar(_StubBackend(), net, maxpool="chain", skip_dead=True)


class _Host:
    def __init__(self, a):
        self.a = a

    def to(self, dev):
        return self


# ---- validation ----
def test_validation_refuses_what_rs_bootstrap_sparse_dev_refuses(emu):
    ptr = C.c_void_p(64)           # only compared with null
    chk = emu.rs_emu_sparse_check
    W = 631
    assert chk(ptr, ptr, ptr, 10, 3, W) == 0 and chk(ptr, ptr, ptr, 10, 10, W) == 0
    assert chk(ptr, ptr, None, 10, 0, W) == 0                                   # no list is needed for no live row
    assert chk(None, None, None, 0, 0, W) == 0                                  # B = 0: a no-op
    assert chk(ptr, ptr, ptr, 0, 1, W) == -1 and chk(ptr, ptr, ptr, 10, 11, W) == -1      # n_live > B
    assert chk(None, ptr, ptr, 10, 3, W) == -1 and chk(ptr, None, ptr, 10, 3, W) == -1    # null out, null in
    assert chk(ptr, ptr, None, 10, 1, W) == -1                                  # null live with n_live > 0
    # row arithmetic: B rows of W words, and twice n_live <= B staged rows, in bytes, fit a signed 64-bit number
    limit = (2**63 - 1) // 8
    assert chk(ptr, ptr, ptr, limit // W, 1, W) == 0 and chk(ptr, ptr, ptr, limit // W + 1, 1, W) == -1
    assert chk(ptr, ptr, ptr, 2**61, 0, W) == -1 and chk(ptr, ptr, ptr, 2**64 - 1, 2**64 - 1, W) == -1
    assert chk(ptr, ptr, ptr, 2**31 + 5, 2**31 + 5, W) == 0                     # past int32 is fine: such rows can only be dead
    # the emulator's kernels refuse the same
    one = np.zeros((1, 5), np.int32)
    assert emu.rs_emu_sparse_gather(_p(one), None, 1, 1, 5, _p(one.copy())) == -1
    assert emu.rs_emu_sparse_gather(_p(one), _p(one), 2, 1, 5, _p(one.copy())) == -1
    assert emu.rs_emu_sparse_fill(_p(one), _p(one), 1, 5, 1, 9) == -1 and emu.rs_emu_sparse_fill(_p(one), _p(one), 1, 5, 1, 14) == -1


def test_no_cpu_fallback_for_the_sparse_call():
    """Without a device nothing computes and the reason is said: RS_ERR_NO_DEVICE. With one, a null context is an argument error."""
    import torch
    import redsec_amd
    L = redsec_amd.load_library()
    want = -1 if torch.cuda.is_available() else -2
    buf = np.full((3, 631), 7, np.int32)
    live = np.array([1], np.int32)
    assert L.rs_bootstrap_sparse_dev(None, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), 1 << 29, 3,
                                     live.ctypes.data_as(C.c_void_p), 1, None) == want
    if want == -2:
        assert b"no HIP device" in L.rs_last_error()
    assert (buf == 7).all()


# ---- exports ----
def test_the_sparse_call_is_exported_documented_and_in_an_object_of_its_own():
    import redsec_amd
    from redsec_amd import build, nets
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    assert "rs_bootstrap_sparse_dev" in redsec_amd.ABI_SYMBOLS and hasattr(redsec_amd.load_library(), "rs_bootstrap_sparse_dev")
    assert re.search(r"\bint rs_bootstrap_sparse_dev\(rs_ctx\* ctx, int32_t\* out, const int32_t\* in, int32_t mu, size_t B, "
                     r"const int32_t\* live, size_t n_live,\s+void\* stream\);", header)
    assert callable(redsec_amd.Backend.bootstrap_sparse) and callable(nets.dead_outputs)
    assert ("rs_sparse", "rs_sparse.hip", []) in build.HIP_OBJECTS
    assert "rs_sparse.h" in build.HIP_DEPS and "rs_sparse.h" in build.EMU_DEPS and "rs_sparse.hip" in build.HIP_SOURCES
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    for f in ("rs_sparse.hip", "rs_sparse.h"):
        code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, f)).read().splitlines())
        assert not re.search(r"\basm\b|__shared__|\batomic|\b(double|float)\b", code), f
    h = open(os.path.join(csrc, "rs_sparse.h")).read()
    assert "modswitch_2N(" in h and "rotated_const(" in h and "gen_rotated_const(" in h       # the kernels' own helpers
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "\n## 20. Sparse bootstraps (`rs_bootstrap_sparse_dev`)" in integ
    assert "an unlisted row is read at word n only" in " ".join(integ.lower().split())
