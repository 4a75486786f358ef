"""The wide throughput form of the keyswitch (csrc/rs_keyswitch_wide.hip: 1,024 ciphertexts x 32 words per workgroup, one barrier
per group of coefficients), forced at small batches with RS_KS_FORM=wide and held, word for word, to the oracle's lweKeySwitch
and to the tiled form (RS_KS_FORM=tiled).

Batch sizes: one lane, one lane short of a tile, a whole tile, one lane into the second tile, two tiles and a lane (more than
one workgroup per word column, a last workgroup with one live lane). Widths: W = 25 (one partial 32-word chunk) and W = 351 /
631 (11 / 20 chunks, the last partial). Inputs: random words, plus coefficients whose digits are all 0, all base - 1, and that
carry through the rounding offset into the top digit or wrap to zero."""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

BATCHES = [1, 1023, 1024, 1025, 2049]
_CACHE = {}


@contextlib.contextmanager
def _forced(form):
    old = os.environ.get("RS_KS_FORM")
    os.environ["RS_KS_FORM"] = form          # read once, in rs_create
    try:
        yield
    finally:
        if old is None:
            del os.environ["RS_KS_FORM"]
        else:
            os.environ["RS_KS_FORM"] = old


def _backend(p, name, form, ks):
    import redsec_amd
    with _forced(form):
        be = redsec_amd.Backend(redsec_amd.params(name, n=p.n), device=0)
    be.load_keys(ks.bk, ks.ksk)
    return be


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()


def _samples(p, B, seed):
    """[B][N + 1] extracted samples: random words with the directed coefficients strewn over the first rows and over row B - 1."""
    rng = np.random.default_rng(seed)
    u = rng.integers(-2**31, 2**31, (B, p.N + 1), dtype=np.int64)
    bits = p.ks_t * p.ks_basebit
    off = 1 << (32 - (1 + bits))                 # prec_offset
    top = ((1 << bits) - 1) << (32 - bits)       # every digit base - 1
    directed = [(0 - off) % 2**32,               # a-bar = 0: every digit 0
                (top - off) % 2**32,             # every digit base - 1
                (top - off + 2 * off - 1) % 2**32,   # ... with the bits below the digits all set
                ((1 << 30) - off) % 2**32,       # the offset carries through every lower digit into the top one
                (2**32 - off) % 2**32,           # the offset wraps a-bar to 0
                off - 1, off]                    # just below / at the first step of the last digit
    for r in sorted({0, min(1, B - 1), B - 1}):
        pos = rng.permutation(p.N)[:8 * len(directed)]
        u[r, pos] = np.tile(directed, 8)
    u[min(2, B - 1), :p.N] = directed[0]         # a whole row of zero digits: the result is (0, ..., 0, b)
    u[min(3, B - 1), :p.N] = directed[1]         # a whole row of top digits
    return (u % 2**32).astype(np.uint32).view(np.int32)


def _toy(toy, name, seed):
    if toy not in _CACHE:
        import torch
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        p = ol.params(toy)
        ks = ol.KeySet(p, seed=seed)
        ctx = ol.Ctx(ks)
        u = _samples(p, max(BATCHES), 100 + seed)
        _CACHE[toy] = (p, ks, ctx, _backend(p, name, "wide", ks), u, ctx.keyswitch(u))   # the reference: once, for every batch size
    return _CACHE[toy]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("toy,name,seed", [("toy", "default128", 21), ("toy_redsec", "redsec_small_v2", 22)])
def test_wide_keyswitch_equals_the_oracle_on_every_row(toy, name, seed, B):
    p, ks, ctx, be, u, want = _toy(toy, name, seed)
    got = be.keyswitch(_dev(u[:B])).cpu().numpy()
    assert be.last_keyswitch() == {"form": "wide", "slices": 1}
    assert got.shape == (B, p.n + 1)
    assert np.array_equal(got, want[:B]), np.argwhere(got != want[:B])[:4].tolist()


def test_wide_keyswitch_on_the_full_default128_width():
    """W = 631: 20 word chunks, the last of 23 words. The keyswitch is a deterministic function of whatever key words it is given,
    so the key is random words (as test_gpu_general.py's full-size sets)."""
    import torch
    p = ol.params("default128")
    rng = np.random.default_rng(23)

    class K:
        pass
    ks = K()
    ks.p = p
    ks.bk = np.zeros(p.n * 2 * p.bk_l * 2 * p.N, np.int32)     # not used by a keyswitch
    ks.ksk = rng.integers(-2**31, 2**31, p.N * p.ks_t * (1 << p.ks_basebit) * (p.n + 1), dtype=np.int32)
    B = 2049
    u = _samples(p, B, 24)
    wide, tiled = _backend(p, "default128", "wide", ks), _backend(p, "default128", "tiled", ks)
    try:
        d_u = _dev(u)
        got = wide.keyswitch(d_u).cpu().numpy()
        assert wide.last_keyswitch() == {"form": "wide", "slices": 1}
        other = tiled.keyswitch(d_u).cpu().numpy()
        assert tiled.last_keyswitch()["form"] in ("tiled", "sliced")
        assert np.array_equal(got, other), np.argwhere(got != other)[:4].tolist()
        pick = np.unique(np.concatenate([[0, 1, 2, 3, 1023, 1024, 2047, 2048], rng.integers(0, B, 56)]))[:64]
        ctx = ol.Ctx(ks)
        assert np.array_equal(got[pick], ctx.keyswitch(u[pick]))
        ctx.close()
    finally:
        wide.close()
        tiled.close()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("toy,name,seed", [("toy", "default128", 21), ("toy_redsec", "redsec_small_v2", 22)])
def test_two_input_keyswitch_of_a_mux_in_both_forms(toy, name, seed):
    """bootsMUX: the keyswitch reads the SUM of two extracted samples and adds a constant to its b word (u1 non-null, bconst != 0)."""
    p, ks, ctx, wide, _, _ = _toy(toy, name, seed)
    B = 1025
    rng = np.random.default_rng(seed)
    mu = ol.to_torus(1, 8)
    a, b, c = (ks.encrypt(np.where(rng.integers(0, 2, B) == 1, mu, -mu), 2.0 ** -15, 300 + k) for k in range(3))
    tiled = _backend(p, name, "tiled", ks)
    try:
        got = wide.mux(_dev(a), _dev(b), _dev(c)).cpu().numpy()
        assert wide.last_keyswitch() == {"form": "wide", "slices": 1}
        other = tiled.mux(_dev(a), _dev(b), _dev(c)).cpu().numpy()
        assert tiled.last_keyswitch()["form"] in ("tiled", "sliced")
        assert np.array_equal(got, other)
        pick = np.array([0, 1, 511, 1023, 1024])
        assert np.array_equal(got[pick], ctx.mux_batch(a[pick], b[pick], c[pick]))
    finally:
        tiled.close()


def test_the_form_follows_the_batch_size_when_nothing_is_forced():
    """Unforced: a small batch stays sliced; the form reported is the host plan's (tests/test_keyswitch_form_cpu.py pins its thresholds)."""
    import redsec_amd
    p, ks, ctx, _, u, want = _toy("toy", "default128", 21)
    assert "RS_KS_FORM" not in os.environ
    be = redsec_amd.Backend(redsec_amd.params("default128", n=p.n), device=0)
    be.load_keys(ks.bk, ks.ksk)
    try:
        got = be.keyswitch(_dev(u[:1025])).cpu().numpy()
        assert be.last_keyswitch()["form"] == "sliced" and be.last_keyswitch()["slices"] > 1
        assert np.array_equal(got, want[:1025])
    finally:
        be.close()
