"""Batched circuit bootstrapping on the device (rs_ring_selector_batch_dev, rs_circuit_bootstrap_batch_dev, rs_last_selector;
INTEGRATION.md section 27): word-for-word equality of the batch keyswitch with the numpy restatement in BOTH of its kernels
(RS_SEL_FORM) at every shape at which the wide kernel takes another path, the plan's choice at both sides of its boundary, equality
with the existing calls of at most 30 bits in all three arithmetic modes, the refusals, and arith.evaluate on redsec_small_v2 with
keys generated on the device."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from redsec_amd import arith, keygen

pytestmark = pytest.mark.gpu

MASK_SEED = bytes(range(170, 202))
NOISE_SEED = bytes(range(51, 83))
KEY_SEED = bytes(range(19, 51))
GUARD = 0x5A5A5A5A
RING_SETS = {1024: "redsec_small_v2", 2048: None, 4096: "redsec_medium", 8192: "redsec_large"}
KS_SHAPES = [(8, 4), (1, 1), (4, 6), (2, 12)]                  # (ks_basebit, ks_t); (8, 4) has off = 0
NAME = "redsec_small_v2"
RB, PIECE = 16, 64                                             # rows of a wide register block, coordinates of a staging piece
FORMS = ("wide", "chunked")

_BACKENDS = {}


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value                                # both are read once, in rs_create
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _fresh_backend(N, form=None, mode=None):
    import redsec_amd
    p = redsec_amd.params(RING_SETS[N] or "default128", n=16)
    p.N = N                                                      # N = 2048 is a ring no shipped set has (tests/test_gpu_ring_cmux.py)
    with _env("RS_SEL_FORM", form), _env("REDSEC_MODE", mode):
        be = redsec_amd.Backend(p, device=0)
    assert be.p.N == N and (mode is None or be.mode() == mode)
    return be


def _backend(N, form=None, mode=None):
    """One small-n context per ring, forced form and arithmetic mode: the keyswitch needs no loaded key, the ring is the context's
    and n_src is an argument."""
    if (N, form, mode) not in _BACKENDS:
        _BACKENDS[(N, form, mode)] = _fresh_backend(N, form, mode)
    return _BACKENDS[(N, form, mode)]


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    import torch
    for be in _BACKENDS.values():
        be.close()
    _BACKENDS.clear()
    torch.cuda.empty_cache()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _words(rng, *shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def _u32(a):
    return np.ascontiguousarray(a, np.int32).view(np.uint32)


def _extreme(rng, rows, n_src, basebit, l, ks_basebit, ks_t):
    """The samples of _extreme in tests/test_gpu_ring_selector.py: random words whose first and last coordinates x_i (the b word
    before its half step is added) are the extreme words and 2^32 - off, which wraps x + off to 0."""
    ct = _words(rng, rows, n_src + 1)
    off = 0 if ks_basebit * ks_t >= 32 else 1 << (31 - ks_basebit * ks_t)
    ext = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, ((1 << 32) - off) & 0xFFFFFFFF], np.uint64).astype(np.uint32)
    for r in range(rows):
        half = 1 << (31 - (r % l + 1) * basebit)
        ct[r, 0] = ext[r % ext.size].view(np.int32)
        ct[r, n_src] = np.uint32((int(ext[(r + 2) % ext.size]) - half) & 0xFFFFFFFF).view(np.int32)
    return ct


def _groups(form, rows, N, n_src):
    return 4 * (N // 512) * (-(-rows // RB) if form == "wide" else -(-(n_src + 1) // 8) * -(-rows // 8))


def _check(N, n_src, count, basebit, l, ks_basebit, ks_t, forms=FORMS, side_stream=False):
    """Random words for the key (equality of the sums needs no real one); ONE numpy reference for both kernels; a selector of guard
    words on either side of the output; a second call into the same buffer; the inputs unchanged; last_selector names the kernel.
    forms = (None,) runs unforced and returns the form the plan took."""
    import torch
    rng = np.random.default_rng(N + 7 * n_src + 100 * count + l + 1000 * ks_t)
    rows = count * l
    ct = _extreme(rng, rows, n_src, basebit, l, ks_basebit, ks_t)
    key = _words(rng, 2, n_src + 1, ks_t, 2, N)
    want = keygen.ring_selector_switch(ct, basebit, l, key, ks_basebit, ks_t)
    took = None
    for form in forms:
        be = _backend(N, form)
        guard = be.empty(count + 2, 2 * l, 2, N).fill_(GUARD)
        out = guard[1:count + 1]
        tct, tkey = _dev(ct), _dev(key)
        if side_stream:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):                                       # a non-default stream, the consumer ordered behind it
                got = be.ring_selector_batch(tct, basebit, l, tkey, ks_basebit, ks_t, out=out)
                twice = got * 2
            s.synchronize()
            assert np.array_equal(_u32(twice.cpu().numpy()), _u32(want) * np.uint32(2))
        else:
            got = be.ring_selector_batch(tct, basebit, l, tkey, ks_basebit, ks_t, out=out)
        took = be.last_selector()
        if form is not None:
            assert took == {"form": form, "workgroups": _groups(form, rows, N, n_src)}, took
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (count, 2 * l, 2, N)
        h = got.cpu().numpy()
        assert np.array_equal(h, want), (form, N, n_src, count, basebit, l, ks_basebit, ks_t, np.argwhere(h != want)[:4].tolist())
        be.ring_selector_batch(tct, basebit, l, tkey, ks_basebit, ks_t, out=out)   # a second call: the same words
        assert np.array_equal(out.cpu().numpy(), want)
        assert bool((guard[0] == GUARD).all()) and bool((guard[count + 1] == GUARD).all())
        assert np.array_equal(tct.cpu().numpy(), ct) and np.array_equal(tkey.cpu().numpy(), key)
    return took


@pytest.mark.parametrize("l", [1, 3])
@pytest.mark.parametrize("count", [1, RB - 1, RB, RB + 1, 2 * RB + 2])
def test_batch_words_equal_numpy_around_the_row_block(count, l):
    """1, RB - 1, RB, RB + 1 and 2 RB + 2: as row counts (l = 1) and as bit counts at l = 3, where a row block straddles selectors.
    RB + 1 at l = 3 also on a side stream with a dependent consumer."""
    _check(1024, 13, count, 3, l, 4, 6)
    if (count, l) == (RB + 1, 3):
        _check(1024, 13, count, 3, l, 4, 6, side_stream=True)


@pytest.mark.parametrize("n_src", [PIECE - 2, PIECE - 1, PIECE, 2 * PIECE + 5])
def test_batch_words_equal_numpy_around_the_staging_piece(n_src):
    """n_src + 1 coordinates one below the staging piece, at it, one past it, and two pieces plus six; nine rows"""
    _check(1024, n_src, 3, 3, 3, 4, 6)


@pytest.mark.parametrize("N", [1024, 2048, 4096, 8192])
def test_batch_words_equal_numpy_on_every_ring(N):
    _check(N, 9, 3, 3, 3, 8, 4)


@pytest.mark.parametrize("ks_basebit,ks_t", KS_SHAPES)
def test_batch_words_equal_numpy_for_every_digit_shape_and_gadget(ks_basebit, ks_t):
    _check(1024, 10, 2, 1, 31, ks_basebit, ks_t)
    _check(1024, 10, 1, 8, 3, ks_basebit, ks_t)


@pytest.mark.parametrize("count", [31, 61])
def test_batch_words_equal_numpy_past_the_old_limit_of_thirty_bits(count):
    _check(1024, 9, count, 4, 2, 4, 6)


@pytest.mark.parametrize("N", [1024, 8192])
def test_the_unforced_call_takes_the_plans_form_at_both_sides_of_its_boundary(N):
    """wide as soon as 4 (N / 512) ceil(rows / RB) workgroups give every CU of the device one (tests/test_ring_selector_batch_cpu.py
    pins the rule); l = 1, so count is the row count"""
    import torch
    assert "RS_SEL_FORM" not in os.environ
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    first = (-(-cus // (4 * (N // 512))) - 1) * RB + 1
    below = _check(N, 9, first - 1, 3, 1, 8, 4, forms=(None,))
    assert below == {"form": "chunked", "workgroups": _groups("chunked", first - 1, N, 9)}, (cus, below)
    at = _check(N, 9, first, 3, 1, 8, 4, forms=(None,))
    assert at == {"form": "wide", "workgroups": _groups("wide", first, N, 9)}, (cus, at)


@pytest.mark.parametrize("form", FORMS)
def test_the_batch_call_equals_the_calls_of_at_most_thirty_bits(form):
    """count = 30 equals rs_ring_selector_dev; count = 61 equals its calls of 30, 30 and 1 concatenated; that call keeps the chunked
    kernel whatever RS_SEL_FORM says"""
    import torch
    N, n_src, basebit, l, ks_basebit, ks_t = 1024, 21, 4, 3, 4, 6
    be = _backend(N, form)
    rng = np.random.default_rng(61)
    ct = _dev(_extreme(rng, 61 * l, n_src, basebit, l, ks_basebit, ks_t))
    key = _dev(_words(rng, 2, n_src + 1, ks_t, 2, N))
    old = [be.ring_selector(ct[a * l:b * l], basebit, l, key, ks_basebit, ks_t) for a, b in ((0, 30), (30, 60), (60, 61))]
    assert be.last_selector() == {"form": "chunked", "workgroups": _groups("chunked", l, N, n_src)}
    got = be.ring_selector_batch(ct, basebit, l, key, ks_basebit, ks_t)
    assert be.last_selector()["form"] == form
    assert torch.equal(got, torch.cat(old))
    assert torch.equal(be.ring_selector_batch(ct[:30 * l], basebit, l, key, ks_basebit, ks_t), old[0])


def _bootstrap_both_routes(be, seed):
    """61 bits of random words at l = 2 under a key of random words (the bootstrap is deterministic): the batch call against
    rs_circuit_bootstrap_dev over 30, 30 and 1 bits"""
    import torch
    N, basebit, l, ks_basebit, ks_t, count = be.p.N, 4, 2, 4, 6, 61
    be.load_synthetic_keys(5)
    rng = np.random.default_rng(seed)
    bits = _dev(_words(rng, count, be.W))
    key = _dev(_words(rng, 2, be.W, ks_t, 2, N))
    held = bits.clone()
    old = torch.cat([be.circuit_bootstrap(bits[a:b], basebit, l, key, ks_basebit, ks_t) for a, b in ((0, 30), (30, 60), (60, 61))])
    guard = be.empty(count + 2, 2 * l, 2, N).fill_(GUARD)
    got = be.circuit_bootstrap_batch(bits, basebit, l, key, ks_basebit, ks_t, out=guard[1:count + 1])
    assert torch.equal(got, old), np.argwhere(got.cpu().numpy() != old.cpu().numpy())[:4].tolist()
    be.circuit_bootstrap_batch(bits, basebit, l, key, ks_basebit, ks_t, out=guard[1:count + 1])
    assert torch.equal(guard[1:count + 1], old) and torch.equal(bits, held)
    assert bool((guard[0] == GUARD).all()) and bool((guard[count + 1] == GUARD).all())
    assert len(torch.unique(old)) > 1000                                      # the bootstraps ran: not a buffer of one word
    return be.last_selector()["form"]


@pytest.mark.parametrize("form", FORMS)
def test_the_composed_batch_call_equals_the_composed_calls_of_thirty_bits(form):
    """the default arithmetic mode, in both kernels"""
    assert _bootstrap_both_routes(_backend(1024, form), 7) == form


@pytest.mark.parametrize("mode", ["exact", "split"])
def test_the_composed_batch_call_equals_the_composed_calls_in_the_other_modes(mode):
    """REDSEC_MODE=exact and split: both steps are exact, so the words are those of the calls of thirty bits there too"""
    assert _bootstrap_both_routes(_backend(1024, "wide", mode), 8) == "wide"


def test_batch_invalid_arguments_the_empty_call_and_too_many_rows():
    """Every refusal of test_selector_invalid_arguments_and_the_empty_call (tests/test_gpu_ring_selector.py) restated for count, the
    rows one launch cannot index, count = 0 and the missing evaluation key: nothing is launched and no buffer changes."""
    import torch
    N, n_src, count, l, ks_t = 1024, 10, 2, 3, 6
    be = _fresh_backend(N)                                                    # a context of its own: no key loaded, nothing launched yet
    L, vp = be.L, C.c_void_p
    rng = np.random.default_rng(1)
    ct, key = _dev(_words(rng, count * l, n_src + 1)), _dev(_words(rng, 2, n_src + 1, ks_t, 2, N))
    bits = _dev(_words(rng, count, be.W))
    out = be.empty(count, 2 * l, 2, N).fill_(7)
    scratch = be.empty(l * N + count * l * (2 * be.W + 1))
    torch.cuda.synchronize()
    P = lambda t: vp(t.data_ptr())

    def call(o=P(out), c=P(ct), d=count, basebit=4, l=l, n=n_src, k=P(key), kb=4, kt=ks_t):
        return L.rs_ring_selector_batch_dev(be.h, o, c, C.c_size_t(d), basebit, l, n, k, kb, kt, None)

    def boot(o=P(out), c=P(bits), d=count, basebit=4, l=l, k=P(key), kb=4, kt=ks_t, sc=P(scratch)):
        return L.rs_circuit_bootstrap_batch_dev(be.h, o, c, C.c_size_t(d), basebit, l, k, kb, kt, sc, None)
    with pytest.raises(Exception, match="no selector keyswitch"):
        be.last_selector()
    assert boot() == -4 and b"rs_load_keys" in L.rs_last_error()             # RS_ERR_STATE: this context has no evaluation key
    assert call(o=None) == -1 and call(c=None) == -1 and call(k=None) == -1 and b"null pointer" in L.rs_last_error()
    for bad in (0, 9, -1):
        assert call(basebit=bad, l=1) == -1 and b"basebit" in L.rs_last_error() and b"outside 1 .. 8" in L.rs_last_error()
        assert call(kb=bad, kt=1) == -1 and b"ks_basebit" in L.rs_last_error() and b"outside 1 .. 8" in L.rs_last_error()
    for bad in (0, -3):
        assert call(l=bad) == -1 and b"l = " in L.rs_last_error() and b"below 1" in L.rs_last_error()
        assert call(kt=bad) == -1 and b"ks_t = " in L.rs_last_error() and b"below 1" in L.rs_last_error()
    for basebit, ll in ((4, 8), (8, 4), (1, 32)):
        assert call(basebit=basebit, l=ll) == -1 and b"passes 31 bits" in L.rs_last_error()
    for kb, kt in ((4, 9), (8, 5), (1, 33)):
        assert call(kb=kb, kt=kt) == -1 and b"passes 32 bits" in L.rs_last_error()
    for bad in (0, -1, 65537):
        assert call(n=bad) == -1 and b"n_src" in L.rs_last_error() and b"outside 1 .. 65536" in L.rs_last_error()
    assert call(k=vp(key.data_ptr() + 4)) == -1 and b"sel_key must be 16-byte aligned" in L.rs_last_error()
    # rows past one launch, in either kernel's grid and in the row arithmetic itself: refused before anything is looked at
    for big in (1 << 31, 1 << 40, (1 << 64) - 1, (1 << 31) // 3 + 1):
        assert call(d=big) == -1 and b"count l = " in L.rs_last_error() and b"rows are too many for one launch" in L.rs_last_error()
    assert call(d=(1 << 31) // 3 + 1) == -1 and b"count l = 2147483649 rows are too many for one launch" in L.rs_last_error()
    # a sel that shares a byte with an input is refused. Every range named below lies inside one allocation of sixteen ring
    # samples (sel is twelve) or inside the key (132)
    arena = _dev(_words(rng, 16, 2, N))
    held, held_key = arena.cpu().numpy(), key.cpu().numpy()
    A, K, row, ring = arena.data_ptr(), key.data_ptr(), 4 * (n_src + 1), 8 * N
    for o in (A, A + row, A + count * l * row - 4):                           # sel == ct, one sample into ct, on its last word
        assert call(o=vp(o), c=vp(A)) == -1 and b"sel overlaps ct" in L.rs_last_error()
    assert call(o=vp(A), c=vp(A + 12 * ring - 4)) == -1 and b"sel overlaps ct" in L.rs_last_error()   # sel's last word is ct's first
    for o in (K, K + ring, K + 120 * ring):                                   # sel on the key's first, second and last twelve samples
        assert call(o=vp(o)) == -1 and b"sel overlaps sel_key" in L.rs_last_error()
    assert call(o=vp(A + 4)) == -1 and b"sel must be 16-byte aligned" in L.rs_last_error()
    with pytest.raises(ValueError, match="sel overlaps ct"):
        be.ring_selector_batch(arena.view(-1)[:count * l * (n_src + 1)].view(count * l, n_src + 1), 4, l, key, 4, ks_t, out=arena[:12])
    with pytest.raises(ValueError, match="sel overlaps sel_key"):
        be.ring_selector_batch(ct, 4, l, key, 4, ks_t, out=key.view(-1, 2, N)[120:])
    # nothing above launched anything; count = 0 is a no-op
    assert call(d=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert np.array_equal(arena.cpu().numpy(), held) and np.array_equal(key.cpu().numpy(), held_key)
    with pytest.raises(Exception, match="no selector keyswitch"):
        be.last_selector()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), keygen.ring_selector_switch(ct.cpu().numpy(), 4, l, key.cpu().numpy(), 4, ks_t))
    assert be.last_selector()["form"] == "chunked"                           # six rows
    with pytest.raises(ValueError, match="explicit ks_basebit"):
        be.ring_selector_batch(ct, 4, l, key)
    with pytest.raises(ValueError):
        be.ring_selector_batch(ct, 4, 8, key, 4, ks_t)
    with pytest.raises(ValueError):
        be.ring_selector_batch(ct, 4, l, key, 4, 9)
    # the composed call refuses the same overlaps and those of its scratch. It looks at them behind the check for a loaded key, so
    # the context gets one of random words; nothing below launches anything else
    be.load_synthetic_keys(5)
    key16 = _dev(_words(rng, 2, be.W, ks_t, 2, N))                           # a key of the context's n = 16
    out.fill_(7)
    torch.cuda.synchronize()
    words = scratch.numel()
    assert words == l * N + count * l * (2 * be.W + 1)
    assert boot(o=None, k=P(key16)) == -1 and boot(sc=None, k=P(key16)) == -1 and b"null pointer" in L.rs_last_error()
    assert boot(d=1 << 40, k=P(key16)) == -1 and b"rows are too many for one launch" in L.rs_last_error()
    assert boot(d=0, k=P(key16)) == 0
    for o in (A, A + 4 * be.W, A + 4 * (count * be.W - 1)):                   # sel == bits, one bit into them, on their last word
        assert boot(o=vp(o), c=vp(A), k=P(key16)) == -1 and b"sel overlaps bits" in L.rs_last_error()
    assert boot(o=P(key16), k=P(key16)) == -1 and b"sel overlaps sel_key" in L.rs_last_error()
    assert boot(o=vp(A), sc=vp(A), k=P(key16)) == -1 and b"sel overlaps scratch" in L.rs_last_error()
    assert boot(o=vp(A), sc=vp(A + 12 * ring - 4), k=P(key16)) == -1 and b"sel overlaps scratch" in L.rs_last_error()   # sel's last word
    assert boot(o=vp(A + 4 * (words - 1)), sc=vp(A), k=P(key16)) == -1 and b"sel overlaps scratch" in L.rs_last_error()  # scratch's last word
    assert boot(c=vp(A + 4 * (words - 1)), sc=vp(A), k=P(key16)) == -1 and b"scratch overlaps bits" in L.rs_last_error()
    assert boot(sc=P(key16), k=P(key16)) == -1 and b"scratch overlaps sel_key" in L.rs_last_error()
    with pytest.raises(ValueError, match="sel overlaps bits"):
        be.circuit_bootstrap_batch(arena.view(-1)[:count * be.W].view(count, be.W), 4, l, key16, 4, ks_t, out=arena[:12])
    with pytest.raises(ValueError, match="sel overlaps sel_key"):
        be.circuit_bootstrap_batch(bits, 4, l, key16, 4, ks_t, out=key16.view(-1, 2, N)[:12])
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and np.array_equal(arena.cpu().numpy(), held)
    be.close()


def test_evaluate_makes_its_selectors_in_one_batch_and_decrypts():
    """redsec_small_v2 with keys generated on the device: arith.evaluate at R = 7, depth 5 (35 bits: two calls on the route of at
    most 30 bits). Every output decrypts to table[index], and the selectors of the ONE batch call equal those of that loop, run
    here, word for word."""
    import redsec_amd
    import torch
    be = redsec_amd.Backend(redsec_amd.params(NAME), device=0)
    try:
        sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
        del bk, ksk
        n, N, depth = be.p.n, be.p.N, 5
        basebit, l, ks_basebit, ks_t = keygen.circuit_bootstrap_default(NAME, depth, digits="alternating")
        dkey = be.upload_selector_key(sk.selector_key(ks_basebit, ks_t, MASK_SEED, NOISE_SEED))
        rng = np.random.default_rng(35)
        table = rng.integers(0, 2, 1 << depth)
        values = np.where(table != 0, 1 << 29, -(1 << 29)).astype(np.int32)
        indices = [0, 31, 1, 16, 21, 10, 27]
        plain = np.array([[(i >> k) & 1 for i in indices] for k in range(depth)])              # [bit][index], LSB first
        bits = _dev(sk.encrypt_bits(plain.ravel(), seed=11)).reshape(depth, len(indices), n + 1)
        out = arith.evaluate(be, bits, values, dkey, 1, basebit, l, ks_basebit, ks_t, digits="alternating")
        assert tuple(out.shape) == (len(indices), n + 1)
        assert np.array_equal(sk.decrypt_bits(out, backend=be), table[indices])
        flat = bits.permute(1, 0, 2).contiguous().reshape(len(indices) * depth, n + 1)       # bit k of index r is sample r depth + k
        assert flat.shape[0] == 35 > arith.CIRCUIT_BOOTSTRAP_BITS
        old = torch.cat([be.circuit_bootstrap(flat[a:a + 30], basebit, l, dkey, ks_basebit, ks_t) for a in (0, 30)])
        new = be.circuit_bootstrap_batch(flat, basebit, l, dkey, ks_basebit, ks_t)
        assert tuple(new.shape) == (35, 2 * l, 2, N) and torch.equal(new, old)
    finally:
        be.close()
        torch.cuda.empty_cache()
