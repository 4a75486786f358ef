"""GPU parity of the three-input gates and the indexed gate batches (include/redsec_hip.h rs_gate3_dev / rs_gate_rows_dev;
INTEGRATION.md section 14) against the CPU oracle, word for word: the combinations are restated in numpy (tests/rows_ref.py) and the
expected output is always the EXISTING oracle's bootstrap of them. Oracle results are computed once per case and shared by the
arithmetic modes (the library's results are the same words in every mode)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import rows_ref as rr
from backend_pool import BackendPool

pytestmark = pytest.mark.gpu

ALPHA = 2.0 ** -15
E8 = 1 << 29
POOL = BackendPool()
_REF = {}          # oracle results, keyed by case: computed by the first arithmetic mode that needs them, never changed


def _ref(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def _bootstrap_rows_once(ctx, x, mu):
    """ctx.bootstrap_batch(x, mu) with every distinct row bootstrapped by the oracle once per module: the comparator's borrow chain
    is the subtractor's, row for row, and both arithmetic modes ask for the same rows."""
    keys = [(mu, row.tobytes()) for row in x]
    missing = [r for r, k in enumerate(keys) if k not in _REF]
    if missing:
        for r, out in zip(missing, ctx.bootstrap_batch(x[missing], mu)):
            _REF[keys[r]] = out
    return np.stack([_REF[k] for k in keys])


def _make(ks, name, **fields):
    import torch
    import redsec_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = redsec_amd.params(name, n=ks.p.n)
    for k, v in fields.items():
        setattr(p, k, v)
    be = redsec_amd.Backend(p, device=0)
    be.load_keys(ks.bk, ks.ksk)
    return be


@pytest.fixture(scope="module", autouse=True)
def _close_module_contexts():
    yield
    POOL.close_all()
    _REF.clear()


@pytest.fixture(autouse=True, params=["fft", "exact"])
def arith_mode(request):
    """Every test runs in the FFT mode and in the exact NTT mode unless it names its own list (indirect parametrisation)."""
    POOL.enter_mode(request.param)
    yield request.param
    POOL.leave_mode(request.param)


@pytest.fixture(scope="module")
def be_toy_default(toy_default):
    return POOL.add(_make(toy_default[0], "default128"))


@pytest.fixture(scope="module")
def be_toy_redsec(toy_redsec):
    return POOL.add(_make(toy_redsec[0], "redsec_small_v2"))


@pytest.fixture(scope="module")
def be_full_default(full_default):
    return POOL.add(_make(full_default[0], "default128"))


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()


def _idx_dev(idx):
    return _dev(np.asarray(idx, np.int64).astype(np.int32))


def _encrypt_bits(ks, bits, seed):
    return ks.encrypt(np.where(np.asarray(bits) == 1, E8, -E8), ALPHA, seed)


def _spread(ops, B, empty_at):
    """B rows over the groups `ops` in order, as evenly as the count allows, with one extra EMPTY group at position `empty_at`."""
    counts = [B // len(ops) + (1 if k < B % len(ops) else 0) for k in range(len(ops))]
    groups = [(op, c) for op, c in zip(ops, counts)]
    groups.insert(empty_at, ("XNOR", 0))
    return groups


def _random_idx(rng, B, in_rows):
    """Random source rows with the four kinds of special index and a repeated row sprinkled in."""
    idx = rng.integers(0, in_rows, (B, 3)).astype(np.int64)
    special = rng.permutation([-1, -2, in_rows, in_rows + 7, -9, 2**31 - 1, -2**31])
    slots = rng.choice(3 * B, size=min(len(special), 3 * B - 1), replace=False)      # at least one real row stays
    idx.ravel()[slots] = special[:len(slots)]
    if B > 1:
        idx[B - 1] = rng.integers(0, in_rows)          # one row three times
    return idx


@pytest.mark.parametrize("mu", [1 << 29, 1 << 28])
@pytest.mark.parametrize("B", [1, 7, 130])
@pytest.mark.parametrize("which,fix", [("be_toy_default", "toy_default"), ("be_toy_redsec", "toy_redsec")])
def test_toy_gate_rows_equal_the_oracle(which, fix, B, mu, request):
    """All thirteen ops in groups (one of them empty), random indices with -1, -2, out-of-range values and repeated rows, batches of
    one row, less than a workgroup's four rows and many workgroups: every call equals the oracle's bootstrap of the restated
    combinations. A batch too small for thirteen groups takes several calls, the op list rotated, until every op has run."""
    be = request.getfixturevalue(which)
    ks, ctx = request.getfixturevalue(fix)
    in_rows = 11
    rng = np.random.default_rng(1000 * B + (mu >> 28))
    inp = _encrypt_bits(ks, rng.integers(0, 2, in_rows), 7 + B)
    dinp = _dev(inp)
    calls = 1 if B >= 13 else -(-13 // B)
    for call in range(calls):
        ops = rr.OPS[call * B % 13:] + rr.OPS[:call * B % 13]
        groups = _spread(ops, B, empty_at=3 + call)
        idx = _random_idx(rng, B, in_rows)
        x = rr.combine(inp, idx, groups)
        want = _ref((fix, B, mu, call), lambda: ctx.bootstrap_batch(x, mu))
        got = be.gate_rows(dinp, _idx_dev(idx), groups, mu=mu).cpu().numpy()
        assert np.array_equal(got, want), (call, groups)
        if mu == E8:
            # rows of the two-input ops are the words of rs_gate_dev on the same sources
            a, b = (rr.source_rows(inp, idx[:, j]).astype(np.int32) for j in (0, 1))
            per_row = np.array(rr.op_per_row(groups))
            for op in ol.GATES:
                rows = np.nonzero(per_row == op)[0]
                if len(rows):
                    assert np.array_equal(be.gate(op, _dev(a[rows]), _dev(b[rows])).cpu().numpy(), got[rows]), op


@pytest.mark.parametrize("which,fix", [("be_toy_default", "toy_default"), ("be_toy_redsec", "toy_redsec")])
def test_gate3_is_gate_rows_with_the_identity_index(which, fix, request):
    be = request.getfixturevalue(which)
    ks, ctx = request.getfixturevalue(fix)
    B = 7
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, (3, B))
    a, b, c = (_encrypt_bits(ks, bits[j], 30 + j) for j in range(3))
    inp = _dev(np.concatenate([a, b, c]))
    r = np.arange(B)
    idx = _idx_dev(np.stack([r, B + r, 2 * B + r], 1))
    for op in ("MAJ3", "XOR3", "MAJ3N"):
        got = be.gate3(op, _dev(a), _dev(b), _dev(c)).cpu().numpy()
        assert np.array_equal(got, be.gate_rows(inp, idx, [(op, B)]).cpu().numpy()), op
        want = _ref((fix, "gate3", op), lambda: ctx.bootstrap_batch(rr.combine3(a, b, c, None, [(op, B)]), E8))
        assert np.array_equal(got, want), op
        assert np.array_equal((ks.phase(got) > 0).astype(int), rr.TRUTH[op](bits[0], bits[1], bits[2])), op


def _aliasing_case(ks, B):
    in_rows = B + 6
    rng = np.random.default_rng(B)
    inp = _encrypt_bits(ks, rng.integers(0, 2, in_rows), 77)
    # output rows 2 .. 2 + B are rows the call reads, in another order and more than once
    idx = np.stack([2 + rng.permutation(B), 2 + (np.arange(B) * 7 + 3) % B, rng.integers(0, in_rows, B)], 1)
    idx[0, 2] = -1
    groups = [("XOR3", B // 2), ("MAJ3N", 0), ("MAJ3", B - B // 2)]
    return inp, idx, groups


def _check_aliasing(be, ks, ctx, fix):
    B = 130
    inp, idx, groups = _aliasing_case(ks, B)
    want = _ref((fix, "alias"), lambda: ctx.bootstrap_batch(rr.combine(inp, idx, groups), E8))
    didx = _idx_dev(idx)
    apart = be.gate_rows(_dev(inp), didx, groups)
    arena = _dev(inp)
    out = be.gate_rows(arena, didx, groups, out=arena[2:2 + B])
    assert out.data_ptr() == arena[2:2 + B].data_ptr()
    return apart, arena, inp, want, B


def test_output_may_alias_rows_the_call_reads(be_toy_default, toy_default):
    ks, ctx = toy_default
    apart, arena, inp, want, B = _check_aliasing(be_toy_default, ks, ctx, "toy_default")
    assert np.array_equal(apart.cpu().numpy(), want)
    got = arena.cpu().numpy()
    assert np.array_equal(got[2:2 + B], want)
    assert np.array_equal(got[:2], inp[:2]) and np.array_equal(got[2 + B:], inp[2 + B:])


def test_aliasing_on_a_side_stream_then_certify(be_toy_default, toy_default, arith_mode):
    import torch
    be = be_toy_default
    ks, ctx = toy_default
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        apart, arena, inp, want, B = _check_aliasing(be, ks, ctx, "toy_default")
        distance, recomputed = be.certify(reset=True)      # synchronises the side stream
    assert np.array_equal(apart.cpu().numpy(), want) and np.array_equal(arena.cpu().numpy()[2:2 + B], want)
    assert recomputed == 0 and distance < 0.2
    be.release_stream(s.cuda_stream)


@pytest.mark.parametrize("arith_mode", ["split"], indirect=True)
def test_split_mode(be_toy_redsec, toy_redsec):
    be = be_toy_redsec
    ks, ctx = toy_redsec
    be.set_mode("split")
    B, in_rows = 130, 9
    rng = np.random.default_rng(8)
    inp = _encrypt_bits(ks, rng.integers(0, 2, in_rows), 3)
    idx = _random_idx(rng, B, in_rows)
    groups = _spread(rr.OPS, B, empty_at=0)
    want = ctx.bootstrap_batch(rr.combine(inp, idx, groups), E8)
    assert np.array_equal(be.gate_rows(_dev(inp), _idx_dev(idx), groups).cpu().numpy(), want)


@pytest.mark.parametrize("arith_mode", ["fft"], indirect=True)
def test_argument_errors_leave_the_context_usable(be_toy_default, toy_default):
    from redsec_amd import backend
    be = be_toy_default
    ks, ctx = toy_default
    L, h = be.L, be.h
    B = 4
    inp = _dev(_encrypt_bits(ks, [0, 1, 1, 0], 1))
    out = be.empty(B, be.W)
    idx = _idx_dev(np.zeros((B, 3)))
    po, pi, px = (C.c_void_p(t.data_ptr()) for t in (out, inp, idx))

    def groups(*items):
        g = (backend.RsRowGroup * len(items))()
        for slot, (op, count, *reserved) in zip(g, items):
            slot.op, slot.count, slot.reserved = op, count, reserved[0] if reserved else 0
        return g
    ok = groups((10, 3), (4, 0), (11, 1))
    rows = lambda o, i, x, g, n, b: L.rs_gate_rows_dev(h, o, i, 4, x, g, n, E8, b, None)
    assert rows(po, pi, px, ok, 3, B) == 0
    for bad in ((None, pi, px, ok, 3, B), (po, None, px, ok, 3, B), (po, pi, None, ok, 3, B), (po, pi, px, None, 3, B),     # null pointers
                (po, pi, px, ok, 0, B), (po, pi, px, groups(*[(0, 0)] * 16 + [(0, B)]), 17, B), (po, pi, px, ok, -1, B),   # n_groups
                (po, pi, px, groups((13, B)), 1, B), (po, pi, px, groups((-1, B)), 1, B),                                  # op
                (po, pi, px, groups((10, B, 1)), 1, B),                                                                     # reserved
                (po, pi, px, ok, 3, B + 1), (po, pi, px, ok, 3, B - 1), (po, pi, px, groups((10, 2**63), (10, 2**63)), 2, 0)):   # sum != B
        assert rows(*bad) == -1, bad[4:]
        assert L.rs_last_error()
    assert rows(po, pi, px, groups(*[(k % 13, 0) for k in range(15)] + [(12, B)]), 16, B) == 0      # 16 groups are allowed
    assert rows(po, pi, px, groups((10, 0)), 1, 0) == 0                                               # B = 0: a no-op
    g3 = lambda op, o, a, b, c, n: L.rs_gate3_dev(h, op, o, a, b, c, n, None)
    for op in (9, 13, -1):
        assert g3(op, po, pi, pi, pi, B) == -1, op
    for args in ((None, pi, pi, pi), (po, None, pi, pi), (po, pi, None, pi), (po, pi, pi, None)):
        assert g3(10, *args, B) == -1
    assert g3(10, po, pi, pi, pi, 0) == 0
    be.sync()
    # the context still computes
    gs = [("MAJ3", 3), ("XOR", 0), ("XOR3", 1)]
    want = ctx.bootstrap_batch(rr.combine(inp.cpu().numpy(), np.zeros((B, 3)), gs), E8)
    assert np.array_equal(be.gate_rows(inp, idx, gs).cpu().numpy(), want)


@pytest.mark.parametrize("arith_mode", ["split"], indirect=True)
def test_general_ring_n2048_on_a_synthetic_key():
    """The general kernels behind the same pre-pass: default-128 gadget on N = 2048, n = 12, a synthetic key generated on the
    device and restated for the oracle (not an encryption of anything: word parity only)."""
    import redsec_amd
    seed = 0x5eed15
    p = ol.params("toy_n2048")
    bp = redsec_amd.params("default128", n=p.n)
    bp.N = p.N

    class K:
        pass
    ks = K()
    ks.p = p
    ks.bk = ol.synthetic_key_words(seed, p.n * 2 * p.bk_l * 2 * p.N)
    ks.ksk = ol.synthetic_key_words(seed ^ 0x6b73, p.N * p.ks_t * (1 << p.ks_basebit) * (p.n + 1))
    ctx = ol.Ctx(ks)
    with POOL.scratch(lambda: redsec_amd.Backend(bp, device=0)) as be:
        be.load_synthetic_keys(seed)
        assert be.mode() == "split"
        B, in_rows = 5, 4
        rng = np.random.default_rng(2)
        inp = rng.integers(-2**31, 2**31, (in_rows, p.n + 1)).astype(np.int32)
        idx = _random_idx(rng, B, in_rows)
        groups = [("MAJ3", 2), ("NAND", 0), ("XOR3", 2), ("MAJ3N", 1)]
        got = be.gate_rows(_dev(inp), _idx_dev(idx), groups).cpu().numpy()
        assert be.last_launch()["form"] == "general"
        assert np.array_equal(got, ctx.bootstrap_batch(rr.combine(inp, idx, groups), E8))
    ctx.close()


# ---- the full default-128 key ----
@pytest.mark.parametrize("op", ["MAJ3", "XOR3", "MAJ3N"])
def test_full_key_three_input_gates_on_fresh_and_on_bootstrapped_inputs(be_full_default, full_default, op):
    """B = 64: the eight input combinations, eight encryptions of each, on fresh ciphertexts (alpha = 2^-15) and again on outputs of
    a previous gate level. Word for word the oracle, and every decryption right: the derived margin is at least 20 sigma."""
    be = be_full_default
    ks, ctx = full_default
    B = 64
    v = np.arange(B) % 8
    bits = np.stack([(v >> 2) & 1, (v >> 1) & 1, v & 1])
    truth = rr.TRUTH[op](bits[0], bits[1], bits[2])
    fresh = [_encrypt_bits(ks, bits[j], 500 + j) for j in range(3)]
    got = be.gate3(op, *(_dev(x) for x in fresh)).cpu().numpy()
    assert np.array_equal(got, _ref(("full", op, 1), lambda: ctx.bootstrap_batch(rr.combine3(*fresh, None, [(op, B)]), E8)))
    assert np.array_equal((ks.phase(got) > 0).astype(int), truth)
    # a previous gate level: AND(x, x) decrypts as x and carries the noise of a gate output
    level = [be.gate("AND", _dev(x), _dev(x)) for x in fresh]
    host = [t.cpu().numpy() for t in level]
    for j in range(3):
        assert np.array_equal((ks.phase(host[j]) > 0).astype(int), bits[j])
    again = be.gate3(op, *level).cpu().numpy()
    assert np.array_equal(again, _ref(("full", op, 2), lambda: ctx.bootstrap_batch(rr.combine3(*host, None, [(op, B)]), E8)))
    assert np.array_equal((ks.phase(again) > 0).astype(int), truth)


class _Recorder:
    """A backend whose gate_rows calls are written down: the arena before the call, the indices, the groups, the result."""

    def __init__(self, be):
        self.be = be
        self.W = be.W
        self.levels = []

    def gate_rows(self, inp, idx, groups, mu=None, out=None):
        before = inp.cpu().numpy().reshape(-1, self.W)
        res = self.be.gate_rows(inp, idx, groups, mu=mu, out=out)
        self.levels.append((before, idx.cpu().numpy().astype(np.int64), list(groups), res.cpu().numpy()))
        return res


ARITH_BITS, ARITH_B = 8, 32


def _arith_inputs(ks):
    """32 pairs of 8-bit values: eight with a = b, eight with b = a + 1, eight with a = b + 1, eight random."""
    rng = np.random.default_rng(15)
    xa = rng.integers(1, 255, ARITH_B)
    xb = np.concatenate([xa[:8], xa[8:16] + 1, xa[16:24] - 1, rng.integers(0, 256, 8)])
    xa[0], xb[0] = 0, 0
    xa[1], xb[1] = 255, 255
    enc = lambda v, seed: np.stack([_encrypt_bits(ks, (v >> i) & 1, seed + i) for i in range(ARITH_BITS)])
    return xa, xb, enc(xa, 9000), enc(xb, 9100)


def _check_levels(name, rec, ctx):
    assert len(rec.levels) == ARITH_BITS
    for bit, (before, idx, groups, got) in enumerate(rec.levels):
        want = _bootstrap_rows_once(ctx, rr.combine(before, idx, groups), E8)
        assert np.array_equal(got, want), (name, bit)


def _value(ks, ct):
    return sum(((ks.phase(ct[i]) > 0).astype(np.int64) << i) for i in range(ct.shape[0]))


def test_full_key_adder(be_full_default, full_default):
    from redsec_amd import arith
    ks, ctx = full_default
    xa, xb, a, b = _arith_inputs(ks)
    rec = _Recorder(be_full_default)
    s = arith.add(rec, _dev(a), _dev(b)).cpu().numpy()
    assert s.shape == (ARITH_BITS + 1, ARITH_B, ks.W)
    _check_levels("add", rec, ctx)
    assert np.array_equal(_value(ks, s), xa + xb)


def test_full_key_subtractor(be_full_default, full_default):
    from redsec_amd import arith
    ks, ctx = full_default
    xa, xb, a, b = _arith_inputs(ks)
    rec = _Recorder(be_full_default)
    d, borrow = arith.sub(rec, _dev(a), _dev(b))
    _check_levels("sub", rec, ctx)
    assert np.array_equal(_value(ks, d.cpu().numpy()), (xa - xb) % 256)
    assert np.array_equal((ks.phase(borrow.cpu().numpy()) > 0).astype(int), (xa < xb).astype(int))


def test_full_key_comparator(be_full_default, full_default):
    from redsec_amd import arith
    ks, ctx = full_default
    xa, xb, a, b = _arith_inputs(ks)
    assert (xa[:8] == xb[:8]).all() and (np.abs(xa[8:24] - xb[8:24]) == 1).all()
    rec = _Recorder(be_full_default)
    lt = arith.less_than(rec, _dev(a), _dev(b)).cpu().numpy()
    _check_levels("less_than", rec, ctx)
    assert all(len(idx) == ARITH_B for _, idx, _, _ in rec.levels)
    assert np.array_equal((ks.phase(lt) > 0).astype(int), (xa < xb).astype(int))
