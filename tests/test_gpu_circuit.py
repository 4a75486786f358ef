"""GPU parity of the compiled circuits (include/redsec_hip.h rs_circuit_create / rs_circuit_run_dev)
against the CPU oracle, word for word: the expected arena comes from tests/circuit_ref.py's gate-by-gate evaluator in netlist order
(the EXISTING oracle's bootstrap and bootsMUX), whatever the level schedule. Oracle results are computed once per case, at the
largest lane count, and shared by the lane counts and the arithmetic modes (a cell's words depend only on its source words)."""
import ctypes as C

import numpy as np
import pytest

import circuit_ref as cr
from backend_pool import BackendPool

pytestmark = pytest.mark.gpu

ALPHA = 2.0 ** -15
E8 = 1 << 29
POOL = BackendPool()
_REF = {}          # oracle results, keyed by case: computed by the first test that needs them, never changed
LANES = 130        # 130 lanes put the 13-cell level past 4 x the CU count: the lock-step form


def _ref(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def _make(ks, name):
    import torch
    import redsec_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    be = redsec_amd.Backend(redsec_amd.params(name, n=ks.p.n), device=0)
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


def _encrypt_bits(ks, bits, seed):
    bits = np.asarray(bits)
    return ks.encrypt(np.where(bits.ravel() == 1, E8, -E8), ALPHA, seed).reshape(bits.shape + (ks.W,))


# ---- one random netlist: 41 cells over 6 inputs in five levels ----
def _random_netlist():
    """Level 1: the thirteen row ops (no MUX, more than eight cells); level 2: five MUX cells and nothing else; levels 3 and 4: mixed,
    MUX cells among them; level 5: three cells. Random polarities everywhere, both constants, every gate an output (some negated)."""
    from redsec_amd import circuit
    rng = np.random.default_rng(2024)
    nl = circuit.Netlist(6)
    ins = nl.inputs()

    def pol(w):
        return nl.not_(w) if rng.integers(0, 2) else w

    def pick(pool):
        return pol(pool[int(rng.integers(0, len(pool)))])
    consts = [nl.const(0), nl.const(1)]
    level1 = []
    for op in range(13):
        srcs = [pick(ins), pick(ins + consts), pick(ins + consts)]
        if op == 1:
            srcs[1] = nl.const(0)
        if op == 11:
            srcs[2] = pol(nl.const(1))
        level1.append(nl.gate(op, srcs[0], srcs[1], srcs[2] if op >= 10 else None))
    level2 = [nl.mux(pick(level1), pick(level1 + ins), pick(level1 + ins + consts)) for _ in range(4)]
    level2.append(nl.mux(pick(level1), nl.const(1), pick(ins)))                          # a MUX with a constant branch

    def mixed(prev, older, plain, muxes):
        out = []
        for _ in range(plain):
            op = int(rng.integers(0, 13))
            srcs = [pick(prev), pick(older), pick(older + consts)]
            order = rng.permutation(3)
            a, b, c = (srcs[k] for k in order) if op >= 10 else (srcs[0], srcs[1], None)
            out.append(nl.gate(op, a, b, c))
        for _ in range(muxes):
            srcs = [pick(prev), pick(older), pick(older)]
            a, b, c = (srcs[k] for k in rng.permutation(3))
            out.append(nl.mux(a, b, c))
        return out
    level3 = mixed(level2, level1 + level2 + ins, 8, 4)
    level4 = mixed(level3, level2 + level3 + ins, 6, 2)
    level5 = mixed(level4, level3 + level4 + ins, 3, 0)
    for w in level1 + level2 + level3 + level4 + level5:
        nl.output(pol(w))
    return nl


def _netlist_case():
    nl = _ref("netlist", _random_netlist)
    plan = _ref("plan", nl.compile)
    return nl, plan


def test_the_random_netlist_has_the_shape_the_cases_need(arith_mode):
    nl, plan = _netlist_case()
    assert plan.cells == 41 and plan.depth == 5 and plan.n_inputs == 6
    assert [(c, m) for _, c, m in plan.levels()] == [(13, 0), (5, 5), (12, 4), (8, 2), (3, 0)]
    assert set(plan.table["op"].tolist()) == set(range(14))
    assert plan.table["neg"].any() and {-1, -2} <= set(plan.table["src"].ravel().tolist())
    assert plan.rotations == 41 + 11
    cus = POOL.live()[0].info()["num_cus"] if POOL.live() else 256
    assert 13 * LANES > 4 * cus


def _inputs(ks, fix):
    rng = np.random.default_rng(99)
    return _ref((fix, "inputs"), lambda: _encrypt_bits(ks, rng.integers(0, 2, (6, LANES)), 31))


def _expected(ks, ctx, fix):
    """the whole arena at 130 lanes, from the oracle evaluator in netlist order"""
    nl, plan = _netlist_case()
    inputs = _inputs(ks, fix)
    return _ref((fix, "arena"), lambda: cr.expected_arena(plan, inputs, cr.oracle_wires(ctx, nl, inputs)))


def _mux_sources(be, arena, cell, lanes):
    """the three (negated) source tensors of a MUX cell, from the device arena"""
    out = []
    for j in range(3):
        src = int(cell["src"][j])
        if src < 0:
            t = _dev(cr.wrap(cr.trivial(src == -2, lanes, be.W)))
        else:
            t = arena[src].contiguous()
        out.append(be.lincomb(t, -1) if (int(cell["neg"]) >> j) & 1 else t)
    return out


@pytest.mark.parametrize("lanes", [1, 3, LANES])
@pytest.mark.parametrize("which,fix", [("be_toy_default", "toy_default"), ("be_toy_redsec", "toy_redsec")])
def test_random_netlist_whole_arena_equals_the_oracle(which, fix, lanes, request):
    be = request.getfixturevalue(which)
    ks, ctx = request.getfixturevalue(fix)
    nl, plan = _netlist_case()
    want = _expected(ks, ctx, fix)[:, :lanes]
    bound = plan.bind(be)
    out = bound.run(_dev(_inputs(ks, fix)[:, :lanes]))
    arena = bound.arena
    got = arena.cpu().numpy()
    assert got.shape == want.shape == (47, lanes, ks.W)
    assert np.array_equal(got[:6], want[:6])
    for v, (first, cells, mux) in enumerate(plan.levels()):
        rows = slice(6 + first, 6 + first + cells)
        assert np.array_equal(got[rows], want[rows]), ("level", v + 1)
    # the outputs: every gate, some negated
    for k, (src, neg) in enumerate(plan.outputs):
        assert np.array_equal(out[k].cpu().numpy(), cr.wrap(-want[src].astype(np.int64)) if neg else want[src]), k
    # the MUX rows are rs_mux_dev's words on the same (negated) sources
    muxes = np.nonzero(plan.table["op"] == cr.MUX)[0]
    assert len(muxes) == 11
    for i in muxes:
        a, b, c = _mux_sources(be, arena, plan.table[i], lanes)
        assert np.array_equal(be.mux(a, b, c).cpu().numpy(), got[6 + i]), ("mux cell", int(i))
    bound.close()


@pytest.mark.parametrize("arith_mode", ["split"], indirect=True)
def test_split_mode_then_certify(be_toy_redsec, toy_redsec):
    be = be_toy_redsec
    ks, ctx = toy_redsec
    be.set_mode("split")
    assert be.mode() == "split"
    nl, plan = _netlist_case()
    lanes = 3
    want = _expected(ks, ctx, "toy_redsec")[:, :lanes]
    bound = plan.bind(be)
    bound.run(_dev(_inputs(ks, "toy_redsec")[:, :lanes]))
    distance, recomputed = be.certify(reset=True)          # raises if the enforced certificate failed
    assert np.array_equal(bound.arena.cpu().numpy(), want)
    assert recomputed == 0 and distance < 0.25
    bound.close()


def test_lane_independence_on_one_stream(be_toy_default, toy_default):
    """The same bound plan at two lane counts, back to back on one stream (the staging buffer and the workspace shrink in use, not
    in size): the lanes they share hold the same rows."""
    ks, ctx = toy_default
    nl, plan = _netlist_case()
    inputs = _inputs(ks, "toy_default")
    bound = plan.bind(be_toy_default)
    bound.run(_dev(inputs[:, :70]))
    wide = bound.arena
    bound.run(_dev(inputs[:, :5]))
    narrow = bound.arena
    assert bound.handle is not None
    assert np.array_equal(narrow.cpu().numpy(), wide.cpu().numpy()[:, :5])
    assert np.array_equal(wide.cpu().numpy(), _expected(ks, ctx, "toy_default")[:, :70])
    bound.close()


def test_stream_independence(be_toy_default, toy_default):
    import torch
    be = be_toy_default
    ks, ctx = toy_default
    nl, plan = _netlist_case()
    inputs = _dev(_inputs(ks, "toy_default")[:, :7])
    bound = plan.bind(be)
    bound.run(inputs)
    first = bound.arena.cpu().numpy()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        bound.run(inputs)
        second = bound.arena
        distance, recomputed = be.certify(reset=True)      # synchronises the side stream
    assert np.array_equal(second.cpu().numpy(), first)
    assert np.array_equal(first, _expected(ks, ctx, "toy_default")[:, :7])
    assert recomputed == 0 and distance < 0.2
    be.release_stream(s.cuda_stream)
    bound.close()


@pytest.mark.parametrize("arith_mode", ["fft"], indirect=True)
def test_argument_errors_leave_the_context_usable(be_toy_default, toy_default):
    be = be_toy_default
    ks, ctx = toy_default
    L, h = be.L, be.h
    nl, plan = _netlist_case()
    lanes = 2
    arena = be.empty(plan.wires, lanes, be.W)
    arena.fill_(0x5a5a5a5a)
    before = arena.cpu().numpy()
    handle = be.circuit_create(plan.table, plan.level_end, plan.n_inputs)
    pa = C.c_void_p(arena.data_ptr())
    assert L.rs_circuit_run_dev(h, handle, None, lanes, None) == -1 and L.rs_last_error()        # null arena
    assert L.rs_circuit_run_dev(h, None, pa, lanes, None) == -1                                   # null circuit
    assert L.rs_circuit_run_dev(h, handle, pa, 0, None) == 0                                      # lanes = 0: a no-op
    assert L.rs_circuit_run_dev(h, handle, pa, 2**61, None) == -1                                 # row arithmetic would overflow
    be.sync()
    assert np.array_equal(arena.cpu().numpy(), before)
    # refused tables create nothing
    bad = plan.table.copy()
    bad["op"][0] = 14
    out = C.c_void_p()
    ends = plan.level_end
    assert L.rs_circuit_create(h, C.byref(out), bad.ctypes.data_as(C.c_void_p), len(bad), ends.ctypes.data_as(C.POINTER(C.c_uint32)),
                               len(ends), plan.n_inputs) == -1 and not out.value
    assert b"op outside 0..13" in L.rs_last_error()
    assert L.rs_circuit_create(h, None, plan.table.ctypes.data_as(C.c_void_p), len(bad), ends.ctypes.data_as(C.POINTER(C.c_uint32)),
                               len(ends), plan.n_inputs) == -1
    # handle bookkeeping: a second destroy and a run after it are refused, not followed
    assert L.rs_circuit_destroy(h, handle) == 0
    assert L.rs_circuit_destroy(h, handle) == -1
    assert L.rs_circuit_run_dev(h, handle, pa, lanes, None) == -1
    assert L.rs_circuit_destroy(h, None) == -1
    be.sync()
    assert np.array_equal(arena.cpu().numpy(), before)
    # a circuit left alive is freed with its context; this context still computes
    be.circuit_create(plan.table, plan.level_end, plan.n_inputs)
    bound = plan.bind(be)
    bound.run(_dev(_inputs(ks, "toy_default")[:, :lanes]))
    assert np.array_equal(bound.arena.cpu().numpy(), _expected(ks, ctx, "toy_default")[:, :lanes])


# ---- the full default-128 key ----
FULL_BITS = 4
FULL_PAIRS = [(0, 0), (0, 1), (1, 0), (15, 15), (15, 1), (1, 15), (6, 11), (11, 6)]


def _full_inputs(ks):
    xa, xb = (np.array(v) for v in zip(*FULL_PAIRS))
    bits = np.stack([(x >> i) & 1 for x in (xa, xb) for i in range(FULL_BITS)])
    return xa, xb, _ref("full inputs", lambda: _encrypt_bits(ks, bits, 7000))


def _value(ks, ct):
    return sum(((ks.phase(ct[i]) > 0).astype(np.int64) << i) for i in range(ct.shape[0]))


@pytest.mark.parametrize("name,function", [("multiplier", "multiply"), ("maximum", "maximum")])
def test_full_key_multiply_and_maximum(be_full_default, full_default, name, function):
    from redsec_amd import arith, circuit
    be = be_full_default
    ks, ctx = full_default
    xa, xb, inputs = _full_inputs(ks)
    nl = getattr(circuit, name)(FULL_BITS)
    wires = _ref(("full", name), lambda: cr.oracle_wires(ctx, nl, inputs))
    a, b = _dev(inputs[:FULL_BITS]), _dev(inputs[FULL_BITS:])
    got = getattr(arith, function)(be, a, b).cpu().numpy()
    want_value = xa * xb if name == "multiplier" else np.maximum(xa, xb)
    assert got.shape == ((2 if name == "multiplier" else 1) * FULL_BITS, len(FULL_PAIRS), ks.W)
    assert np.array_equal(_value(ks, got), want_value)
    for k, w in enumerate(nl.outputs):
        assert not w.neg and np.array_equal(got[k], wires[w.node]), (name, k)
    bound = arith._plan(be, name, FULL_BITS)
    assert np.array_equal(bound.arena.cpu().numpy(), cr.expected_arena(bound.plan, inputs, wires))
