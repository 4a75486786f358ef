"""Directed inputs and certificate coverage of every blind-rotation form (tests/directed_rows.py has the rows and positions).

Part A: WHOLE batches against the oracle, word for word, in every form `Backend.last_launch()` can name. One input slab per
parameter set holds the directed rows (rotation exponents 0, 1, N-1, N, N+1, 2N-1; mod-switch ties; extreme words; trivial and
single-step rows) at the union of the positions where some form's bookkeeping changes (wave slots, last full and ragged group,
later sweeps of a persistent grid, both sides of the tail cut), fresh encryptions elsewhere. The oracle runs once per operation
on the whole slab; a case runs a prefix and compares with the slice.

Part B: the FFT mode is exact because every wave publishes the largest rounding distance it saw and that distance gates the
exact recomputation. A row whose masks are 0 runs no CMUX step and measures exactly 0.0 (tests/test_directed_cpu.py), so in a
batch of such rows with ONE ordinary ciphertext at row r the call's certificate is non-zero if and only if the wave(s) that own
row r publish -- a probe without a tolerance, run at every position of positions_for. The general-ring kernels are probed the
same way through rounding_certificate() in split mode. The split lock-step forms (split_coop, split_duo, split_workgroup)
publish no distance by design -- they rest on the a-priori bound of the split-key product -- and are not asserted on here.

Measured on an MI355X (profiles/r13/certificate_coverage.jsonl): the smallest distance of a batch with one active row, over all
forms and both toy sets, is recorded there per form; LIMIT below is at most that minimum / 1024 (and the tests assert so).
"""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import directed_rows as dr
import emu_lib
import oracle_lib as ol
from backend_pool import BackendPool
# the launch cases and what last_launch() must report for them (the CPU tests replay the same tables on the launch plan)
from directed_rows import BMAX, CASES, FFT_CASES, _B, _resident

pytestmark = pytest.mark.gpu

ALPHA = 2.0 ** -15
LIMIT = 2.0 ** -30          # the tiny certificate limit of part B: every call with one active row must be recomputed under it
E8 = 1 << 29
MU_SIGN = 1 << 20           # ol.to_torus(1, 4096)
LUT_FIRST = 3

POOL = BackendPool()
SEEN = set()                # form names part A has asserted
COVERAGE = {}               # part B: form -> figures for profiles/r13/certificate_coverage.jsonl
SETS = {"toy_default": "default128", "toy_redsec": "redsec_small_v2"}
GENERAL = {"toy_n2048": ("default128", 12), "toy_medium": ("redsec_medium", 13), "toy_large": ("redsec_large", 14)}


@pytest.fixture(scope="module", autouse=True)
def _close_module_contexts():
    yield
    POOL.close_all()


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()


def _make(ks, name):
    import torch
    import redsec_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = redsec_amd.params(name, n=ks.p.n)
    p.N = ks.p.N
    be = redsec_amd.Backend(p, device=0)
    be.load_keys(ks.bk, ks.ksk)
    return be


def _threads():
    return max(1, min(16, ol._cpu_share()))


def _wo_ks(ctx, x, mu):
    """Ctx.bootstrap_wo_ks is a per-row loop: rows are independent and the library call releases the interpreter lock."""
    with ThreadPoolExecutor(_threads()) as ex:
        return np.concatenate(list(ex.map(lambda part: ctx.bootstrap_wo_ks(part, mu), np.array_split(x, 8 * _threads()))))


def _luts(p, count, rng):
    luts = rng.integers(-2**31, 2**31, (count, p.N)).astype(np.int32)
    luts[0, ::5] = -2**31
    luts[1, 1::7] = 2**31 - 1
    luts[count - 1, :] = np.where(np.arange(p.N) % 2 == 0, -2**31, 2**31 - 1)
    return luts


@pytest.fixture(scope="module")
def num_cus(toy_default):
    with POOL.scratch(lambda: _make(toy_default[0], "default128")) as be:
        return be.info()["num_cus"]


class Slab:
    """Inputs a, b, c [Bmax][n+1] of one parameter set and the oracle's whole-slab result of every operation (computed once, on
    first use)."""

    def __init__(self, ks, ctx, Bmax, positions, seed):
        self.ks, self.ctx, self.B = ks, ctx, Bmax
        rng = np.random.default_rng(seed)
        self.rows, self.labels = dr.directed_rows(ks.p, rng)
        R = len(self.rows)
        positions = sorted(set(positions) | set(range(R)))          # every directed row once at the front, then round-robin
        fresh = [ks.encrypt(np.where(rng.integers(0, 2, Bmax) == 1, E8, -E8), ALPHA, seed + k) for k in range(3)]
        self.a, self.where = dr.embed(self.rows, Bmax, positions, fresh[0])
        self.b, _ = dr.embed(self.rows, Bmax, positions, fresh[1], shift=7)
        self.c, _ = dr.embed(self.rows, Bmax, positions[R:], fresh[2], shift=13)
        self.luts = _luts(ks.p, 7 if ks.p.bk_l == 3 else 5, rng)
        self._ref, self._dev = {}, {}

    def dev(self, which):
        if which not in self._dev:
            self._dev[which] = _dev(getattr(self, which))
        return self._dev[which]

    def ref(self, op):
        if op not in self._ref:
            ctx, a, b, c = self.ctx, self.a, self.b, self.c
            self._ref[op] = {
                "wo_ks": lambda: _wo_ks(ctx, a, E8),
                "bootstrap": lambda: ctx.bootstrap_batch(a, MU_SIGN),
                "XOR": lambda: ctx.gate_batch("XOR", a, b),
                "NAND": lambda: ctx.gate_batch("NAND", a, b),
                "gate_mu": lambda: ctx.bootstrap_batch(ol.gate_precombine("ORNY", a, b), -2**31),
                "mux": lambda: ctx.mux_batch(a, b, c),
                "lut": lambda: ctx.bootstrap_lut_batch(a, np.roll(self.luts, -LUT_FIRST, axis=0)),
            }[op]()
        return self._ref[op]

    def run(self, be, op, B):
        a, b, c = (self.dev(w)[:B] for w in "abc")
        if op == "wo_ks":
            return be.bootstrap_wo_ks(a, E8)
        if op == "bootstrap":
            return be.bootstrap(a, MU_SIGN)
        if op in ("XOR", "NAND"):
            return be.gate(op, a, b)
        if op == "gate_mu":
            return be.gate_mu("ORNY", a, b, -2**31)
        if op == "mux":
            return be.mux(a, b, c)
        return be.bootstrap_lut(a, self.dev("luts"), first=LUT_FIRST)


OPS = ["bootstrap", "wo_ks", "XOR", "NAND", "gate_mu", "mux", "lut"]
_SLABS = {}


def _slab(fixture, request, cus):
    if fixture not in _SLABS:
        ks, ctx = request.getfixturevalue(fixture)
        Bmax = _B(cus, BMAX)
        positions = set()
        for case, _ in CASES:
            if case[1] == fixture:
                positions |= set(dr.positions_for(case[4], _B(cus, case[3]), cus))
        _SLABS[fixture] = Slab(ks, ctx, Bmax, positions, seed=1300 + len(_SLABS))
    return _SLABS[fixture]


def _context(ks, name, switches, monkeypatch):
    """A scratch context created under the given launch switches (read once, in rs_create)."""
    for s in switches:
        monkeypatch.setenv(s, "1")
    cm = POOL.scratch(lambda: _make(ks, name))
    be = cm.__enter__()
    for s in switches:
        monkeypatch.delenv(s)
    return cm, be


# =====================================================================================================================
# Part A
# =====================================================================================================================
@pytest.mark.parametrize("case,mode", CASES, ids=[c[0] for c, _ in CASES])
def test_directed_rows_whole_batch_equals_the_oracle(case, mode, request, monkeypatch, num_cus):
    _, fixture, switches, bspec, form, waves, _ = case
    cus = num_cus
    slab = _slab(fixture, request, cus)
    B = _B(cus, bspec)
    assert B <= slab.B
    cm, be = _context(slab.ks, SETS[fixture], switches, monkeypatch)
    try:
        be.set_mode(mode)
        want = {"form": form, "waves_per_block": waves, "resident": _resident(case, B, cus)}
        planned, _ = emu_lib.launch_plan(dr.TRAITS[fixture, mode], slab.ks.p.n, B, be.info()["num_cus"], dr.switch_bits(switches))
        for op in OPS:
            got = slab.run(be, op, B)
            assert be.last_launch() == want, (op, be.last_launch())
            assert be.last_launch() == planned, (op, planned)
            got = got.cpu().numpy()
            ref = slab.ref(op)[:B]
            bad = np.nonzero((got != ref).any(axis=1))[0]
            assert bad.size == 0, (op, [(int(r), slab.labels[slab.where[r]] if r in slab.where else "fresh") for r in bad[:12]])
        assert be.fft_fallbacks() == 0
        if mode == "fft":
            dist, recomputed = be.certify()
            assert 0 < dist < 0.2 and recomputed == 0
        SEEN.add(form)
        if case[0].endswith("-tail"):
            # the cut-off rows ran in the latency form of their own size: reported by a call on exactly those rows
            tail = B % (8 * cus)
            got = be.bootstrap(slab.dev("a")[B - tail:B], MU_SIGN)
            assert be.last_launch()["form"] in ("coop8", "coop8_listed")
            assert np.array_equal(got.cpu().numpy(), slab.ref("bootstrap")[B - tail:B])
            assert {B - tail - 1, B - tail} <= set(dr.positions_for(form, B, cus))
    finally:
        cm.__exit__(None, None, None)


class GenSlab:
    """The general ring kernels' own slab: B = resident workgroups + 5 rows, so that some workgroups take a second ciphertext."""

    def __init__(self, toy):
        name, seed = GENERAL[toy]
        self.ks = ol.KeySet(ol.params(toy), seed=seed)
        self.ctx = ol.Ctx(self.ks)
        self.be = POOL.add(_make(self.ks, name))
        assert self.be.mode() == "split"
        p, rng = self.ks.p, np.random.default_rng(seed)
        self.cus = self.be.info()["num_cus"]
        probe = _dev(dr.identity_rows(p, 16 * self.cus + 1, rng))           # no CMUX step: costs nothing
        self.be.bootstrap(probe, E8)
        launch = self.be.last_launch()
        assert launch["form"] == "general"
        self.resident = launch["resident"]
        assert self.resident <= 16 * self.cus
        self.B = self.resident + 5
        self.rows, self.labels = dr.directed_rows(p, rng)
        self.positions = dr.positions_for("general", self.B, self.cus, sweep=self.resident)
        fresh = [self.ks.encrypt(np.where(rng.integers(0, 2, self.B) == 1, E8, -E8), 2.0 ** -20, seed + k) for k in range(3)]
        spots = sorted(set(self.positions) | set(range(len(self.rows))))
        self.a, self.where = dr.embed(self.rows, self.B, spots, fresh[0])
        self.b, _ = dr.embed(self.rows, self.B, spots, fresh[1], shift=7)
        self.c = fresh[2]
        self.luts = _luts(p, 5, rng)


_GEN = {}


def _gen(toy):
    if toy not in _GEN:
        _GEN[toy] = GenSlab(toy)
    return _GEN[toy]


@pytest.mark.parametrize("toy", sorted(GENERAL))
def test_directed_rows_on_the_general_ring_kernels(toy):
    g = _gen(toy)
    be, ctx, B = g.be, g.ctx, g.B
    a, b, c, luts = _dev(g.a), _dev(g.b), _dev(g.c), _dev(g.luts)
    want = {"form": "general", "waves_per_block": (g.ks.p.N // 16) // 64, "resident": g.resident}
    runs = [
        ("bootstrap", lambda: be.bootstrap(a, MU_SIGN), lambda: ctx.bootstrap_batch(g.a, MU_SIGN)),
        ("wo_ks", lambda: be.bootstrap_wo_ks(a, E8), lambda: _wo_ks(ctx, g.a, E8)),
        ("XOR", lambda: be.gate("XOR", a, b), lambda: ctx.gate_batch("XOR", g.a, g.b)),
        ("NAND", lambda: be.gate("NAND", a, b), lambda: ctx.gate_batch("NAND", g.a, g.b)),
        ("mux", lambda: be.mux(a, b, c), lambda: ctx.mux_batch(g.a, g.b, g.c)),
        ("lut", lambda: be.bootstrap_lut(a, luts, first=LUT_FIRST), lambda: ctx.bootstrap_lut_batch(g.a, np.roll(g.luts, -LUT_FIRST, axis=0))),
    ]
    for op, run, oracle in runs:
        got = run()
        assert be.last_launch() == want, op
        got, ref = got.cpu().numpy(), oracle()
        bad = np.nonzero((got != ref).any(axis=1))[0]
        assert bad.size == 0, (op, [(int(r), g.labels[g.where[r]] if r in g.where else "fresh") for r in bad[:12]])
    assert be.fft_fallbacks() == 0
    assert 0 < be.rounding_certificate(reset=True) < 0.25
    SEEN.add("general")


# =====================================================================================================================
# Part B
# =====================================================================================================================
class Probe:
    """A batch of identity rows of one parameter set, the oracle's result on it, and a few ordinary ciphertexts with theirs."""

    def __init__(self, ks, ctx, Bmax, seed):
        p, rng = ks.p, np.random.default_rng(seed)
        self.ks, self.ctx = ks, ctx
        self.ident = [dr.identity_rows(p, Bmax, rng) for _ in range(3)]
        self.ref_ident = ctx.bootstrap_batch(self.ident[0], E8)              # no CMUX step: the keyswitch alone costs
        self.ref_mux_ident = ctx.mux_batch(*self.ident)
        self.active = ks.encrypt([E8, -E8, E8, -E8, E8], ALPHA, seed + 1)
        assert dr.modswitch(p, self.active)[:, :p.n].all()                   # every step of an ordinary row is a real one
        self.ref_active = ctx.bootstrap_batch(self.active, E8)
        self.steps = np.concatenate([dr.step_rows(p, row) for row in self.active[:2]])       # step 0 alone, step n-1 alone
        self.ref_steps = ctx.bootstrap_batch(self.steps, E8)


_PROBES = {}


def _probe(fixture, request, Bmax):
    if fixture not in _PROBES:
        ks, ctx = request.getfixturevalue(fixture)
        _PROBES[fixture] = Probe(ks, ctx, Bmax, seed=1400 + len(_PROBES))
    return _PROBES[fixture]


def _note(key, **figures):
    rec = COVERAGE.setdefault(key, {"identity": [], "single_active": [], "single_step": [], "mux_second_rotation": []})
    for k, v in figures.items():
        rec[k].append(float(v))


@pytest.mark.parametrize("case", FFT_CASES, ids=[c[0] for c in FFT_CASES])
def test_every_wave_that_rounds_publishes_its_distance(case, request, monkeypatch, num_cus):
    """All-identity batch: distance exactly 0.0, nothing recomputed, outputs equal to the oracle. One ordinary ciphertext at row
    r, for every r of positions_for: distance > 0 (and >= 1024 LIMIT, what LIMIT was chosen by); under LIMIT exactly one more
    recomputed call and outputs equal to the oracle. The same with a row of one CMUX step (step 0 alone, step n-1 alone) and with
    a MUX whose first rotation is silent (a, b identity rows, c ordinary)."""
    import torch
    cid, fixture, switches, bspec, form, waves, _ = case
    cus = num_cus
    B = _B(cus, bspec)
    pr = _probe(fixture, request, _B(cus, BMAX))
    positions = dr.positions_for(form, B, cus)
    if cid.endswith("-tail"):
        cut = B - B % (8 * cus)
        assert {cut - 1, cut} <= set(positions)          # an active row in the main launch only, and in the cut-off launch only
    cm, be = _context(pr.ks, SETS[fixture], switches, monkeypatch)
    try:
        be.set_mode("fft")
        x, xb, xc = (_dev(v[:B]) for v in pr.ident)
        ident = x.clone()
        ref = _dev(pr.ref_ident[:B])
        ref_mux = _dev(pr.ref_mux_ident[:B])
        want = {"form": form, "waves_per_block": waves, "resident": _resident(case, B, cus)}
        be.certify(reset=True)
        count = be.fft_fallbacks()

        def call(run, limit=None):
            if limit is not None:
                be.set_certificate_limit(limit)
            try:
                out = run()
                dist, _ = be.certify(reset=True)
            finally:
                be.set_certificate_limit(0.25)
            return out, dist, be.fft_fallbacks()

        out, dist, n = call(lambda: be.bootstrap(x, E8))
        assert be.last_launch() == want
        assert dist == 0.0 and n == count and torch.equal(out, ref)
        out, dist, n = call(lambda: be.bootstrap(x, E8), LIMIT)                  # still nothing to recompute: 0.0 < LIMIT
        assert dist == 0.0 and n == count and torch.equal(out, ref)
        out, dist, n = call(lambda: be.mux(x, xb, xc))
        assert dist == 0.0 and n == count and torch.equal(out, ref_mux)
        _note(form, identity=dist)

        def one_active(r, row, ref_row, kind):
            nonlocal count
            x[r] = row
            ref[r] = ref_row
            out, dist, n = call(lambda: be.bootstrap(x, E8))
            assert dist > 0, (kind, r, "the wave(s) of this row published nothing")
            assert dist >= 1024 * LIMIT and dist < 0.2, (kind, r, dist)
            assert n == count and torch.equal(out, ref), (kind, r)
            _note(form, **{kind: dist})
            out, dist, n = call(lambda: be.bootstrap(x, E8), LIMIT)
            assert dist > 0 and n == count + 1 and torch.equal(out, ref), (kind, r, dist, n - count)
            count = n
            x[r] = ident[r]
            ref[r] = _dev(pr.ref_ident[r])

        for k, r in enumerate(positions):
            one_active(r, _dev(pr.active[k % len(pr.active)]), _dev(pr.ref_active[k % len(pr.active)]), "single_active")
        for k, r in enumerate(sorted({positions[0], positions[len(positions) // 2], positions[-1]})):
            for s in (0, 1):                                       # step 0 alone, step n-1 alone
                one_active(r, _dev(pr.steps[(2 * k + s) % 4]), _dev(pr.ref_steps[(2 * k + s) % 4]), "single_step")
        for k, r in enumerate(sorted({positions[0], positions[-1]})):
            xc[r] = _dev(pr.active[k])
            ref_mux[r] = _dev(pr.ctx.mux_batch(pr.ident[0][r:r + 1], pr.ident[1][r:r + 1], pr.active[k:k + 1])[0])
            out, dist, n = call(lambda: be.mux(x, xb, xc))
            assert dist > 0 and n == count and torch.equal(out, ref_mux), ("mux", r, dist)
            _note(form, mux_second_rotation=dist)
            out, dist, n = call(lambda: be.mux(x, xb, xc), LIMIT)
            assert dist > 0 and n == count + 1 and torch.equal(out, ref_mux), ("mux", r, dist, n - count)
            count = n
            xc[r] = _dev(pr.ident[2][r])
            ref_mux[r] = _dev(pr.ref_mux_ident[r])
        assert be.last_launch() == want
    finally:
        be.set_certificate_limit(0.25)
        cm.__exit__(None, None, None)


@pytest.mark.parametrize("toy", sorted(GENERAL))
def test_the_general_kernels_publish_for_every_resident_slot_and_sweep(toy):
    """Split mode on the general rings: rounding_certificate() is the running maximum the kernels publish on their own."""
    import torch
    g = _gen(toy)
    be, ctx, p = g.be, g.ctx, g.ks.p
    rng = np.random.default_rng(7)
    ident = dr.identity_rows(p, g.B, rng)
    active = g.ks.encrypt([E8, -E8, E8], 2.0 ** -20, 5)
    assert dr.modswitch(p, active)[:, :p.n].all()
    steps = dr.step_rows(p, active[0])
    ref_ident, ref_active, ref_steps = (ctx.bootstrap_batch(v, E8) for v in (ident, active, steps))
    x, ref = _dev(ident), _dev(ref_ident)
    be.rounding_certificate(reset=True)
    out = be.bootstrap(x, E8)
    assert be.last_launch()["form"] == "general"
    assert be.rounding_certificate(reset=True) == 0.0 and torch.equal(out, ref)
    _note("general", identity=0.0)
    trials = [(r, active[k % 3], ref_active[k % 3], "single_active") for k, r in enumerate(g.positions)]
    trials += [(r, steps[s], ref_steps[s], "single_step") for r in (g.positions[0], g.positions[-1]) for s in (0, 1)]
    for r, row, ref_row, kind in trials:
        x[r] = _dev(row)
        ref[r] = _dev(ref_row)
        out = be.bootstrap(x, E8)
        dist = be.rounding_certificate(reset=True)
        assert 0 < dist < 0.25, (kind, r, dist)
        assert torch.equal(out, ref), (kind, r)
        _note("general", **{kind: dist})
        x[r] = _dev(ident[r])
        ref[r] = _dev(ref_ident[r])
    # MUX: only the second rotation is active
    xb, xc = _dev(dr.identity_rows(p, g.B, rng)), _dev(dr.identity_rows(p, g.B, rng))
    r = g.positions[-1]
    be.mux(x, xb, xc)
    assert be.rounding_certificate(reset=True) == 0.0
    xc[r] = _dev(active[1])
    out = be.mux(x, xb, xc)
    dist = be.rounding_certificate(reset=True)
    assert 0 < dist < 0.25
    assert np.array_equal(out[r].cpu().numpy(), ctx.mux_batch(ident[r:r + 1], xb[r:r + 1].cpu().numpy(), active[1:2])[0])
    _note("general", mux_second_rotation=dist)


# =====================================================================================================================
# The listed coop8 step's guard and packing
# =====================================================================================================================
def test_more_steps_than_the_listed_step_holds_run_the_unlisted_coop8_kernel():
    """blind_rotate_coop8_listed_kernel packs a step as (i << 16) | bara into a list of kCoop8MaxSteps + 1 entries; the launcher
    sends a key with more steps to blind_rotate_coop8_kernel. A default-128-shaped context with n = kCoop8MaxSteps + 52 on a
    synthetic key (generated on the device; the oracle restates the generator): form coop8, three rows equal to the oracle."""
    import redsec_amd
    n, seed = 2048 + 52, 0xd17ec7ed
    p = ol.params("default128")
    p.n = n

    def make():
        be = redsec_amd.Backend(redsec_amd.params("default128", n=n), device=0)
        be.load_synthetic_keys(seed)
        return be

    class K:
        pass
    ks = K()
    ks.p = p
    ks.bk = ol.synthetic_key_words(seed, n * 2 * p.bk_l * 2 * p.N)
    ks.ksk = np.zeros(8, np.int32)                       # never read: only the blind rotation runs on the oracle
    ctx = ol.Ctx(ks)
    rng = np.random.default_rng(3)
    ct = rng.integers(-2**31, 2**31, (3, n + 1), dtype=np.int32)
    ct[1, 5:40] = 0                                      # identity steps: the listed form would skip them
    ct[2, :n] = dr.directed_rows(p, rng)[0][3, :n]       # every step rotates by N
    with POOL.scratch(make) as be:
        assert be.mode() == "fft"
        u = be.bootstrap_wo_ks(_dev(ct), E8)
        assert be.last_launch() == {"form": "coop8", "waves_per_block": 8, "resident": 1}
        assert np.array_equal(u.cpu().numpy(), ctx.bootstrap_wo_ks(ct, E8))
        assert be.fft_fallbacks() == 0
    ctx.close()


def test_more_steps_than_the_duo_kernel_holds_run_one_wave_per_ciphertext(num_cus):
    """blind_rotate_duo_kernel keeps the mod-switched mask words of its four ciphertexts in LDS, 640 per ciphertext (the shipped
    REDsec set has n = 350); rs_create accepts n up to 16,384. A REDsec-shaped context with n = 700 at a duo-sized batch must not
    take that kernel: form per_wave, sampled rows (first group, ragged last group) equal to the oracle."""
    import redsec_amd
    n, seed = 700, 0xd17ec7ee
    p = ol.params("redsec_small_v2")
    p.n = n

    def make():
        be = redsec_amd.Backend(redsec_amd.params("redsec_small_v2", n=n), device=0)
        be.load_synthetic_keys(seed)
        return be

    class K:
        pass
    ks = K()
    ks.p = p
    ks.bk = ol.synthetic_key_words(seed, n * 2 * p.bk_l * 2 * p.N)
    ks.ksk = np.zeros(8, np.int32)                       # never read: only the blind rotation runs on the oracle
    ctx = ol.Ctx(ks)
    B = 2 * num_cus + 5
    ct = np.random.default_rng(4).integers(-2**31, 2**31, (B, n + 1), dtype=np.int32)
    sample = np.r_[0, 1, B - 1]
    with POOL.scratch(make) as be:
        assert be.mode() == "fft"
        u = be.bootstrap_wo_ks(_dev(ct), E8)
        assert be.last_launch() == {"form": "per_wave", "waves_per_block": 2, "resident": 2 * num_cus}
        assert np.array_equal(u.cpu().numpy()[sample], ctx.bootstrap_wo_ks(ct[sample], E8))
        assert be.fft_fallbacks() == 0
    ctx.close()


# =====================================================================================================================
# Meta: every form has directed coverage
# =====================================================================================================================
def test_every_form_name_was_seen_with_directed_rows():
    """Runs last in this module. A form added to Backend.last_launch()'s list without a case above fails here."""
    import inspect
    import re
    import redsec_amd
    src = inspect.getsource(redsec_amd.Backend.last_launch)
    names = re.findall(r'"([a-z0-9_]+)"', src[src.index('"form": [') + len('"form": ['):src.index("][f.value]")])
    assert len(names) == 11 and sorted(names) == sorted(dr.FORMS)
    assert SEEN == set(names), sorted(set(names) ^ SEEN)
    assert set(COVERAGE) == {c[4] for c in FFT_CASES} | {"general"}
    out = os.environ.get("REDSEC_CERTIFICATE_COVERAGE_OUT")
    if out:
        with open(out, "w") as f:
            for form in sorted(COVERAGE):
                rec = {"form": form, "limit": LIMIT if form != "general" else None}
                for kind, v in COVERAGE[form].items():
                    rec[kind] = {"runs": len(v), "min": min(v), "max": max(v)} if v else None
                f.write(json.dumps(rec) + "\n")
