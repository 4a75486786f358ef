"""Directed inputs on the CPU: the rows of tests/directed_rows.py through the lane emulator of the device kernels (exact NTT
and FFT) against the oracle, word for word; the rounding-distance facts the GPU certificate-coverage tests rest on (a row
without a CMUX step measures exactly 0.0, a row with one step measures more); a self-check of positions_for; and the launch plan
(redsec_amd/csrc/rs_launch_plan.h through the emulator library): the GPU tests' case tables replayed on it and its invariants
swept over every boundary batch size, with geometry() as its independent second opinion."""
import itertools

import numpy as np
import pytest

import directed_rows as dr
import emu_lib
import oracle_lib as ol

SETS = [(0, "toy_default"), (1, "toy_redsec")]


def _rows(ks, seed=5):
    return dr.directed_rows(ks.p, np.random.default_rng(seed))


def test_directed_rows_hit_what_they_name(toy_default):
    ks, _ = toy_default
    p = ks.p
    rows, labels = _rows(ks)
    assert rows.dtype == np.int32 and rows.shape == (len(labels), p.n + 1) and len(set(labels)) == len(labels)
    bara = dr.modswitch(p, rows)
    N = p.N
    for e in dr.exponents(p):
        assert np.all(bara[labels.index("exp%d" % e)] == e)
        assert bara[labels.index("trivial_exp%d" % e)].tolist() == [0] * p.n + [e]
    r = bara[labels.index("exp%d_step0" % (N + 1))]
    assert r[0] == N + 1 and not r[1:p.n].any()
    r = bara[labels.index("exp%d_last" % (2 * N - 1))]
    assert r[p.n - 1] == 2 * N - 1 and not r[:p.n - 1].any()
    r = bara[labels.index("exp1_alt")]
    assert r[:p.n].tolist() == [1 - (i % 2) for i in range(p.n)]
    # ties: one below k q + q/2 stays at k, on it and one above round up; the top one wraps to 0
    for k in (0, N - 1, N, 2 * N - 1):
        got = [bara[labels.index("tie_k%d%+d" % (k, d))][0] for d in (-1, 0, 1)]
        assert got == [k, (k + 1) % (2 * N), (k + 1) % (2 * N)], (k, got)
        mirrored = [bara[labels.index("tie_k%d%+d" % (k, d))][p.n] for d in (-1, 0, 1)]
        assert mirrored == [(k + 1) % (2 * N), (k + 1) % (2 * N), k]
    assert not bara[labels.index("all_minus1")].any()                  # 0xFFFFFFFF rounds to 2N = 0
    assert np.all(bara[labels.index("all_int_min")] == N) and np.all(bara[labels.index("all_int_max")] == N)
    assert np.all(rows[labels.index("all_int_max")] == 2**31 - 1)
    for where, i in (("first", 0), ("mid", p.n // 2), ("last", p.n - 1)):
        r = bara[labels.index("single_" + where)][:p.n]
        assert r[i] != 0 and np.count_nonzero(r) == 1
    assert not dr.modswitch(p, dr.identity_rows(p, 9, np.random.default_rng(1)))[:, :p.n].any()


@pytest.mark.parametrize("cfg,fixture", SETS)
def test_directed_rows_through_the_emulator_equal_the_oracle(cfg, fixture, request):
    ks, ctx = request.getfixturevalue(fixture)
    n = ks.p.n
    rows, labels = _rows(ks)
    for mu in (ol.to_torus(1, 8), -2**31):
        ref = ctx.bootstrap_wo_ks(rows, mu)
        for i, label in enumerate(labels):
            u, _ = emu_lib.blind_rotate(cfg, n, rows[i], None, 1, 0, 0, mu, ks.bk)
            assert np.array_equal(u, ref[i]), ("ntt", label, mu)
            u, _, dev = emu_lib.blind_rotate_fft(cfg, n, rows[i], None, 1, 0, 0, mu, ks.bk)
            assert np.array_equal(u, ref[i]), ("fft", label, mu)
            assert 0.0 <= dev < 0.2, (label, dev)


@pytest.mark.parametrize("cfg,fixture", SETS)
def test_directed_rows_through_the_gate_precombination(cfg, fixture, request):
    """XOR (c = 2 on both inputs, constant 1/4) and NAND (c = -1, constant 1/8): the directed rows meet each other, paired with a
    shifted copy of themselves, so that the combined words wrap as well."""
    ks, ctx = request.getfixturevalue(fixture)
    n = ks.p.n
    rows, labels = _rows(ks)
    other = np.roll(rows, 7, axis=0)
    mu = ol.to_torus(1, 8)
    for op, c, bconst in (("XOR", 2, ol.to_torus(1, 4)), ("NAND", -1, ol.to_torus(1, 8))):
        ref = ctx.bootstrap_wo_ks(ol.gate_precombine(op, rows, other), mu)
        for i, label in enumerate(labels):
            u, _ = emu_lib.blind_rotate(cfg, n, rows[i], other[i], c, c, bconst, mu, ks.bk)
            assert np.array_equal(u, ref[i]), ("ntt", op, label)
            u, _, dev = emu_lib.blind_rotate_fft(cfg, n, rows[i], other[i], c, c, bconst, mu, ks.bk)
            assert np.array_equal(u, ref[i]), ("fft", op, label)


@pytest.mark.parametrize("cfg,fixture", SETS)
def test_identity_rows_measure_zero_and_one_step_measures_more(cfg, fixture, request):
    """What makes the certificate a probe without a tolerance: a row none of whose mask words mod-switches to a non-zero
    exponent runs no CMUX step, nothing is rounded, and its distance is exactly 0.0; one step already rounds N products."""
    ks, ctx = request.getfixturevalue(fixture)
    p, n = ks.p, ks.p.n
    rng = np.random.default_rng(5)
    rows, labels = dr.directed_rows(p, rng)
    mu = ol.to_torus(1, 8)

    def dist(row):
        return emu_lib.blind_rotate_fft(cfg, n, row, None, 1, 0, 0, mu, ks.bk)[2]
    silent = [l for l in labels if l.startswith("trivial_") or l in ("exp0", "all_zero", "all_minus1", "tie_k%d+0" % (2 * p.N - 1),
                                                                     "tie_k%d+1" % (2 * p.N - 1))]
    assert len(silent) >= 20
    for label in silent:
        assert dist(rows[labels.index(label)]) == 0.0, label
    for row in dr.identity_rows(p, 6, rng):
        assert dist(row) == 0.0
    for label in ("single_first", "single_mid", "single_last", "exp1_step0", "exp%d_last" % p.N):
        d = dist(rows[labels.index(label)])
        assert 1e-7 < d < 0.2, (label, d)
    ordinary = ks.encrypt([mu, -mu, mu], 2.0 ** -15, 77)
    for row in ordinary:
        assert 1e-5 < dist(row) < 0.2
        for cut in dr.step_rows(p, row):                     # its step 0 alone, its step n-1 alone
            assert np.count_nonzero(dr.modswitch(p, cut)[:n]) == 1
            assert 1e-7 < dist(cut) < 0.2


def test_embed_places_rows_round_robin(toy_default):
    ks, _ = toy_default
    rows, labels = _rows(ks)
    filler = dr.identity_rows(ks.p, 40, np.random.default_rng(2))
    batch, where = dr.embed(rows, 40, [3, 39, 17, 3], filler, shift=len(rows) - 1)
    assert sorted(where) == [3, 17, 39] and [where[k] for k in (3, 17, 39)] == [len(rows) - 1, 0, 1]
    for pos in range(40):
        assert np.array_equal(batch[pos], rows[where[pos]] if pos in where else filler[pos])


@pytest.mark.parametrize("cus", [256, 3])
def test_positions_cover_every_slot_and_group_class(cus):
    def pos(form, B, **kw):
        out = dr.positions_for(form, B, cus, **kw)
        assert out == sorted(set(out)) and 0 <= out[0] and out[-1] == B - 1
        return set(out)

    # lock-step groups of 8: every slot of the first group, both ends of the last full group, the whole ragged group
    B = 6 * cus + 5
    g = pos("workgroup", B)
    full = B // 8
    assert set(range(8)) <= g and {8 * full - 8, 8 * full - 1} <= g and set(range(8 * full, B)) <= g and len(g) < 8 + 2 + 8 + 2
    assert dr.geometry("workgroup", B, cus) == (8, 8 * cus, None)
    # more than one sweep of the persistent grid, and the cut-off tail launch
    B = 16 * cus + 11
    g = pos("workgroup", B)
    assert dr.geometry("workgroup", B, cus) == (8, 8 * cus, 16 * cus)
    assert {16 * cus - 1, 16 * cus} <= g and set(range(16 * cus + 8, B)) <= g
    assert any(8 * cus <= r < 16 * cus for r in g)
    sweeps = {r // (8 * cus) for r in g}
    assert sweeps == {0, 1, 2}
    assert dr.geometry("workgroup", 8 * cus + 4 * cus + 1, cus)[2] is None          # a tail too long to be cut
    # half-size groups, the duo forms
    for form, B in (("workgroup", 3 * cus + 2), ("duo", 3 * cus + 2), ("split_duo", 4 * cus - 1)):
        g = pos(form, B)
        assert dr.geometry(form, B, cus)[0] == 4
        full = B // 4
        assert set(range(4)) <= g and {4 * full - 4, 4 * full - 1} <= g and set(range(4 * full, B)) <= g
    # one ciphertext per workgroup
    for form in ("coop2", "coop4", "coop8", "coop8_listed", "split_coop"):
        assert pos(form, cus) == {0, cus // 2, cus - 1}
        assert pos(form, 1) == {0}
    # the per-wave kernel: 1, 2, 4 or 8 waves per workgroup by batch size; persistent beyond one workgroup per CU
    for B, slots in ((cus + 1, 1), (2 * cus + 1, 2), (4 * cus + 3, 4), (8 * cus + 5, 8)):
        assert dr.geometry("per_wave", B, cus)[0] == slots
        g = pos("per_wave", B)
        assert set(range(slots)) <= g and set(range(B // slots * slots, B)) <= g
    assert any(r >= 8 * cus for r in pos("per_wave", 8 * cus + 5))
    g = pos("split_workgroup", 16 * cus + 3)
    assert {r // (8 * cus) for r in g} == {0, 1, 2} and dr.geometry("split_workgroup", 3 * cus, cus)[0] == 4
    # the general kernel: `sweep` = its resident workgroups
    g = pos("general", 50, sweep=16)
    assert {0, 49} <= g and {r // 16 for r in g} == {0, 1, 2, 3}
    assert set(dr.FORMS) == {"per_wave", "workgroup", "duo", "coop2", "coop4", "general", "split_workgroup", "split_coop", "split_duo",
                             "coop8", "coop8_listed"}
    with pytest.raises(KeyError):
        dr.positions_for("no_such_form", 9, cus)


# =====================================================================================================================
# The launch plan
# =====================================================================================================================
@pytest.mark.parametrize("cus", [256, 3])
def test_the_launch_plan_replays_the_case_tables(cus):
    """test_gpu_directed.py's `last_launch() == want`, made on the CPU: form, waves and resident ciphertexts of every case."""
    for case, mode in dr.CASES:
        cid, fixture, switches, bspec, form, waves, _ = case
        # the tables give "k x #CUs and a few rows more", the few rows as a count that is meant to stay below one per CU (true on
        # every device the GPU tests see): on the 3-CU model it is cut down to that, or 9 rows alone would be 3 x #CUs
        B = dr._B(cus, (bspec[0], min(bspec[1], cus - 1)))
        info, steps = emu_lib.launch_plan(dr.TRAITS[fixture, mode], dr.TOY_N[fixture], B, cus, dr.switch_bits(switches))
        assert info == {"form": form, "waves_per_block": waves, "resident": dr._resident(case, B, cus)}, (cid, info)
        assert (steps[0]["form"], steps[0]["waves"]) == (form, waves)
        assert len(steps) == (2 if cid.endswith("-tail") else 1), cid
        if cid.endswith("-tail"):                              # the cut-off rows run as a call on exactly those rows would
            tail = B % (8 * cus)
            _, alone = emu_lib.launch_plan(dr.TRAITS[fixture, mode], dr.TOY_N[fixture], tail, cus, dr.switch_bits(switches))
            assert steps[1] == dict(alone[0], first=B - tail) and (alone[0]["form"] in ("coop8", "coop8_listed"))
        assert steps[0]["persistent"] == (cid.endswith("-perwave-persistent") or cid in ("d-exact-perwave", "r-exact-perwave")), cid


_PER_CU = ("workgroup", "duo", "split_workgroup", "split_duo")          # lock-step forms: at most one workgroup per CU


def _default_form(traits, n, B, cus):
    """(form, waves) of the main launch with no switch set, by batch size per CU: DESIGN.md's table of forms, restated."""
    wg, L, coop4, listed, split = traits
    four = coop4 and B <= cus
    if split:
        return ("split_coop", 4 if four else 2) if B <= 2 * cus else ("split_duo", 8) if B <= 4 * cus else ("split_workgroup", 8)
    if wg and B <= cus:
        return ("coop8_listed" if listed >= 0 and n <= 2048 else "coop8", 8)
    if B <= 2 * cus:
        return ("coop4", 4) if four else ("coop2", 2)
    if wg and B > 4 * cus:
        return ("workgroup", 8)
    if wg and L % 2 == 1:
        return ("workgroup", 4)
    if wg and n <= 640:
        return ("duo", 8)
    return ("per_wave", 8 if B >= 8 * cus else 4 if B >= 4 * cus else 2)


@pytest.mark.parametrize("cus", [256, 3])
def test_the_launch_plan_holds_its_invariants_at_every_boundary(cus):
    used_pairs = {tuple(case[2]) for case, _ in dr.CASES if len(case[2]) == 2}
    switch_sets = [()] + [(s,) for s in dr.SWITCHES] + sorted(used_pairs)
    assert ("RS_NO_WG", "RS_NO_PERSIST") in switch_sets
    seen = set()
    for (name, mode), traits in sorted(dr.TRAITS.items()):
        # beside the edge list: the longest tail that is cut off and the shortest that is not
        for switches, n, edge, offered in itertools.product(switch_sets, (10, 640, 641, 2048, 2049), dr.EDGES + [(12, 0), (12, 1)], (True, False)):
            B = dr._B(cus, edge)
            info, steps = emu_lib.launch_plan(traits, n, B, cus, dr.switch_bits(switches), offered)
            ctx = (name, mode, switches, n, B, steps)
            main = steps[0]
            assert (info["form"], info["waves_per_block"]) == (main["form"], main["waves"]), ctx
            if not switches:
                assert (main["form"], main["waves"]) == _default_form(traits, n, B, cus), ctx
            # the steps tile [0, B) exactly once, in order
            assert len(steps) in (1, 2) and main["first"] == 0 and sum(s["rows"] for s in steps) == B, ctx
            assert all(s["rows"] > 0 for s in steps) and steps[-1]["first"] == B - steps[-1]["rows"], ctx
            for s in steps:
                seen.add((s["form"], s["waves"]))
                assert s["block"] == 64 * s["waves"] and s["grid"] >= 1, ctx
                assert s["form"].startswith("split") == (mode == "split") and s["form"] != "general", ctx
                if s["form"] in _PER_CU or s["persistent"]:
                    assert s["grid"] <= cus, ctx
                if s["persistent"]:
                    assert s["form"] == "per_wave" and s["waves"] == 8 and "RS_NO_PERSIST" not in switches and s["rows"] > 8 * cus, ctx
                if s["form"] == "coop8_listed":
                    assert n <= 2048 and traits[3] >= 0, ctx
                if s["form"] == "duo":
                    assert n <= 640 and traits[1] % 2 == 0, ctx
                # every row has a wave (or, persistent / lock-step, a sweep that reaches it)
                g, sweep, _ = dr.geometry(s["form"], B if s is main else s["rows"], cus)
                if s["form"] == "per_wave":
                    assert s["persistent"] or s["grid"] * s["waves"] >= s["rows"], ctx
                else:
                    assert s["grid"] == min(-(-s["rows"] // g), cus if s["form"] in _PER_CU else s["rows"]), ctx
            # second opinion: rows per workgroup, rows per sweep and the cut position
            g, sweep, cut = dr.geometry(main["form"], B, cus)
            assert main["waves"] == (g if main["form"] in ("per_wave", "workgroup", "split_workgroup") else main["waves"]), ctx
            if main["form"] in _PER_CU:
                assert info["resident"] == g * main["grid"] and (sweep is None or info["resident"] == min(sweep, g * -(-main["rows"] // g))), ctx
            if main["form"] == "per_wave" and main["persistent"]:
                assert sweep == main["grid"] * main["waves"] == info["resident"], ctx
            if "RS_NO_TAIL" not in switches:
                assert (steps[1]["first"] if len(steps) == 2 else None) == cut, ctx
            if len(steps) == 2:
                tail = steps[1]
                assert main["form"] == "workgroup" and main["waves"] == 8 and B > 8 * cus and 0 < tail["rows"] <= 4 * cus, ctx
                assert tail["rows"] == B % (8 * cus) and not tail["cohort"] and info["resident"] == 8 * cus, ctx
            for s in steps:
                if s["cohort"]:
                    groups = -(-s["rows"] // s["waves"])
                    assert cus == 256 and offered and "RS_NO_COHORT" not in switches and groups > s["grid"], ctx
                    assert s["form"] in ("workgroup", "split_workgroup") and s["cohort_lag"] >= 1 and s["cohort_every"] in (1, 2), ctx
                    # the lag keeps a cohort within a third of an XCD's 4 MB L2: a step reads 2l rows (split: 4l half-rows) of 16 KB
                    step_bytes = (4 if mode == "split" else 2) * traits[1] * 16384
                    assert s["cohort_lag"] == max(1, (4 << 20) // 3 // step_bytes - 1), ctx
                    assert s["cohort_every"] == (2 if s["cohort_lag"] >= 4 else 1), ctx
                else:
                    assert s["cohort_every"] == 0 and s["cohort_lag"] == 0, ctx
    assert {f for f, _ in seen} == set(dr.FORMS) - {"general"}
    if cus == 256:                                             # cohorts are planned at all: whole-chip, more groups than grid
        _, steps = emu_lib.launch_plan(dr.TRAITS["toy_redsec", "split"], 20, 24 * cus, cus)
        assert steps[0]["cohort"] and (steps[0]["cohort_lag"], steps[0]["cohort_every"]) == (1, 1)
        _, steps = emu_lib.launch_plan(dr.TRAITS["toy_default", "fft"], 24, 24 * cus, cus)
        assert steps[0]["cohort"] and (steps[0]["cohort_lag"], steps[0]["cohort_every"]) == (13, 2)


@pytest.mark.parametrize("cus", [256, 3])
def test_a_cut_off_tail_on_the_per_wave_kernel_keeps_eight_waves(cus):
    """A tail that no latency or half-size form takes runs one wave per ciphertext with the WHOLE batch's eight waves per
    workgroup (by itself a batch of its size would take 1, 2 or 4) and without the work counter."""
    for (fixture, extra), tail_rows in itertools.product((("toy_default", "RS_NO_WG4"), ("toy_redsec", "RS_NO_DUO")), (1, cus, 2 * cus + 1, 4 * cus)):
        B = 8 * cus + tail_rows
        bits = dr.switch_bits(("RS_NO_COOP", extra))
        info, steps = emu_lib.launch_plan(dr.TRAITS[fixture, "fft"], dr.TOY_N[fixture], B, cus, bits)
        assert info == {"form": "workgroup", "waves_per_block": 8, "resident": 8 * cus} and len(steps) == 2
        tail = steps[1]
        assert (tail["form"], tail["waves"], tail["block"], tail["persistent"]) == ("per_wave", 8, 512, 0)
        assert (tail["first"], tail["rows"], tail["grid"]) == (8 * cus, tail_rows, -(-tail_rows // 8))
        alone, _ = emu_lib.launch_plan(dr.TRAITS[fixture, "fft"], dr.TOY_N[fixture], tail_rows, cus, bits)
        assert alone["form"] == "per_wave" and alone["waves_per_block"] == (4 if tail_rows >= 4 * cus else 2 if tail_rows >= 2 * cus else 1)
