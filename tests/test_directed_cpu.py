"""Directed inputs on the CPU: the rows of tests/directed_rows.py through the lane emulator of the device kernels (exact NTT
and FFT) against the oracle, word for word; the rounding-distance facts the GPU certificate-coverage tests rest on (a row
without a CMUX step measures exactly 0.0, a row with one step measures more); and a self-check of positions_for."""
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
