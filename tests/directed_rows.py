"""Directed LWE inputs of the blind rotation and the batch positions where its kernels' bookkeeping changes.

Test infrastructure (not a conftest; nothing under redsec_amd/ imports it). A blind rotation is a total function of the n + 1
ciphertext words, so every row here is an ordinary input: the words are chosen to land on the rotation exponents where the
index and the sign of X^bara wrap (0, 1, N-1, N, N+1, 2N-1), on the ties of the mod-switch to 2N (one below, on, one above
k q + q/2, the last of which rounds to 2N and wraps to 0), and on the extreme 32-bit words. With q = 2^32 / 2N the mod-switch
is bara = ((word + q/2) mod 2^33) >> log2 q, taken mod 2N by the rotation.
"""
import numpy as np


def q_of(p):
    return (1 << 32) // (2 * p.N)


def exponents(p):
    N = p.N
    return [0, 1, N - 1, N, N + 1, 2 * N - 1]


def _i32(words):
    return (np.asarray(words, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def ties(p):
    """(label, word, mirrored word) around the rounding ties k q + q/2 for k in {0, N-1, N, 2N-1}."""
    q, N = q_of(p), p.N
    out = []
    for k in (0, N - 1, N, 2 * N - 1):
        for d in (-1, 0, 1):
            out.append(("k%d%+d" % (k, d), k * q + q // 2 + d, k * q + q // 2 - d))
    return out


def modswitch(p, words):
    """bara of every word (the oracle's modSwitchFromTorus32 to 2N), reduced mod 2N as the rotation sees it."""
    q = q_of(p)
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    return ((w + q // 2) // q) % (2 * p.N)


def directed_rows(p, rng):
    """-> (int32 [R][n+1], labels). The rows the module docstring describes; `rng` only fills the single-step rows."""
    n, q = p.n, q_of(p)
    rows, labels = [], []

    def add(label, masks, b):
        r = np.zeros(n + 1, np.int64)
        r[:n] = masks
        r[n] = b
        rows.append(_i32(r)); labels.append(label)

    step0 = np.zeros(n, np.int64); step0[0] = 1
    last = np.zeros(n, np.int64); last[n - 1] = 1
    other = (np.arange(n) % 2 == 0).astype(np.int64)
    for e in exponents(p):                       # exponent rows: every mask word and the b word
        add("exp%d" % e, e * q, e * q)
    for e in exponents(p)[1:]:                   # ... on one step or every other step only
        add("exp%d_step0" % e, step0 * e * q, e * q)
        add("exp%d_last" % e, last * e * q, e * q)
        add("exp%d_alt" % e, other * e * q, e * q)
    for label, w, mirror in ties(p):             # tie rows
        add("tie_" + label, w, mirror)
    for label, w in (("minus1", -1), ("int_min", -2**31), ("int_max", 2**31 - 1), ("zero", 0)):
        add("all_" + label, w, w)                # extreme rows
    for e in exponents(p):                       # trivial rows: the initial rotation and the sample extraction alone
        add("trivial_exp%d" % e, 0, e * q)
    for label, w, _ in ties(p):
        add("trivial_tie_" + label, 0, w)
    for where, i in (("first", 0), ("mid", n // 2), ("last", n - 1)):     # single-step rows: bara != 0 at one index
        m = np.zeros(n, np.int64)
        m[i] = int(rng.integers(q, 2**32 - q))
        add("single_" + where, m, int(rng.integers(0, 2**32)))
    return np.stack(rows), labels


def identity_rows(p, count, rng):
    """Rows whose masks are 0 (no CMUX step runs: rounding distance exactly 0) with a random b word."""
    out = np.zeros((count, p.n + 1), np.int32)
    out[:, p.n] = _i32(rng.integers(0, 2**32, count))
    return out


def step_rows(p, row):
    """`row` cut down to its step 0 alone and to its step n-1 alone (b word kept) -> int32 [2][n+1]."""
    out = np.zeros((2, p.n + 1), np.int32)
    out[:, p.n] = row[p.n]
    out[0, 0] = row[0]
    out[1, p.n - 1] = row[p.n - 1]
    return out


def embed(rows, B, positions, filler, shift=0):
    """A batch [B][n+1]: `filler` ([B][n+1], fresh encryptions or identity rows) with the directed rows written at `positions`,
    taken round-robin from row `shift` on. -> (batch, {position: row index})."""
    out = np.array(filler[:B], dtype=np.int32, copy=True)
    assert out.shape[0] == B
    where = {}
    for k, pos in enumerate(sorted(set(int(x) for x in positions))):
        assert 0 <= pos < B
        where[pos] = (shift + k) % len(rows)
        out[pos] = rows[where[pos]]
    return out, where


FORMS = ["per_wave", "workgroup", "duo", "coop2", "coop4", "general", "split_workgroup", "split_coop", "split_duo", "coop8",
         "coop8_listed"]


def geometry(form, B, cus, group=None, sweep=None):
    """(rows per workgroup, rows per sweep of a persistent grid or None, first row of a cut-off tail launch or None) of a launch
    of `form` on B rows -- the rules of the launch plan (redsec_amd/csrc/rs_launch_plan.h) restated independently: its second
    opinion (tests/test_directed_cpu.py compares the two)."""
    cut = None
    if form in ("coop2", "coop4", "coop8", "coop8_listed", "split_coop"):
        g, s = 1, None                            # one ciphertext per workgroup, its waves share it
    elif form == "general":
        g, s = 1, None                            # persistent workgroups, one ciphertext at a time: `sweep` = resident ones
    elif form in ("duo", "split_duo"):
        g, s = 4, None
    elif form == "per_wave":
        g = 8 if B >= 8 * cus else 4 if B >= 4 * cus else 2 if B >= 2 * cus else 1
        s = 8 * cus if g == 8 else None           # eight waves per workgroup: one workgroup per CU, waves pull work
    elif form == "workgroup":
        g = 8 if B > 4 * cus else 4
        s = 8 * cus if g == 8 else None
        tail = B % (8 * cus)
        if g == 8 and B > 8 * cus and 0 < tail <= 4 * cus:
            cut = B - tail
    elif form == "split_workgroup":
        g = 8 if B > 4 * cus else 4
        s = g * cus
    else:
        raise KeyError(form)
    return (group or g), (sweep or s), cut


def positions_for(form, B, cus, group=None, sweep=None):
    """The batch positions that matter for `form`: every wave slot of the first group, the first and last slot of the last full
    group, every row of the ragged group, one row in each later sweep of a persistent grid (a different slot each time) and the
    rows either side of the tail cut. Sorted, unique, all < B."""
    g, s, cut = geometry(form, B, cus, group, sweep)
    pos = set(range(min(g, B)))
    full = B // g
    if full:
        pos |= {(full - 1) * g, full * g - 1}
    pos |= set(range(full * g, B))
    if s:
        for k in range(1, (B + s - 1) // s):
            pos.add(min(k * s + (k * 3 + 1) % g, B - 1))
    if cut is not None:
        pos |= {cut - 1, cut}
    pos.add(B - 1)
    if g == 1:
        pos.add(B // 2)                           # one ciphertext per workgroup: a workgroup in the middle of the grid as well
    return sorted(pos)


# ---- the launch cases: (switches set while the context is created, batch size in units of (#CUs, rows), form, waves) ----
def _B(cus, spec):
    return spec[0] * cus + spec[1]


BMAX = (8, 11)              # 8 x #CUs + 11: a second sweep of the persistent grids, and a tail of 11 rows that is cut off
FFT_CASES = [
    # id, fixture, switches, B, form, waves per workgroup, rows per sweep in #CUs (0: one row per workgroup)
    ("d-listed", "toy_default", (), (1, 0), "coop8_listed", 8, 0),
    ("d-listed-few", "toy_default", (), (0, 9), "coop8_listed", 8, 0),
    ("d-coop8", "toy_default", ("RS_NO_COOP8_LISTED",), (1, 0), "coop8", 8, 0),
    ("d-coop2", "toy_default", (), (1, 3), "coop2", 2, 0),
    ("d-wg4", "toy_default", (), (3, 2), "workgroup", 4, 4),
    ("d-wg8", "toy_default", (), (6, 5), "workgroup", 8, 8),
    ("d-tail", "toy_default", (), BMAX, "workgroup", 8, 8),
    ("d-sweeps", "toy_default", ("RS_NO_TAIL",), BMAX, "workgroup", 8, 8),
    ("d-perwave-persistent", "toy_default", ("RS_NO_WG",), BMAX, "per_wave", 8, None),
    ("d-perwave-nopersist", "toy_default", ("RS_NO_WG", "RS_NO_PERSIST"), BMAX, "per_wave", 8, None),
    ("d-perwave-2", "toy_default", ("RS_NO_WG4",), (3, 2), "per_wave", 2, None),
    ("d-perwave-1", "toy_default", ("RS_NO_COOP",), (1, 3), "per_wave", 1, None),
    ("r-coop8", "toy_redsec", (), (1, 0), "coop8", 8, 0),
    ("r-coop4", "toy_redsec", ("RS_NO_COOP8",), (1, 0), "coop4", 4, 0),
    ("r-coop2", "toy_redsec", (), (1, 3), "coop2", 2, 0),
    ("r-duo", "toy_redsec", (), (3, 2), "duo", 8, 4),
    ("r-perwave-2", "toy_redsec", ("RS_NO_DUO",), (3, 2), "per_wave", 2, None),
    ("r-wg8", "toy_redsec", (), (6, 5), "workgroup", 8, 8),
    ("r-tail", "toy_redsec", (), BMAX, "workgroup", 8, 8),
    ("r-sweeps", "toy_redsec", ("RS_NO_TAIL",), BMAX, "workgroup", 8, 8),
    ("r-perwave-persistent", "toy_redsec", ("RS_NO_WG",), BMAX, "per_wave", 8, None),
]
EXACT_CASES = [
    ("d-exact-coop2", "toy_default", (), (1, 3), "coop2", 2, 0),
    ("d-exact-perwave", "toy_default", (), BMAX, "per_wave", 8, None),
    ("r-exact-coop4", "toy_redsec", (), (1, 0), "coop4", 4, 0),
    ("r-exact-coop2", "toy_redsec", (), (1, 3), "coop2", 2, 0),
    ("r-exact-perwave-4", "toy_redsec", (), (6, 5), "per_wave", 4, None),
    ("r-exact-perwave", "toy_redsec", (), BMAX, "per_wave", 8, None),
]
SPLIT_CASES = [
    ("d-split-coop", "toy_default", (), (1, 0), "split_coop", 2, 0),
    ("d-split-duo", "toy_default", (), (3, 2), "split_duo", 8, 4),
    ("d-split-wg4", "toy_default", ("RS_NO_DUO",), (3, 2), "split_workgroup", 4, 4),
    ("d-split-wg8", "toy_default", (), (6, 5), "split_workgroup", 8, 8),
    ("d-split-sweeps", "toy_default", (), BMAX, "split_workgroup", 8, 8),
    ("r-split-coop4", "toy_redsec", (), (1, 0), "split_coop", 4, 0),
    ("r-split-coop2", "toy_redsec", (), (1, 3), "split_coop", 2, 0),
    ("r-split-duo", "toy_redsec", (), (3, 2), "split_duo", 8, 4),
    ("r-split-wg4", "toy_redsec", ("RS_NO_DUO",), (3, 2), "split_workgroup", 4, 4),
    ("r-split-wg8", "toy_redsec", (), (6, 5), "split_workgroup", 8, 8),
    ("r-split-sweeps", "toy_redsec", (), BMAX, "split_workgroup", 8, 8),
]
CASES = [(c, "fft") for c in FFT_CASES] + [(c, "exact") for c in EXACT_CASES] + [(c, "split") for c in SPLIT_CASES]


def _resident(case, B, cus):
    """What last_launch() must report as the ciphertexts of one key sweep."""
    form, waves, per_cu = case[4], case[5], case[6]
    if per_cu == 0:
        return 1
    if per_cu is None:                                   # per-wave kernel: the waves resident at once
        return min(B, waves * cus)
    groups = (B + per_cu - 1) // per_cu
    return per_cu * min(groups, cus)


# ---- the launch plan's inputs (redsec_amd/csrc/rs_launch_plan.h through emu_lib.launch_plan) ----
# FormTraits (workgroup_form, L, coop4, listed_cfg, split) of every (parameter set, mode) the launchers plan for: what
# form_traits (rs_bootstrap.h) fills in for the policy. test_gpu_directed.py compares the plan under these with the real launch.
TRAITS = {
    ("toy_default", "fft"): (1, 3, 0, 0, 0), ("toy_redsec", "fft"): (1, 10, 1, -1, 0),
    ("toy_default", "exact"): (0, 3, 0, -1, 0), ("toy_redsec", "exact"): (0, 10, 1, -1, 0),
    ("toy_default", "split"): (1, 3, 0, -1, 1), ("toy_redsec", "split"): (1, 10, 1, -1, 1),
    ("small_l3_bgbit10", "split"): (1, 3, 0, -1, 1),          # redsec_params_small's gadget: split mode only
}
TOY_N = {"toy_default": 24, "toy_redsec": 20}
# the switches of LaunchOpts that touch the blind rotation, in the bit order rs_emu_launch_plan takes them
SWITCHES = ["RS_NO_COOP", "RS_NO_WG", "RS_NO_DUO", "RS_NO_PERSIST", "RS_NO_WG4", "RS_NO_TAIL", "RS_NO_COOP8", "RS_NO_COOP8_LISTED",
            "RS_NO_COHORT"]
# the batch sizes where some form's rule changes (tools/stress_modes.py walks the same list on the device)
EDGES = [(0, 1), (0, 2), (1, -1), (1, 0), (1, 1), (2, 0), (2, 1), (4, 0), (4, 1), (8, -1), (8, 0), (8, 1), (12, 5), (16, 3), (24, 0)]


def switch_bits(switches):
    return sum(1 << SWITCHES.index(s) for s in switches)
