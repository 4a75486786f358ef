"""The ring pipeline DECRYPTED on the large rings: rs_pack_dev, rs_circuit_bootstrap_dev / rs_ring_selector_dev, rs_ring_cmux_dev,
rs_ring_rekey_dev, rs_ring_lookup_dev and rs_rlwe_pk_encrypt_dev on redsec_medium (N = 4096) and redsec_large (N = 8192) with real
keys, every result decrypted on the host with tests/ring_truth.py (plain numpy from the definitions, nothing of the product) and
the host's copy of the secrets -- never with backend=be, where the device would decrypt its own work. The word tests of these
kernels (test_gpu_pack.py, test_gpu_ring_rekey.py, test_gpu_ring_cmux.py, test_gpu_ring_selector.py) hold the large rings against
numpy restatements in redsec_amd/keygen.py over random words; a convention that a kernel and its restatement share (a sign, the
order of the two selector families, a gadget level) passes there and fails here, because the ciphertexts stop decrypting. From
N = 2048 on the kernels have several source blocks, windows that start inside (-p, p), 8 and 16 tiles a polynomial and the
general-ring blind rotation; N = 2048 has no shipped set, hence no client keys, and stays covered by the word tests only.

Contexts are redsec_amd.params(name, n=16): key generation and every bootstrap cost 16 blind-rotation steps, and every formula
is evaluated at n = 16. The key seed is one whose LWE secret has n / 2 = 8 set bits, what pack_sigma's rounding term counts.

Shapes chosen by hand. keygen.circuit_bootstrap_default raises ValueError on both sets at every depth and step (INTEGRATION.md
section 24), and so does the same search with the formulas at n = 16: the sets' bootstrap output noise sigma_u (5.0e-5 and 7.0e-5)
is the rounding of their own LWE keyswitch (18 bits), which n does not change, and a CMUX under a produced selector multiplies it
by (N/2 - c)/2 at coefficient c. SHAPE = (5, 2, 8, 3) is what the default's search order (smallest l, then smallest ks_t, then
the (basebit, ks_basebit) of the smallest sigma) gives when its criterion "8 sigma of the worst coefficient inside step / 2" is
replaced by "sigma of the worst coefficient within 1 % of the least any shape reaches": 0.0790 / 0.112 (depth 1 / 2) on
redsec_medium and 0.213 / 0.302 on redsec_large at coefficient 0, the same shape for both depths and both sets. Key rows carry
keygen.ring_selector_default_stdev(name) = 2^-31 (the sets' own key noise truncates to zero).

What that noise allows. At slots 0 .. 63 one CMUX under a produced selector has sigma_c = 0.077 .. 0.079 (medium) and 0.210 ..
0.213 (large): the margin 1/8 of a +-1/8 bit is 1.6 and 0.6 sigma, and the 1/32 of a 1/16-step table row after a lookup of depth
2 is 0.3 and 0.1 sigma (4.2 and 2.2 sigma at the best coefficient, N/2 - 1). Reading bits off those phases is therefore not a
property these parameter sets have, whatever the kernels do. The three CMUXes of the chain (AND(1, 1), AND(1, 0), and the
public-key input under AND(1, 1)) do read their 64 bits and that is asserted: their sample errors w_0 + w_1 came out at 0.2 .. 0.7
sigma, and every word of the chain is seeded and exact, so the draw is the same on every run -- it says that THESE ciphertexts
decrypt, not that the next seed's will. The 64 selectors of the pooled statistic and the lookups are not read (the file prints how
many of their slots read right: 10,611 of 16,384 and 9,362 of 32,768 for the lookups). What is asserted everywhere is what
decryption shows about the kernels: every phase within 8 sigma_c of the phase of the ciphertext the bit chooses, and the pooled
variance inside the band of tests/test_ring_selector_cpu.py. The conventions themselves are pinned where noise leaves room: the
produced selector rows decrypt to the gadget rows (m h_j on X^0, -m h_j S) within 8 sigma of selector_row_sigma, which is 2^-14
against h_1 = 2^-10; and a CMUX under a client's selector of 2^-31 rows reads every bit of 29 ciphertexts.
"""
import numpy as np
import pytest

import ring_truth
from redsec_amd import arith, keygen

pytestmark = pytest.mark.gpu

RINGS = [("redsec_medium", 4096), ("redsec_large", 8192)]
N_LWE = 16
SHAPE = (5, 2, 8, 3)                                       # (basebit, l, ks_basebit, ks_t): the module docstring
SIGMA_K = 2.0 ** -31                                       # the deviation the key rows are made with


def _truncated_std(scale):
    """standard deviation of trunc(scale z), z ~ N(0, 1): the noise word of a row made with sigma = scale 2^-32"""
    z = np.linspace(-12.0, 12.0, 2_400_001)
    w = np.exp(-0.5 * z * z)
    v = np.trunc(scale * z)
    return float(np.sqrt((w * v * v).sum() / w.sum()))


# sigma_row / sigma_k of the formulas is the deviation of a row's PHASE. A noise word is sigma z truncated towards zero (TFHE's
# dtot32); at 2^-31 that is trunc(2 z), of deviation 1.66 words and not 2: the formulas are evaluated with what the rows carry
SIGMA_ROW = _truncated_std(SIGMA_K * 2.0 ** 32) / 2.0 ** 32
KEY_SEED = bytes(range(24, 56))                            # lwe secret of weight 8 at n = 16
OTHER_SEED = bytes(range(77, 109))
SEEDS = {k: bytes((b + 29 * i + 3) & 0xFF for b in range(32)) for i, k in enumerate(
    ("pack mask", "pack noise", "sel mask", "sel noise", "rekey mask", "rekey noise", "pk mask", "pk noise", "pk rand",
     "client mask", "client noise"))}
SLOTS = 64
GROUPS = 8                                                 # packed ciphertexts of 64 NAND results: the first two are the chain's, all
                                                           # eight the samples of the packing statistic (512: the band is 4.8 deviations)
POOL = 64                                                  # produced selectors of the pooled statistic, one independent draw each


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _bits_of(phase):
    return (np.asarray(phase, np.int32) > 0).astype(np.int64)


def _eighths(bits):
    return np.where(np.asarray(bits) != 0, 1 << 29, -(1 << 29)).astype(np.int32)


class _Ring:
    pass


@pytest.fixture(scope="module", params=RINGS, ids=[name for name, _ in RINGS])
def ring(request):
    """One context per ring with an evaluation key generated on the device, the keys of every step, two packed ciphertexts of 64
    NAND results each and their phases. Closed at the end."""
    import redsec_amd
    import torch
    name, N = request.param
    r = _Ring()
    r.name, r.N = name, N
    r.be = be = redsec_amd.Backend(redsec_amd.params(name, n=N_LWE), device=0)
    assert be.p.N == N and be.p.n == N_LWE
    r.sk, bk, ksk = keygen.generate(be, seed=KEY_SEED)
    del bk, ksk
    assert int(r.sk.lwe_key.sum()) == N_LWE // 2
    r.s, r.S = np.asarray(r.sk.lwe_key, np.int64), np.asarray(r.sk.tlwe_key, np.int64)
    r.sigma_u = keygen.bootstrap_sigma(name, n=N_LWE)
    assert keygen.ring_selector_default_stdev(name) == SIGMA_K
    # step 1: 2 x 64 NAND results, each 64 packed by its own call
    r.pack_shape = keygen.pack_default(name)
    pack_key = r.sk.packing_key(mask_seed=SEEDS["pack mask"], noise_seed=SEEDS["pack noise"], stdev=SIGMA_K, backend=be)
    assert (pack_key.basebit, pack_key.t) == r.pack_shape
    d_pack = be.upload_packing_key(pack_key)
    rng = np.random.default_rng(N)
    r.x, r.y = rng.integers(0, 2, (GROUPS, SLOTS)), rng.integers(0, 2, (GROUPS, SLOTS))
    ex, ey = _dev(r.sk.encrypt_bits(r.x.ravel(), seed=3)), _dev(r.sk.encrypt_bits(r.y.ravel(), seed=4))
    r.nand = be.gate("NAND", ex, ey)                                            # [512][n+1]
    every = torch.cat([be.pack(r.nand[k * SLOTS:(k + 1) * SLOTS].contiguous(), d_pack, *r.pack_shape) for k in range(GROUPS)])
    assert tuple(every.shape) == (GROUPS, 2, N)
    r.every, r.packed = every, every[:2].contiguous()
    r.phase_every = np.stack([ring_truth.rlwe_phase(ct, r.S) for ct in every.cpu().numpy()])
    r.phase_packed = r.phase_every[:2]
    # steps 2, 3, 5: ONE selector key at the shape's (ks_basebit, ks_t)
    basebit, l, ks_basebit, ks_t = SHAPE
    r.sel_key = r.sk.selector_key(ks_basebit, ks_t, SEEDS["sel mask"], SEEDS["sel noise"], stdev=SIGMA_K)
    r.d_sel_key = be.upload_selector_key(r.sel_key)
    r.cache = {}
    yield r
    be.close()
    torch.cuda.empty_cache()


def _and_bits(r, pairs, seed):
    """AND(u, v) of encrypted bit pairs, computed by the server -> [len(pairs)][n+1] at +-1/8"""
    uv = np.asarray(pairs, np.int64)
    eu, ev = _dev(r.sk.encrypt_bits(uv[:, 0], seed=seed)), _dev(r.sk.encrypt_bits(uv[:, 1], seed=seed + 1))
    return r.be.gate("AND", eu, ev)


def _issue_selectors(r):
    """the selectors of (u, v) = (1, 1) and (1, 0): bit = AND(u, v) from a gate, sel = circuit_bootstrap(bit) -> [2][2l][2][N]"""
    if "sel" not in r.cache:
        basebit, l, ks_basebit, ks_t = SHAPE
        r.cache["bits"] = _and_bits(r, [(1, 1), (1, 0)], seed=7)
        r.cache["sel"] = r.be.circuit_bootstrap(r.cache["bits"], basebit, l, r.d_sel_key, ks_basebit, ks_t)
    return r.cache["bits"], r.cache["sel"]


def _public_key_input(r):
    """one ring ciphertext of N bits at +-1/8 encrypted on the device under an RLWE public key of the ring secret, rows of 2^-31
    -> (the ciphertext [1][2][N], its phase under S, the bits)"""
    if "fresh" not in r.cache:
        pk = r.sk.rlwe_public_key(SEEDS["pk mask"], SEEDS["pk noise"], stdev=SIGMA_K)
        bits = np.random.default_rng(r.N + 1).integers(0, 2, r.N)
        fresh = r.be.rlwe_pk_encrypt(pk, _dev(_eighths(bits)), SEEDS["pk rand"], stdev=SIGMA_K)
        assert tuple(fresh.shape) == (1, 2, r.N)
        r.cache["fresh"] = (fresh, ring_truth.rlwe_phase(fresh.cpu().numpy()[0], r.S), bits)
    return r.cache["fresh"]


def _issue_cmux(r):
    """out = ring_cmux(packed[1], packed[0], sel) under the selectors of (1, 1) and (1, 0) -> (the two [1][2][N], their phases)"""
    if "cmux" not in r.cache:
        _, sel = _issue_selectors(r)
        outs = [r.be.ring_cmux(r.packed[1:], r.packed[:1], sel[k], SHAPE[0], SHAPE[1]) for k in range(2)]
        r.cache["cmux"] = (outs, [ring_truth.rlwe_phase(o.cpu().numpy()[0], r.S) for o in outs])
    return r.cache["cmux"]


def _sigma_c(r, bit, depth=1):
    basebit, l, ks_basebit, ks_t = SHAPE
    return keygen.circuit_bootstrap_sigma(r.N, N_LWE, basebit, l, ks_basebit, ks_t, r.sigma_u, SIGMA_ROW, depth=depth, bit=bit,
                                          coefficient=np.arange(r.N))


def test_packed_nand_results_decrypt_to_the_truth_table(ring):
    """Step 1. Slots 0 .. 63 of each packed ciphertext read NAND(x, y); the packing error, the slot's phase against the phase of
    the gate's output under the LWE secret, lies within 8 pack_sigma(n = 16, count = 64) and its rms within 15 % of it (the band
    of tests/test_pack_cpu.py). The two ciphertexts of the chain and six more of the same kind, so that the rms has 512 samples.
    Slots from 64 on are not looked at."""
    r = ring
    want = 1 - (r.x & r.y)
    before = ring_truth.lwe_phase(r.nand.cpu().numpy(), r.s).reshape(GROUPS, SLOTS)
    assert np.array_equal(_bits_of(before), want)
    sigma = keygen.pack_sigma(N_LWE, r.N, r.pack_shape[0], r.pack_shape[1], SLOTS, SIGMA_ROW)
    assert np.abs(ring_truth.error(before, _eighths(want))).max() < 8 * r.sigma_u
    err = ring_truth.error(r.phase_every[:, :SLOTS], before)
    ratio = float(np.sqrt(np.mean(err * err))) / sigma
    print("%s pack: rms / pack_sigma = %.3f (sigma %.3g), largest %.2f sigma" % (r.name, ratio, sigma, np.abs(err).max() / sigma))
    assert np.array_equal(_bits_of(r.phase_every[:, :SLOTS]), want)
    assert np.abs(err).max() < 8 * sigma
    assert abs(ratio - 1.0) < 0.15


def test_circuit_bootstrap_equals_its_three_calls_and_its_rows_decrypt_to_the_gadget(ring):
    """Step 2. rs_circuit_bootstrap_dev on a general ring (its scratch layout, its constant test polynomials h_j / 2 on the
    general-ring bootstrap_lut, the selector keyswitch from n_src = n) equals gather, bootstrap_lut and ring_selector word for
    word. Then the convention, with the real key: under S, row l + j of the selector of bit m has phase m h_j at X^0 and row j has
    -m h_j S(X), h_j = 2^(32-(j+1) basebit), every coefficient within 8 sigma of keygen.selector_row_sigma (the sample error w_j
    where the message sits, the key noise everywhere). h_j in place of h_j / 2 in the test polynomial puts 3 h_j / 2 or -h_j / 2
    there (hundreds of sigma at level 0, ten at level 1), and swapped families put the S multiple on the wrong rows."""
    r = ring
    be, N = r.be, r.N
    basebit, l, ks_basebit, ks_t = SHAPE
    bits, sel = _issue_selectors(r)
    rep = be.gather_rows(bits, _dev(np.repeat(np.arange(2), l)))
    half = np.array([1 << (31 - (j + 1) * basebit) for j in range(l)], np.int32)
    level = be.bootstrap_lut(rep, _dev(np.repeat(half[:, None], N, axis=1)))
    apart = be.ring_selector(level, basebit, l, r.d_sel_key, ks_basebit, ks_t)
    h_sel = sel.cpu().numpy()
    assert h_sel.shape == (2, 2 * l, 2, N) and np.array_equal(apart.cpu().numpy(), h_sel)
    # the level samples themselves: +-h_j / 2 under the LWE secret, within 8 sigma_u
    want_level = np.array([(2 * m - 1) * int(half[j]) for m in (1, 0) for j in range(l)], np.int64).astype(np.int32)
    assert np.abs(ring_truth.error(ring_truth.lwe_phase(level.cpu().numpy(), r.s), want_level)).max() < 8 * r.sigma_u
    sw, skey = keygen.selector_row_sigma(N_LWE, ks_basebit, ks_t, r.sigma_u, SIGMA_ROW)
    worst = 0.0
    for k, m in enumerate((1, 0)):
        for j in range(l):
            h = 1 << (32 - (j + 1) * basebit)
            on_b = np.zeros(N, np.int64)
            on_b[0] = m * h
            for row, want, where in ((h_sel[k, j], -m * h * r.S, r.S == 1), (h_sel[k, l + j], on_b, np.arange(N) == 0)):
                err = ring_truth.error(ring_truth.rlwe_phase(row, r.S), (want & 0xFFFFFFFF).astype(np.uint32))
                worst = max(worst, float(np.abs(err / np.sqrt(np.where(where, sw * sw, 0.0) + skey * skey)).max()))
    print("%s produced selector rows: worst |error| / sigma = %.2f (sigma_w %.3g, sigma_key %.3g)" % (r.name, worst, sw, skey))
    assert worst <= 8.0


def test_cmux_under_a_clients_selector_reads_every_bit_of_a_public_key_input(ring):
    """Step 6, and the CMUX where noise leaves room. One ring ciphertext of N bits at +-1/8 encrypted on the device under an RLWE
    public key of the ring secret (rows of 2^-31) decrypts to its bits, every error within 8 x 2^-31 sqrt(N + 1) (e u, e1 S and e2
    with u and S of weight about N / 2). It then goes through rs_ring_cmux_dev as d1 against packed ciphertext 0 under a client's
    selector of each bit at the shape's (basebit, l) and rows of 2^-31, in one call with the 28 pairs (d1, d0) = (packed j, packed
    i), i < j, of the eight packed ciphertexts: row 0 reads all N bits of the input for a selector of 1 and the 64 NAND results
    for a selector of 0, the other rows the 64 NAND results of j or of i; every phase lies within 8 ring_cmux_sigma of the chosen
    one's and the rms within 15 % of it (the band of tests/test_ring_cmux_cpu.py). 29 ciphertexts because the rounding term of a
    selector of 1 is -(r * S)(X) for the rounding errors r of x.a, and S = 1/2 (1 + X + .. + X^(N-1)) + (a +-1/2 polynomial): half
    of that term's energy sits in the few slowest modes of the ring, four fifths of that half in one, so the variance of ONE
    ciphertext scatters by 40 % and its rms by 20 %; over 29 the rms scatters by 3.7 % and the band is four of those."""
    import torch
    r = ring
    be, N = r.be, r.N
    basebit, l = SHAPE[:2]
    fresh, phase_fresh, bits = _public_key_input(r)
    err = ring_truth.error(phase_fresh, _eighths(bits))
    print("%s public-key input: largest error %.2f of 2^-31 sqrt(N + 1)" % (r.name, np.abs(err).max() / (SIGMA_K * np.sqrt(N + 1.0))))
    assert np.array_equal(_bits_of(phase_fresh), bits) and np.abs(err).max() < 8 * SIGMA_K * np.sqrt(N + 1.0)
    lo, hi = (list(v) for v in zip(*[(i, j) for i in range(GROUPS) for j in range(i + 1, GROUPS)]))
    d0 = torch.cat([r.packed[:1], r.every[lo]])
    d1 = torch.cat([fresh, r.every[hi]])
    nand = 1 - (r.x & r.y)
    phase_of = (np.concatenate([r.phase_every[:1], r.phase_every[lo]]), np.concatenate([phase_fresh[None], r.phase_every[hi]]))
    for m in (1, 0):
        sel = r.sk.ring_selector(m, 1, basebit, l, bytes(b ^ m for b in SEEDS["client mask"]), bytes(b ^ m for b in SEEDS["client noise"]),
                                 stdev=SIGMA_K)
        out = be.ring_cmux(d1, d0, sel).cpu().numpy()
        phase = np.stack([ring_truth.rlwe_phase(ct, r.S) for ct in out])
        sigma = keygen.ring_cmux_sigma(N, basebit, l, SIGMA_ROW, bit=m)
        err = ring_truth.error(phase, phase_of[m])
        ratio = float(np.sqrt(np.mean(err * err))) / sigma
        print("%s CMUX, client's selector of %d, %d ciphertexts: rms / ring_cmux_sigma = %.3f (sigma %.3g), largest %.2f sigma"
              % (r.name, m, len(out), ratio, sigma, np.abs(err).max() / sigma))
        if m:
            assert np.array_equal(_bits_of(phase[0]), bits)
        else:
            assert np.array_equal(_bits_of(phase[0, :SLOTS]), nand[0])
        assert np.array_equal(_bits_of(phase[1:, :SLOTS]), nand[hi if m else lo])
        assert np.abs(err).max() < 8 * sigma
        assert abs(ratio - 1.0) < 0.15


def test_cmux_under_bits_the_server_computed_follows_the_chosen_ciphertext(ring):
    """Steps 2, 3 and 6. For (u, v) = (1, 1) and (1, 0): bit = AND(u, v) from rs_gate_dev, its selector from
    rs_circuit_bootstrap_dev, out = ring_cmux(packed[1], packed[0], sel); then the public-key input as d1 against packed[0] under
    the selector of (1, 1). Every coefficient of out lies within 8 circuit_bootstrap_sigma(n = 16, bit = u & v, coefficient c) of
    the phase of the ciphertext that u & v chooses. Then the statistic: POOL = 64 further selectors from ANDs of random pairs, one
    CMUX each; the mean over the pool of mean_c(error_c^2 / sigma_c^2) lies inside the band of tests/test_ring_selector_cpu.py, four
    relative deviations sqrt(2 / draws) either side. That test counts every sample error w_j as a draw; at this shape and these
    rings three quarters of a selector's variance is the digits' mean, (w_0 + w_1) times ONE polynomial -(1 - T_c)/2, so a
    selector is one Gaussian draw and its ratio is distributed like chi^2_1: draws = POOL, 0.29 .. 1.71 in variance. Slots 0 .. 63
    of the three results of the chain read the 64 bits of the chosen ciphertext; the margin 1/8 is 1.6 (medium) and 0.6 (large)
    of these sigma_c, so that holds for these seeded draws and is not asked of the pool (the module docstring)."""
    r = ring
    be, N = r.be, r.N
    basebit, l, ks_basebit, ks_t = SHAPE
    _, sel = _issue_selectors(r)
    fresh, phase_fresh, fresh_bits = _public_key_input(r)
    outs, phases = _issue_cmux(r)
    third = be.ring_cmux(fresh, r.packed[:1], sel[0], basebit, l)
    phases = phases + [ring_truth.rlwe_phase(third.cpu().numpy()[0], r.S)]
    chosen = (r.phase_packed[1], r.phase_packed[0], phase_fresh)
    want_bits = (1 - (r.x[1] & r.y[1]), 1 - (r.x[0] & r.y[0]), fresh_bits[:SLOTS])
    for what, m, phase, before, want in zip(("AND(1, 1)", "AND(1, 0)", "AND(1, 1), public-key d1"), (1, 0, 1), phases, chosen, want_bits):
        sigma = _sigma_c(r, m)
        err = ring_truth.error(phase, before)
        right = int((_bits_of(phase[:SLOTS]) == want).sum())
        print("%s CMUX under %s: largest |error| / sigma_c = %.2f, mean error^2 / sigma_c^2 = %.3f, sigma_c(0) = %.3g, %d of %d slots read right"
              % (r.name, what, np.abs(err / sigma).max(), np.mean(err * err / sigma ** 2), sigma[0], right, SLOTS))
        assert (np.abs(err) < 8 * sigma).all(), (what, float(np.abs(err / sigma).max()))
        assert right == SLOTS, (what, right)                                  # these seeded draws read right: the module docstring
    # the pooled variance over POOL selectors
    rng = np.random.default_rng(N + 2)
    pairs = rng.integers(0, 2, (POOL, 2))
    pairs[:4] = ((1, 1), (1, 1), (0, 1), (0, 0))                              # both selector bits are in the pool
    bits = _and_bits(r, pairs, seed=21)
    sels = [be.circuit_bootstrap(bits[lo:lo + 16].contiguous(), basebit, l, r.d_sel_key, ks_basebit, ks_t) for lo in range(0, POOL, 16)]
    pool = be.empty(POOL, 2, N)
    for k in range(POOL):
        be.ring_cmux(r.packed[1:], r.packed[:1], sels[k // 16][k % 16], basebit, l, out=pool[k:k + 1])
    pool = pool.cpu().numpy()
    ratios = []
    for k, (u, v) in enumerate(pairs):
        err = ring_truth.error(ring_truth.rlwe_phase(pool[k], r.S), r.phase_packed[u & v])
        sigma = _sigma_c(r, int(u & v))
        assert (np.abs(err) < 8 * sigma).all(), (k, float(np.abs(err / sigma).max()))
        ratios.append(float(np.mean(err * err / sigma ** 2)))
    ratio = float(np.mean(ratios))
    band = 4 * np.sqrt(2.0 / POOL)
    print("%s CMUX under %d produced selectors: variance / formula = %.3f (rms / formula %.3f), band %.2f .. %.2f"
          % (r.name, POOL, ratio, np.sqrt(ratio), 1 - band, 1 + band))
    assert 1 - band <= ratio <= 1 + band


def test_ring_rekey_hands_the_results_to_a_recipient(ring):
    """Step 4. A recipient secret from another seed and a seeded ring key of keygen.ring_rekey_default(name) = (4, 6) with rows
    of 2^-31: the two CMUX results under the bits the server computed and the eight packed ciphertexts are re-keyed in one call
    (ten, because the rounding term scatters from ciphertext to ciphertext as in the CMUX under a client's selector). Under the
    recipient's secret the packed ones read the NAND truth table and the CMUX results the same 64 bits as under the source secret
    before the call; the re-keying error of every coefficient, recipient's phase against source's phase, lies within 8
    ring_rekey_sigma and its rms within 25 % of it (the band of tests/test_ring_rekey_cpu.py)."""
    import torch
    from redsec_amd import client
    r = ring
    be, N = r.be, r.N
    cmux_out, cmux_phase = _issue_cmux(r)
    other = client.SecretKeySet.from_secret(r.name, *keygen.secret_keys(r.name, OTHER_SEED, n=N_LWE))
    S2 = np.asarray(other.tlwe_key, np.int64)
    assert not np.array_equal(S2, r.S)
    basebit, t = keygen.ring_rekey_default(r.name)
    key = r.sk.ring_rekey_to(other, mask_seed=SEEDS["rekey mask"], noise_seed=SEEDS["rekey noise"], stdev=SIGMA_K)
    assert (key.basebit, key.t) == (basebit, t)
    src = torch.cat([r.every] + cmux_out)
    out = be.ring_rekey(src, key)
    assert tuple(out.shape) == (GROUPS + 2, 2, N)
    before = np.stack(list(r.phase_every) + cmux_phase)
    after = np.stack([ring_truth.rlwe_phase(ct, S2) for ct in out.cpu().numpy()])
    sigma = keygen.ring_rekey_sigma(N, basebit, t, SIGMA_ROW)
    err = ring_truth.error(after, before)
    ratio = float(np.sqrt(np.mean(err * err))) / sigma
    print("%s ring re-key (%d, %d): rms / ring_rekey_sigma = %.3f (sigma %.3g), largest %.2f sigma" % (r.name, basebit, t, ratio, sigma, np.abs(err).max() / sigma))
    assert np.array_equal(_bits_of(after[:GROUPS, :SLOTS]), 1 - (r.x & r.y))
    assert np.array_equal(_bits_of(after[GROUPS:, :SLOTS]), _bits_of(before[GROUPS:, :SLOTS]))
    assert np.abs(err).max() < 8 * sigma
    assert 0.75 < ratio < 1.25
    # not the source's secret any more: under S the re-keyed words are noise
    assert np.abs(ring_truth.error(ring_truth.rlwe_phase(out[0].cpu().numpy(), r.S), before[0])).max() > 0.25


def test_lookup_of_depth_two_follows_the_table_row(ring):
    """Step 5. A table of four trivial rows of random multiples of 1/16 (keygen.ring_trivial), the two index bits ANDs the server
    computed, arith.lookup for all four indices at SHAPE (the shape of depth 2 is the same: the module docstring). Every one of
    the N coefficients lies within 8 circuit_bootstrap_sigma(depth = 2, coefficient c) of table[index]. The formula is an upper
    bound here (the first level runs over plaintext rows, whose Da_j = 0), so the ratio is printed and held from above only (the
    CPU test of the lookup, tests/test_ring_selector_cpu.py, has the 8 sigma and no band): four deviations sqrt(2 / draws) of the
    4 x 2 selectors. Rounding the phases to sixteenths is beyond these sets (1/32 is at best 4.2 and 2.2
    sigma_c): how many slots read right is printed, not asserted."""
    r = ring
    be, N = r.be, r.N
    basebit, l, ks_basebit, ks_t = SHAPE
    values = np.random.default_rng(N + 3).integers(0, 16, (4, N))
    rows = (values << 28).astype(np.uint32).view(np.int32)
    table = _dev(keygen.ring_trivial(rows))
    sigma = _sigma_c(r, 1, depth=2)
    # index bits, LSB first, for indices 0 .. 3: bit k of index i = AND(1, (i >> k) & 1)
    bits = _and_bits(r, [(1, (i >> k) & 1) for i in range(4) for k in range(2)], seed=31).reshape(4, 2, N_LWE + 1)
    assert np.array_equal(_bits_of(ring_truth.lwe_phase(bits.cpu().numpy().reshape(8, -1), r.s)).reshape(4, 2),
                          [[(i >> k) & 1 for k in range(2)] for i in range(4)])
    worst, ratios, right = 0.0, [], 0
    for index in range(4):
        out = arith.lookup(be, bits[index].contiguous(), table, r.d_sel_key, basebit, l, ks_basebit, ks_t)
        assert tuple(out.shape) == (2, N)
        phase = ring_truth.rlwe_phase(out.cpu().numpy(), r.S)
        err = ring_truth.error(phase, rows[index])
        worst = max(worst, float(np.abs(err / sigma).max()))
        ratios.append(float(np.mean(err * err / sigma ** 2)))
        right += int(((((phase.view(np.uint32).astype(np.int64) + (1 << 27)) >> 28) & 15) == values[index]).sum())
        assert (np.abs(err) < 8 * sigma).all(), (index, float(np.abs(err / sigma).max()))
    ratio = float(np.mean(ratios))
    print("%s lookup of depth 2: largest |error| / sigma_c = %.2f, variance / formula = %.3f (an upper bound), %d of %d slots read right"
          % (r.name, worst, ratio, right, 4 * N))
    assert ratio <= 1 + 4 * np.sqrt(2.0 / (4 * 2))
