"""Measurements of the three-input gates and the indexed gate batches, one JSON line each.

--noise: per parameter set, under a key from keygen.generate (the set's deviations), B random bit triples encrypted on the device;
  their gate outputs AND(x, x) are the "bootstrapped inputs". For MAJ3 and XOR3: the error of the inputs' COMBINED phase (sum_j c_j
  phase_j against its noise-free value), its standard deviation and margin / sigma (margin 1/8 resp. 1/4; also with the derived
  mod-switch rounding term sqrt((n/2 + 1) / 12) / (2N) of the next bootstrap added in quadrature), the smallest distance of a
  combined phase from 0 and 1/2, and the error of the gate's OUTPUT phase against +-1/8. Phases by rs_phase_dev. Recorded, not gated.
--time: default-128 under a generated key, FFT mode, device events around every step:
  gate       rs_gate_dev NAND at B = 65,536 (runs on any tree with Backend.gate: the parent commit's too, for the same-box A/B)
  gate_rows  rs_gate_rows_dev with one NAND group and the identity index on the same operands (trees that have it)
  add        arith.add of 8 bits over 4,096 lanes against the five-gate ripple adder built from rs_gate_dev (34 gate batches)
  The sha256 of each result goes into the line: the NAND words of the three variants must be the same.

usage: python tools/gate3_measure.py --noise [--sets default128,...] [--B 4096] [--out FILE]     (appends to FILE)
       python tools/gate3_measure.py --time [--label NAME] [--steps 12] [--out FILE]
       REDSEC_TREE=<checkout of another commit> REDSEC_HIP_LIB=<its library> python tools/gate3_measure.py --time --label parent ...
           the same steps with that commit's package and library (the A side of a same-box A/B: alternate the two commands)
"""
import argparse
import hashlib
import json
import math
import os
import statistics
import sys

ROOT = os.environ.get("REDSEC_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = ("default128", "redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large")
E8 = 1 << 29
COEF = {"MAJ3": (1, 1, 1), "XOR3": (-2, -2, -2), "MAJ3N": (-1, 1, 1)}
TRUTH = {"MAJ3": lambda a, b, c: (a + b + c >= 2) * 1, "XOR3": lambda a, b, c: a ^ b ^ c, "MAJ3N": lambda a, b, c: ((1 - a) + b + c >= 2) * 1}
MARGIN = {"MAJ3": 0.125, "XOR3": 0.25, "MAJ3N": 0.125}


def _signed(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def _stats(t):
    import numpy as np
    return dict(mean=float(t.mean()), std=float(t.std()), max_abs=float(np.abs(t).max()))


def noise(name, B):
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    p = be.p
    (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    sk, bk, ksk = keygen.generate(be, seed=bytes(range(60, 92)))
    del bk, ksk
    rng = np.random.default_rng(15)
    bits = rng.integers(0, 2, (3, B))
    enc = lambda v, first: be.encrypt_seeded(sk.lwe_key, torch.from_numpy(np.where(v, E8, -E8).astype(np.int32)).cuda(),
                                             bytes(range(32)), bytes(range(200, 232)), first=first, stdev=ks_stdev, full=True)[1]
    fresh = [enc(bits[j], j * B) for j in range(3)]
    level = [be.gate("AND", x, x) for x in fresh]                        # outputs of a previous gate level
    phases = [be.phase(x, sk.lwe_key).cpu().numpy().astype(np.int64) for x in level]
    ideal_in = [np.where(bits[j] == 1, E8, -E8).astype(np.int64) for j in range(3)]
    modswitch = math.sqrt((p.n / 2 + 1) / 12.0) / (2 * p.N)
    d = dict(what="gate3_noise", set=name, n=p.n, N=p.N, B=B, input_stdev=ks_stdev, bk_stdev=bk_stdev, ks_stdev=ks_stdev,
             inputs="AND(x, x) of fresh encryptions", modswitch_sigma_derived=modswitch,
             input_sigma=float(np.std(np.concatenate([_signed(ph - want) for ph, want in zip(phases, ideal_in)]) / 2.0 ** 32)))
    for op in ("MAJ3", "XOR3"):
        c = COEF[op]
        combined = _signed(sum(cj * ph for cj, ph in zip(c, phases)))
        ideal = _signed(sum(cj * w for cj, w in zip(c, ideal_in)))
        err = _signed(combined - ideal) / 2.0 ** 32
        truth = TRUTH[op](bits[0], bits[1], bits[2])
        assert np.array_equal((ideal > 0).astype(int), truth)
        edge = np.minimum(np.abs(combined), (1 << 31) - np.abs(combined)) / 2.0 ** 32
        out = be.gate3(op, *level)
        ph = be.phase(out, sk.lwe_key).cpu().numpy().astype(np.int64)
        out_err = _signed(ph - np.where(truth == 1, E8, -E8)) / 2.0 ** 32
        s = _stats(err)
        d[op] = dict(margin=MARGIN[op], combined_phase_error=s, margin_over_sigma=MARGIN[op] / s["std"],
                     margin_over_sigma_with_modswitch=MARGIN[op] / math.sqrt(s["std"] ** 2 + modswitch ** 2),
                     smallest_distance_from_a_boundary=float(edge.min()), output_phase_error=_stats(out_err),
                     wrong_outputs=int(((ph > 0).astype(int) != truth).sum()))
    d["device"] = torch.cuda.get_device_name(0)
    be.close()
    torch.cuda.empty_cache()
    return d


def _timed(fn, steps, warmup=2):
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, dict(steps=steps, median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def five_gate_add(be, a, b):
    """BinOps::add's sequence (lib/BinOps_enc.cpp:55-119) with every gate level one batch: 2 + 5 (bits - 2) + 2 gate batches."""
    bits = a.shape[0]
    out, carry = [], None
    for i in range(bits):
        t0 = be.gate("XOR", a[i], b[i])
        if carry is None:
            out.append(t0)
            carry = be.gate("AND", a[i], b[i])
            continue
        out.append(be.gate("XOR", carry, t0))
        if i + 1 < bits:
            carry = be.gate("OR", be.gate("AND", carry, t0), be.gate("AND", a[i], b[i]))
    return out


def times(label, steps):
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import keygen
    be = redsec_amd.Backend(redsec_amd.params("default128"), device=0)
    sk, bk, ksk = keygen.generate(be, seed=bytes(range(60, 92)))
    del bk, ksk
    assert be.mode() == "fft"
    lines = []
    B = 65536
    rng = np.random.default_rng(1)
    xa, xb = rng.integers(0, 2, B), rng.integers(0, 2, B)
    enc = lambda v, first: be.encrypt_seeded(sk.lwe_key, torch.from_numpy(np.where(v, E8, -E8).astype(np.int32)).cuda(),
                                             bytes(range(32)), bytes(range(200, 232)), first=first, stdev=2.0 ** -15, full=True)[1]
    ca, cb = enc(xa, 0), enc(xb, B)
    out = be.empty(B, be.W)
    res, t = _timed(lambda: be.gate("NAND", ca, cb, out=out), steps)
    assert np.array_equal(sk.decrypt_bits(res[:64].cpu().numpy()), (1 - (xa & xb))[:64])
    lines.append(dict(what="gate_rows_time", label=label, call="rs_gate_dev NAND", B=B, sha=_sha(res), **t))
    if hasattr(be, "gate_rows"):
        inp = torch.cat([ca, cb])
        r = torch.arange(B, dtype=torch.int32, device="cuda")
        idx = torch.stack([r, r + B, torch.full_like(r, -1)], 1).contiguous()
        res, t = _timed(lambda: be.gate_rows(inp, idx, [("NAND", B)], out=out), steps)
        lines.append(dict(what="gate_rows_time", label=label, call="rs_gate_rows_dev one NAND group, identity index", B=B, sha=_sha(res),
                          prepass_bytes=3 * B * be.W * 4, **t))
        del inp, idx
        from redsec_amd import arith
        lanes, bits = 4096, 8
        va, vb = rng.integers(0, 256, lanes), rng.integers(0, 256, lanes)
        a = torch.stack([enc((va >> i) & 1, 10 * B + i * lanes) for i in range(bits)])
        b = torch.stack([enc((vb >> i) & 1, 11 * B + i * lanes) for i in range(bits)])
        s, t_new = _timed(lambda: arith.add(be, a, b), max(3, steps // 2))
        value = sum(sk.decrypt_bits(s[i].cpu().numpy()) << i for i in range(bits + 1))
        assert np.array_equal(value, va + vb)
        s5, t_old = _timed(lambda: five_gate_add(be, a, b), max(3, steps // 2))
        value5 = sum(sk.decrypt_bits(s5[i].cpu().numpy()) << i for i in range(bits))
        assert np.array_equal(value5, (va + vb) % 256)
        lines.append(dict(what="adder_time", label=label, lanes=lanes, bits=bits, arith_add=dict(bootstraps=2 * bits * lanes, calls=bits, **t_new),
                          five_gate_ripple=dict(bootstraps=34 * lanes, calls=34, **t_old),
                          ratio_five_gate_over_arith=round(t_old["median_ms"] / t_new["median_ms"], 3)))
    for d in lines:
        d["device"] = torch.cuda.get_device_name(0)
    be.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--sets", default=",".join(SETS))
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.noise:
        for name in args.sets.split(","):
            lines.append(noise(name, args.B))
            print(json.dumps(lines[-1]), flush=True)
    if args.time:
        lines += times(args.label, args.steps)
        for d in lines:
            print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
