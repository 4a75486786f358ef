"""Measurements of the compiled circuits, one JSON line each. default-128 under a generated key, FFT
mode, device events around every call.

--time:
  add        8-bit addition over 4,096 lanes: arith.add (one rs_gate_rows_dev call per bit, index tables in torch) against the same
             sixteen cells through a compiled plan (circuit.adder: one rs_circuit_run_dev call). Both run the same 16 x lanes
             rotations, so the difference is the pre-pass and the host loop. The sum words of the two must be the same (sha256).
  multiply   8 x 8 bits over 1,024 lanes (arith.multiply), with the plan's cells, rotations and depth
  maximum    8 bits over 4,096 lanes (arith.maximum)
--kernels WORKLOAD: runs one of the three workloads five times and nothing else, to be put under `rocprofv3 --kernel-trace --stats`
--fold FILE: the share of circuit_rows_kernel and circuit_fold_kernel in the kernel time of such a run's *_kernel_stats.csv

usage: python tools/circuit_measure.py --time [--steps 5] [--out FILE]     (appends to FILE)
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/circuit_measure.py --kernels multiply
       python tools/circuit_measure.py --fold DIR/.../..._kernel_stats.csv --label multiply [--out FILE]
"""
import argparse
import csv
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E8 = 1 << 29
SHAPES = {"add": (8, 4096), "multiply": (8, 1024), "maximum": (8, 4096)}


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


class Bench:
    def __init__(self):
        import numpy as np
        import torch
        import redsec_amd
        from redsec_amd import keygen
        self.np, self.torch = np, torch
        self.be = redsec_amd.Backend(redsec_amd.params("default128"), device=0)
        self.sk, bk, ksk = keygen.generate(self.be, seed=bytes(range(60, 92)))
        del bk, ksk
        assert self.be.mode() == "fft"
        self.rng = np.random.default_rng(17)
        self.first = 0

    def operands(self, bits, lanes):
        np, torch = self.np, self.torch
        values = [self.rng.integers(0, 1 << bits, lanes) for _ in range(2)]
        cts = []
        for v in values:
            rows = []
            for i in range(bits):
                mu = torch.from_numpy(np.where((v >> i) & 1, E8, -E8).astype(np.int32)).cuda()
                rows.append(self.be.encrypt_seeded(self.sk.lwe_key, mu, bytes(range(32)), bytes(range(200, 232)), first=self.first,
                                                   stdev=2.0 ** -15, full=True)[1])
                self.first += lanes
            cts.append(torch.stack(rows))
        return values, cts

    def value(self, ct):
        return sum(self.sk.decrypt_bits(ct[i].cpu().numpy()).astype(self.np.int64) << i for i in range(ct.shape[0]))

    def workload(self, name):
        """(callable, check of its result, facts)"""
        from redsec_amd import arith, circuit
        np = self.np
        bits, lanes = SHAPES[name]
        (va, vb), (a, b) = self.operands(bits, lanes)
        if name == "add":
            plan = circuit.adder(bits).compile()
            bound = plan.bind(self.be)
            inputs = self.torch.cat([a, b])
            fn = lambda: bound.run(inputs)
            want = va + vb
            self.parent_add = (lambda: arith.add(self.be, a, b))
        else:
            plan = arith._plan(self.be, "multiplier" if name == "multiply" else "maximum", bits).plan
            fn = (lambda: arith.multiply(self.be, a, b)) if name == "multiply" else (lambda: arith.maximum(self.be, a, b))
            want = va * vb if name == "multiply" else np.maximum(va, vb)
        facts = dict(bits=bits, lanes=lanes, cells=plan.cells, rotations=plan.rotations, depth=plan.depth,
                     bootstraps=plan.rotations * lanes, widest_level_rows=max(c + m for _, c, m in plan.levels()) * lanes)
        return fn, (lambda out: bool(np.array_equal(self.value(out), want))), facts


def times(steps):
    bench = Bench()
    torch = bench.torch
    lines = []
    for name in ("add", "multiply", "maximum"):
        fn, check, facts = bench.workload(name)
        out, t = _timed(fn, steps)
        assert check(out), name
        d = dict(what="circuit_time", workload=name, **facts, plan=t, ms_per_1000_bootstraps=round(1000 * t["median_ms"] / facts["bootstraps"], 4))
        if name == "add":
            ref, t_ref = _timed(bench.parent_add, steps)
            assert check(ref) and _sha(ref) == _sha(out), "the plan's sum words differ from arith.add's"
            d.update(arith_add=t_ref, sha=_sha(out), plan_minus_arith_add_ms=round(t["median_ms"] - t_ref["median_ms"], 3),
                     ratio_plan_over_arith_add=round(t["median_ms"] / t_ref["median_ms"], 4))
        d["device"] = torch.cuda.get_device_name(0)
        lines.append(d)
        print(json.dumps(d), flush=True)
    bench.be.close()
    return lines


def kernels(name):
    bench = Bench()
    fn, check, facts = bench.workload(name)
    for _ in range(5):
        out = fn()
    bench.torch.cuda.synchronize()
    assert check(out), name
    bench.be.close()


def fold(path, label):
    rows = list(csv.DictReader(open(path)))
    total = sum(int(r["TotalDurationNs"]) for r in rows)
    pick = lambda key: sum(int(r["TotalDurationNs"]) for r in rows if key in r["Name"])
    calls = lambda key: sum(int(r["Calls"]) for r in rows if key in r["Name"])
    pre, fol = pick("circuit_rows_kernel"), pick("circuit_fold_kernel")
    run = pre + fol + pick("blind_rotate") + pick("keyswitch")
    return dict(prepass_and_fold_share_of_the_runs=round((pre + fol) / run, 5) if run else None, what="circuit_kernel_share", workload=label, kernel_time_ms=round(total / 1e6, 3),
                circuit_rows_ms=round(pre / 1e6, 3), circuit_rows_calls=calls("circuit_rows_kernel"),
                circuit_fold_ms=round(fol / 1e6, 3), circuit_fold_calls=calls("circuit_fold_kernel"),
                blind_rotation_ms=round(pick("blind_rotate") / 1e6, 3), keyswitch_ms=round(pick("keyswitch") / 1e6, 3),
                note="kernel_time_ms is the whole process (key generation and encryption included); the share is taken of the "
                     "circuit, blind-rotation and keyswitch kernels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--kernels", choices=sorted(SHAPES))
    ap.add_argument("--fold")
    ap.add_argument("--label", default="")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.time:
        lines += times(args.steps)
    if args.kernels:
        kernels(args.kernels)
    if args.fold:
        lines.append(fold(args.fold, args.label))
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
