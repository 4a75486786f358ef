"""The packing key on the device (rs_pack_keygen_dev, rs_pack_expand_dev, rs_audit_pack_key_dev) on one MI355X: one JSON line per
parameter set, all five at their full size with keygen.pack_default digits (redsec_large: 1.0 GB of bodies, 2.0 GB expanded).

Times (HIP events on the current stream around the call, one untimed call, then the median and the extremes of --reps calls; the
generator and the audit are synchronous calls, so their times hold the private copy of the secret, the launch and the wait):
  keygen_ms            Backend.pack_keygen (pack_keygen_kernel); masked_adds = n t N^2, masked_adds_per_s = that over keygen_ms
  expand_ms            Backend.expand_packing_key (pack_expand_kernel); expand_bytes_per_s = the 8 n t N bytes written over expand_ms
  audit_seeded_ms      Backend.audit_packing_key on the bodies with the mask seed; audit_full_ms on the expanded key;
                       audit_adds = n t N popcount(S) rotated adds, audit_adds_per_s over audit_seeded_ms
  numpy_s_per_row      keygen.pack_key on the first 32 rows, on this box's CPUs (numpy_threads = OMP_NUM_THREADS, else the
                       process's CPUs); numpy_key_s = that times n t (an extrapolation)
The deviation is the set's rlwe_default_stdev, or 2^-30 where that truncates to zero. A last line (what = "compare") quotes the
best rate of rlwe_pk_encrypt_kernel (profiles/r19/rlwe_pk_time.jsonl) and of audit_bk_kernel (profiles/r11/key_audit_time.jsonl)
beside the best of this run: comparisons, not gates.

usage: python tools/pack_key_time.py [--reps 20] [--sets default128,redsec_large] [--out profiles/r21/pack_key_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = ("default128", "redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large")
NUMPY_ROWS = 32


def _times_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))


def _best(path, field, scale=1.0):
    try:
        vals = [json.loads(line).get(field) for line in open(os.path.join(ROOT, path)) if line.strip()]
    except OSError:
        return None
    vals = [v * scale for v in vals if isinstance(v, (int, float))]
    return max(vals) if vals else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", default=",".join(SETS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import keygen
    key_seed, mask_seed, noise_seed = bytes(range(32)), bytes(range(64, 96)), bytes(range(100, 132))
    lines = []

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    for name in args.sets.split(","):
        be = redsec_amd.Backend(redsec_amd.params(name), device=0)
        n, N = be.p.n, be.p.N
        basebit, t = keygen.pack_default(name)
        lwe, S = keygen.secret_keys(name, key_seed)
        try:
            stdev = keygen.rlwe_default_stdev(name)
        except ValueError:
            stdev = 2.0 ** -30
        limit = keygen.pack_noise_limit(stdev)
        body, full = be.empty(n, t, N), be.empty(n, t, 2, N)
        kg = _times_ms(lambda: be.pack_keygen(lwe, S, mask_seed, noise_seed, basebit, t, stdev, out=body), args.reps)
        ex = _times_ms(lambda: be.expand_packing_key(mask_seed, body, t, out=full), args.reps)
        report = {}
        seeded = _times_ms(lambda: report.update(be.audit_packing_key(lwe, S, body, basebit, t, mask_seed=mask_seed, limit=limit)), args.reps)
        report_full = {}
        whole = _times_ms(lambda: report_full.update(be.audit_packing_key(lwe, S, full, basebit, t, limit=limit)), args.reps)
        rows = np.arange(min(NUMPY_ROWS, n * t))
        t0 = time.perf_counter()
        want = keygen.pack_key(name, lwe, S, mask_seed, noise_seed, basebit, t, stdev, rows=rows)
        per_row = (time.perf_counter() - t0) / len(rows)
        same = bool(np.array_equal(body.view(n * t, N)[:len(rows)].cpu().numpy(), want))
        adds, audit_adds = n * t * N * N, n * t * N * int(S.sum())
        emit(dict(what="pack_key", set=name, n=n, N=N, basebit=basebit, t=t, rows=n * t, stdev=stdev, reps=args.reps,
                  body_bytes=4 * n * t * N, expanded_bytes=8 * n * t * N,
                  keygen_ms=kg["ms"], keygen_ms_min=kg["ms_min"], keygen_ms_max=kg["ms_max"], masked_adds=adds,
                  masked_adds_per_s=round(adds / (kg["ms"] * 1e-3), 1),
                  expand_ms=ex["ms"], expand_ms_min=ex["ms_min"], expand_ms_max=ex["ms_max"],
                  expand_bytes_per_s=round(8 * n * t * N / (ex["ms"] * 1e-3), 1),
                  audit_seeded_ms=seeded["ms"], audit_seeded_ms_min=seeded["ms_min"], audit_seeded_ms_max=seeded["ms_max"],
                  audit_full_ms=whole["ms"], audit_full_ms_min=whole["ms_min"], audit_full_ms_max=whole["ms_max"],
                  audit_adds=audit_adds, audit_adds_per_s=round(audit_adds / (seeded["ms"] * 1e-3), 1),
                  report=report, report_full=report_full, limit=limit,
                  numpy_rows=len(rows), numpy_s_per_row=round(per_row, 5), numpy_key_s=round(per_row * n * t, 2),
                  numpy_rows_equal_device=same, numpy_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0)))))
        del body, full
        be.close()
        torch.cuda.empty_cache()

    emit(dict(what="compare",
              pack_keygen_best_masked_adds_per_s=max(d["masked_adds_per_s"] for d in lines),
              rlwe_pk_encrypt_best_masked_adds_per_s=_best("profiles/r19/rlwe_pk_time.jsonl", "masked_adds_per_s"),
              audit_pack_best_adds_per_s=max(d["audit_adds_per_s"] for d in lines),
              audit_bk_best_adds_per_s=_best("profiles/r11/key_audit_time.jsonl", "audit_full_bk_Gadds_per_s", 1e9)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
