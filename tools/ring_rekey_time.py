"""Ring re-keying (rs_ring_rekey_dev) on one MI355X, one JSON line each.

Times (HIP events on the current stream, one untimed call per shape, then the median and the extremes of --reps calls; random words
for key and ciphertexts: the arithmetic does not depend on the words):
  what = "rekey": R = 1 and R = 64 at default-128 with (2, 8) and at redsec_small_v2 with (4, 5), R = 1 at redsec_large with (4, 6)
      rekey_ms            Backend.ring_rekey (ring_rekey_init_kernel + ring_rekey_kernel)
      mads_per_s          R t 2 N^2 multiply-adds per call (one key word times one digit) over rekey_ms
      ceiling_mads_per_s  1,024 SIMDs x 64 lanes x 2.4 GHz / 4.3 cycles (v_mul_lo_u32 per wave64, MEASUREMENTS.md section 4.1) = 3.66e13
      workgroups          2 (N / 512) (N / 1024) t R

usage: python tools/ring_rekey_time.py [--reps 20] [--out profiles/r25/ring_rekey_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CEILING_MADS_PER_S = 1024 * 64 * 2.4e9 / 4.3
REKEY_SHAPES = (("default128", 2, 8, (1, 64)), ("redsec_small_v2", 4, 5, (1, 64)), ("redsec_large", 4, 6, (1,)))


def _stats(ts):
    return dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))


def _event_ms(fn, reps):
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
    return _stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import redsec_amd
    from redsec_amd import keygen
    rand = lambda *shape: torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0").to(torch.int32)
    lines = []

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    for name, basebit, t, counts in REKEY_SHAPES:
        be = redsec_amd.Backend(redsec_amd.params(name, n=16), device=0)     # the call needs no key: the ring is what matters
        N = be.p.N
        assert (basebit, t) == keygen.ring_rekey_default(name, "seeded")
        key = rand(t + 1, 2, N)
        for R in counts:
            rl, out = rand(R, 2, N), be.empty(R, 2, N)
            tm = _event_ms(lambda: be.ring_rekey(rl, key, basebit, t, out=out), args.reps)
            mads = R * t * 2 * N * N
            rate = mads / (tm["ms"] * 1e-3)
            emit(dict(what="rekey", set=name, N=N, basebit=basebit, t=t, R=R, rekey_ms=tm["ms"], rekey_ms_min=tm["ms_min"],
                      rekey_ms_max=tm["ms_max"], mads=mads, mads_per_s=round(rate, 1), ceiling_mads_per_s=round(CEILING_MADS_PER_S, 1),
                      fraction_of_ceiling=round(rate / CEILING_MADS_PER_S, 4), workgroups=2 * (N // 512) * (N // 1024) * t * R,
                      key_bytes=4 * (t + 1) * 2 * N, reps=args.reps))
        be.close()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
