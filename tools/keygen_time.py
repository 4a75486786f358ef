"""Evaluation-key generation time per parameter set (one JSON line per measurement).

  device: rs_keygen_dev (redsec_amd.Backend.keygen) at every set's full size, the set's noise deviations; one untimed call
          first (code-object load), then the median of --reps synchronous calls (wall clock around the call, which ends with a
          device synchronisation). Also the time of rs_load_keys_dev for the generated key (the transform into the split domain).
  host:   client.SecretKeySet for default128 and redsec_small_v2 (numpy, one call each) as the comparison.

usage: python tools/keygen_time.py [--reps 5] [--out profiles/r08/keygen_time.jsonl] [--no-host]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
    seed = bytes(range(32))
    for name in SETS:
        be = redsec_amd.Backend(redsec_amd.params(name), device=0)
        (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
        lwe, tlwe = keygen.secret_keys(name, seed)
        bk, ksk = be.keygen(lwe, tlwe, seed, bk_stdev, ks_stdev)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            be.keygen(lwe, tlwe, seed, bk_stdev, ks_stdev, bk=bk, ksk=ksk)
            ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        be.load_keys_dev(bk, ksk)
        load_s = time.perf_counter() - t0
        p = be.p
        emit(dict(what="device_keygen", set=name, n=p.n, N=p.N, reps=args.reps, median_ms=round(1e3 * statistics.median(ts), 3),
                  min_ms=round(1e3 * min(ts), 3), bk_bytes=bk.numel() * 4, ksk_bytes=ksk.numel() * 4,
                  write_GBps=round((bk.numel() + ksk.numel()) * 4 / statistics.median(ts) / 1e9, 1),
                  load_keys_dev_ms=round(1e3 * load_s, 1), device=torch.cuda.get_device_name(0)))
        be.close()
        del bk, ksk
        torch.cuda.empty_cache()
    if not args.no_host:
        for name in ("default128", "redsec_small_v2"):
            t0 = time.perf_counter()
            client.SecretKeySet(name, seed=1)
            emit(dict(what="host_SecretKeySet", set=name, seconds=round(time.perf_counter() - t0, 2), cpus=os.cpu_count()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
