"""Keyswitch kernel time against the batch size, in the tiled and the wide form (RS_KS_FORM, rs_host.h keyswitch_form), on a key of
random words at the full width of the parameter set. One JSON line per (set, form, B); the median of `--reps` timed launches after
two warm-up launches, by torch events around Backend.keyswitch (the allocation of its output included, as in every caller).

usage: python tools/keyswitch_sweep.py [--sets default128,redsec_small_v2] [--batches 4096,16384,65536,131072] [--forms tiled,wide]
       REDSEC_HIP_LIB=variants/lib_X.so python tools/keyswitch_sweep.py ...      (a variant library, e.g. the sample-load probe)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import redsec_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="default128,redsec_small_v2")
    ap.add_argument("--batches", default="4096,16384,65536,131072")
    ap.add_argument("--forms", default="tiled,wide")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    rng = np.random.default_rng(16)
    for name in a.sets.split(","):
        p = redsec_amd.params(name)
        bk = np.zeros(p.n * 2 * p.bk_l * 2 * p.N, np.int32)
        ksk = rng.integers(-2**31, 2**31, p.N * p.ks_t * (1 << p.ks_basebit) * (p.n + 1), dtype=np.int32)
        for form in a.forms.split(","):
            os.environ["RS_KS_FORM"] = form          # read once, in rs_create
            be = redsec_amd.Backend(p, device=0)
            be.load_keys(bk, ksk)
            for B in (int(b) for b in a.batches.split(",")):
                u = torch.randint(-2**31, 2**31, (B, p.N + 1), dtype=torch.int32, device="cuda")
                ms = []
                for rep in range(a.reps + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = be.keyswitch(u)
                    e1.record()
                    e1.synchronize()
                    if rep >= 2:
                        ms.append(e0.elapsed_time(e1))
                print(json.dumps({"params": name, "W": p.n + 1, "forced": form, "ran": be.last_keyswitch(), "B": B,
                                  "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                  "checksum": int(out.sum(dtype=torch.int64).item()), "lib": os.environ.get("REDSEC_HIP_LIB", "")}), flush=True)
                del u, out
            be.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
