"""Circuit bootstrapping (rs_ring_selector_dev, rs_circuit_bootstrap_dev) on one MI355X, one JSON line each.

Times (HIP events on the current stream, one untimed call per shape, then the median and the extremes of --reps calls) on
redsec_small_v2 (n = 350, N = 1024) with an evaluation key generated on the device, at depth 1, 3 and 10:
  what = "selector": rs_ring_selector_dev alone over random words (the arithmetic does not depend on the words), at the set's
      default shape (keygen.circuit_bootstrap_default: l = 3, ks_t = 3) and at (ks_basebit, ks_t) = (4, 6), the 34 MB key
      selector_ms         ring_selector_init_kernel + ring_selector_kernel
      key_bytes           2 (n + 1) ks_t 8 N
      key_stream_ms       key_bytes / 8 TB/s, the HBM3E rate of the part: what one pass over the key costs at best
      key_stream_copy_ms  key_bytes / 6.3 TB/s, what a plain vector copy reaches on this part
      key_passes          row blocks of eight: each reads the whole key again
      workgroups          4 (N / 512) ceil((n + 1) / 8) ceil(depth l / 8)
  what = "circuit_bootstrap": rs_circuit_bootstrap_dev through the C ABI with its scratch allocated beforehand, over encrypted
      bits: the gather, ONE programmable bootstrap of depth l rows and the selector keyswitch
      circuit_bootstrap_ms, and bootstrap_ms of Backend.bootstrap_lut over as many rows beside it

usage: python tools/ring_selector_time.py [--reps 20] [--out profiles/r27/ring_selector_time.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
COPY_BYTES_PER_S = 6.3e12
NAME = "redsec_small_v2"
DEPTHS = (1, 3, 10)


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
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import keygen
    rand = lambda *shape: torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0").to(torch.int32)
    lines = []

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    be = redsec_amd.Backend(redsec_amd.params(NAME), device=0)
    sk, bk, ksk = keygen.generate(be, seed=bytes(range(19, 51)))
    del bk, ksk
    N, n = be.p.N, be.p.n
    basebit, l, dkb, dkt = keygen.circuit_bootstrap_default(NAME)
    vp = lambda t: C.c_void_p(t.data_ptr())
    for ks_basebit, ks_t in ((dkb, dkt), (4, 6)):
        key = rand(2, n + 1, ks_t, 2, N)
        key_bytes = key.numel() * 4
        for depth in DEPTHS:
            rows = depth * l
            ct, out = rand(rows, n + 1), be.empty(depth, 2 * l, 2, N)
            tm = _event_ms(lambda: be.ring_selector(ct, basebit, l, key, ks_basebit, ks_t, out=out), args.reps)
            passes = -(-rows // 8)
            emit(dict(what="selector", set=NAME, N=N, n_src=n, depth=depth, basebit=basebit, l=l, ks_basebit=ks_basebit, ks_t=ks_t, rows=rows,
                      selector_ms=tm["ms"], selector_ms_min=tm["ms_min"], selector_ms_max=tm["ms_max"], key_bytes=key_bytes,
                      key_stream_ms=round(key_bytes / HBM_BYTES_PER_S * 1e3, 4), key_stream_copy_ms=round(key_bytes / COPY_BYTES_PER_S * 1e3, 4), key_passes=passes,
                      key_bytes_per_s=round(key_bytes * passes / (tm["ms"] * 1e-3), 1),
                      workgroups=4 * (N // 512) * -(-(n + 1) // 8) * passes, reps=args.reps))
            if (ks_basebit, ks_t) != (dkb, dkt):
                continue
            bits = torch.from_numpy(sk.encrypt_bits(np.arange(depth) & 1, seed=11)).to("cuda:0")
            scratch = be.empty(l * N + rows * (2 * (n + 1) + 1))

            def boot():
                rc = be.L.rs_circuit_bootstrap_dev(be.h, vp(out), vp(bits), depth, basebit, l, vp(key), ks_basebit, ks_t, vp(scratch), be._stream())
                assert rc == 0, be.L.rs_last_error()
            tc = _event_ms(boot, args.reps)
            lut, rep, lev = rand(l, N), rand(rows, n + 1), be.empty(rows, n + 1)
            tb = _event_ms(lambda: be.bootstrap_lut(rep, lut, out=lev), args.reps)
            emit(dict(what="circuit_bootstrap", set=NAME, N=N, n=n, depth=depth, basebit=basebit, l=l, ks_basebit=ks_basebit, ks_t=ks_t, rows=rows,
                      circuit_bootstrap_ms=tc["ms"], circuit_bootstrap_ms_min=tc["ms_min"], circuit_bootstrap_ms_max=tc["ms_max"],
                      bootstrap_ms=tb["ms"], bootstrap_ms_min=tb["ms_min"], bootstrap_ms_max=tb["ms_max"], key_bytes=key_bytes,
                      key_stream_ms=round(key_bytes / HBM_BYTES_PER_S * 1e3, 4), reps=args.reps))
    be.close()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
