"""Packed results (rs_pack_dev) on one MI355X: times, reply sizes and decrypted packing error (one JSON line each).

Times (HIP events on the current stream, one untimed call per shape, then the median and the extremes of --reps calls):
  what = "time": default-128 with keygen.pack_default (4, 4) at 10, 1,024 and 65,536 results; redsec_small_v2 with (4, 5) at 10
      pack_ms             Backend.pack (pack_init_kernel + pack_kernel), random words for key and samples
      mads_per_s          the n t 2 N count_r multiply-adds of every ciphertext over pack_ms
      ceiling_mads_per_s  1,024 SIMDs x 64 lanes x 2.4 GHz / 4.3 cycles (v_mul_lo_u32 per wave64, MEASUREMENTS.md section 4.1) = 3.66e13
      gate_ms             one NAND batch of `count` ciphertexts on the same box (the bootstraps that produce that many results),
                          median of at most 5 calls
      bytes_packed        8 N ceil(count / N) against bytes_lwe = 4 (n + 1) count
Noise (what = "noise"; secret keys of a seed, a real PackingKey of pack_default at the set's bk_stdev): fresh encryptions packed and
decrypted; root mean square, largest value and mean of (packed phase - sample phase) beside keygen.pack_sigma.

usage: python tools/pack_time.py [--reps 20] [--out profiles/r20/pack_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("default128", 10), ("default128", 1024), ("default128", 65536), ("redsec_small_v2", 10))
NOISE = (("default128", 64), ("default128", 1024), ("redsec_small_v2", 10), ("redsec_small_v2", 1024))
CEILING_MADS_PER_S = 1024 * 64 * 2.4e9 / 4.3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    key_seed, mask_seed, noise_seed = bytes(range(32)), bytes(range(64, 96)), bytes(range(100, 132))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    rand = lambda *shape: torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0").to(torch.int32)
    ceiling = CEILING_MADS_PER_S
    lines = []

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    backends = {}
    for name in ("default128", "redsec_small_v2"):
        be = redsec_amd.Backend(redsec_amd.params(name), device=0)
        sk, bk, ksk = keygen.generate(be, seed=key_seed)
        del bk, ksk
        backends[name] = (be, sk)

    for name, count in SHAPES:
        be, sk = backends[name]
        n, N = be.p.n, be.p.N
        basebit, t = keygen.pack_default(name)
        key, ct = rand(n, t, 2, N), rand(count, n + 1)
        R = -(-count // N)
        out = be.empty(R, 2, N)
        tm = _times_ms(lambda: be.pack(ct, key, basebit, t, out=out), args.reps)
        mads = n * t * 2 * N * count                          # every ciphertext: n t rows x 2 N coefficients x its slots
        gate = _times_ms(lambda: be.gate("NAND", ct, ct), min(args.reps, 5))
        emit(dict(what="time", set=name, n=n, N=N, basebit=basebit, t=t, count=count, ciphertexts=R, pack_ms=tm["ms"],
                  pack_ms_min=tm["ms_min"], pack_ms_max=tm["ms_max"], mads=mads, mads_per_s=round(mads / (tm["ms"] * 1e-3), 1),
                  ceiling_mads_per_s=round(ceiling, 1), fraction_of_ceiling=round(mads / (tm["ms"] * 1e-3) / ceiling, 4),
                  gate_ms=gate["ms"], pack_over_gate=round(tm["ms"] / gate["ms"], 4), bytes_packed=8 * N * R, bytes_lwe=4 * (n + 1) * count,
                  key_bytes_expanded=8 * n * t * N, reps=args.reps))
        del key, ct, out

    for name, count in NOISE:
        be, sk = backends[name]
        n, N = be.p.n, be.p.N
        pk = sk.packing_key(mask_seed=mask_seed, noise_seed=noise_seed)
        sigma = keygen.pack_sigma(n, N, pk.basebit, pk.t, count, client.PARAM_SETS[name][8])
        v = np.random.default_rng(count).integers(-2048, 2048, count)
        ct = sk.encrypt_torus(v * (1 << 20), client.PARAM_SETS[name][7], 5)
        packed = be.pack(dev(ct), pk)
        err = (sk.packed_phase(packed, count, backend=be).view(np.uint32) - sk.phase(ct).view(np.uint32)).view(np.int32) / 2.0 ** 32
        emit(dict(what="noise", set=name, n=n, N=N, basebit=pk.basebit, t=pk.t, count=count, key_bytes=pk.nbytes, pack_sigma=sigma,
                  rms=float(np.sqrt(np.mean(err * err))), largest=float(np.abs(err).max()), mean=float(err.mean()),
                  rms_over_sigma=round(float(np.sqrt(np.mean(err * err)) / sigma), 4), largest_over_sigma=round(float(np.abs(err).max() / sigma), 3)))

    for be, _ in backends.values():
        be.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
