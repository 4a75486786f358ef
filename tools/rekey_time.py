"""Re-keying (rs_rekey_dev) on one MI355X: times beside the keyswitch and the NAND batch of as many samples, and the decrypted
re-keying error (one JSON line each).

Times (HIP events on the current stream, one untimed call per shape, then the median and the extremes of --reps calls):
  what = "time": default-128 to default-128 with keygen.rekey_default (2, 8), and redsec_small_v2 to its ring key (n_dst = N = 1024)
  with (4, 5), at 10, 1,024 and 65,536 samples
      rekey_ms            Backend.rekey (rekey_init_kernel + rekey_kernel), random words for key and samples
      mads_per_s          B n_src t (n_dst + 1) multiply-adds per call (one key word times one digit) over rekey_ms
      ceiling_mads_per_s  1,024 SIMDs x 64 lanes x 2.4 GHz / 4.3 cycles (v_mul_lo_u32 per wave64, MEASUREMENTS.md section 4.1) = 3.66e13
      keyswitch_ms        rs_keyswitch_dev of as many samples [B][N+1] under the context's loaded key, same call, same box
      gate_ms             one NAND batch of as many ciphertexts (the bootstraps that produce that many results), median of at
                          most 5 calls
Noise (what = "noise"; secrets of two seeds, a real RekeyKey of rekey_default made on the device): fresh encryptions re-keyed and
decrypted; root mean square, largest value and mean of (phase under the recipient's key - phase under the source key) beside
keygen.rekey_sigma.

usage: python tools/rekey_time.py [--reps 20] [--out profiles/r24/rekey_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (10, 1024, 65536)
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
    key_seed, other_seed = bytes(range(32)), bytes(range(32, 64))
    mask_seed, noise_seed, rand_seed = bytes(range(64, 96)), bytes(range(100, 132)), bytes(range(140, 172))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    rand = lambda *shape: torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0").to(torch.int32)
    u32 = lambda a: np.ascontiguousarray(a, np.int32).view(np.uint32)
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

    # (label, set, n_dst): default-128 to a default-128 LWE key; redsec_small_v2 to a ring key
    for label, name, ring in (("default128 -> default128", "default128", False), ("redsec_small_v2 -> its ring key", "redsec_small_v2", True)):
        be, sk = backends[name]
        n_src, N = be.p.n, be.p.N
        n_dst = N if ring else n_src
        basebit, t = keygen.rekey_default(name)
        key = rand(n_src, t, n_dst + 1)
        for count in COUNTS:
            ct, u = rand(count, n_src + 1), rand(count, N + 1)
            out = be.empty(count, n_dst + 1)
            tm = _times_ms(lambda: be.rekey(ct, key, basebit, t, out=out), args.reps)
            ks = _times_ms(lambda: be.keyswitch(u), args.reps)
            gate = _times_ms(lambda: be.gate("NAND", ct, ct), min(args.reps, 5))
            mads = count * n_src * t * (n_dst + 1)
            rate = mads / (tm["ms"] * 1e-3)
            emit(dict(what="time", shape=label, set=name, n_src=n_src, n_dst=n_dst, basebit=basebit, t=t, count=count, rekey_ms=tm["ms"],
                      rekey_ms_min=tm["ms_min"], rekey_ms_max=tm["ms_max"], mads=mads, mads_per_s=round(rate, 1),
                      ceiling_mads_per_s=round(CEILING_MADS_PER_S, 1), fraction_of_ceiling=round(rate / CEILING_MADS_PER_S, 4),
                      keyswitch_ms=ks["ms"], keyswitch_ms_min=ks["ms_min"], keyswitch_ms_max=ks["ms_max"], gate_ms=gate["ms"],
                      gate_ms_min=gate["ms_min"], gate_ms_max=gate["ms_max"], rekey_over_gate=round(tm["ms"] / gate["ms"], 4),
                      key_bytes_expanded=4 * n_src * t * (n_dst + 1), reps=args.reps))
            del ct, u, out
        del key

    for name, ring, count in (("default128", False, 64), ("default128", False, 1024), ("redsec_small_v2", True, 10), ("redsec_small_v2", True, 1024)):
        be, sk = backends[name]
        other = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, other_seed))
        if ring:
            key = sk.rekey_for(other.rlwe_public_key(mask_seed, noise_seed), rand_seed=rand_seed, backend=be)
            row = client.PARAM_SETS[name][8] * float(np.sqrt(be.p.N + 1.0))
        else:
            key = sk.rekey_to(other, mask_seed=mask_seed, noise_seed=noise_seed, backend=be)
            row = client.PARAM_SETS[name][7]
        sigma = keygen.rekey_sigma(key.n_src, key.basebit, key.t, row)
        v = np.random.default_rng(count).integers(-2048, 2048, count)
        ct = sk.encrypt_torus(v * (1 << 20), client.PARAM_SETS[name][7], 5)
        out = be.rekey(dev(ct), key)
        err = (u32(other.phase(out, backend=be, ring=ring)) - u32(sk.phase(ct))).view(np.int32) / 2.0 ** 32
        emit(dict(what="noise", set=name, form=key.form, n_src=key.n_src, n_dst=key.n_dst, basebit=key.basebit, t=key.t, count=count,
                  key_bytes=key.nbytes, sigma_row=row, rekey_sigma=sigma, rms=float(np.sqrt(np.mean(err * err))),
                  largest=float(np.abs(err).max()), mean=float(err.mean()),
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
