"""Encrypted selection (rs_ring_cmux_dev, rs_ring_lookup_dev) on one MI355X, one JSON line each.

Times (HIP events on the current stream, one untimed call per shape, then the median and the extremes of --reps calls; random words
for selectors and ciphertexts: the arithmetic does not depend on the words):
  what = "cmux": R = 1, 64 and 1,024 at redsec_small_v2 (N = 1024) and R = 1 at redsec_large (N = 8192), shape (4, 6)
      cmux_ms             Backend.ring_cmux (ring_cmux_init_kernel + ring_cmux_kernel)
      mads_per_s          R 2l 2 N^2 multiply-adds per call (one selector word times one digit) over cmux_ms
      ceiling_mads_per_s  1,024 SIMDs x 64 lanes x 2.4 GHz / 4.3 cycles (v_mul_lo_u32 per wave64, MEASUREMENTS.md section 4.1) = 3.66e13
      workgroups          2 (N / 512) (N / 1024) 2l R
  what = "lookup": 1,024 entries, depth 10, at redsec_small_v2 with (4, 6): lookup_ms of rs_ring_lookup_dev through the C ABI, its scratch
      allocated beforehand, 1,023 CMUXes in 10 levels
  what = "rekey": rs_ring_rekey_dev at R = 64, N = 1024, (4, 5), in the same process: the same inner loop, its share beside ours
  what = "noise": the decrypted error of a depth-10 lookup of a 1,024-row trivial table under a real seeded selector of the set's
      default shape and deviation: rms and largest error, each over keygen.ring_cmux_sigma(depth = 10)

  --digits: the leg of the alternating form (rs_ring_cmux_alt_dev, rs_ring_lookup_alt_dev) and nothing else:
      what = "cmux_digits" (R = 1, 64, 1,024) and "lookup_digits" (1,024 entries) at redsec_small_v2 with (4, 6), both forms in this
      one process on the same buffers, --rounds rounds of --reps calls a form, the forms taking turns within a round: per form the
      median of the rounds' medians with the least and the largest of them, and alternating_over_signed, the ratio of the two
      medians. No speed gate: the multiply-add count is the same. windows_overlap says whether min .. max of the two forms meet

usage: python tools/ring_cmux_time.py [--reps 20] [--out profiles/r26/ring_cmux_time.jsonl]
       python tools/ring_cmux_time.py --digits [--reps 20] [--rounds 5] [--out profiles/r30/ring_cmux_alt_time.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CEILING_MADS_PER_S = 1024 * 64 * 2.4e9 / 4.3
SHAPE = (4, 6)
CMUX_RUNS = (("redsec_small_v2", (1, 64, 1024)), ("redsec_large", (1,)))


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
    ap.add_argument("--digits", action="store_true", help="time the alternating form beside the signed one, and nothing else")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    rand = lambda *shape: torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0").to(torch.int32)
    lines = []
    basebit, l = SHAPE

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    def rate(d, key, mads):
        r = mads / (d[key] * 1e-3)
        d.update(mads=mads, mads_per_s=round(r, 1), ceiling_mads_per_s=round(CEILING_MADS_PER_S, 1), fraction_of_ceiling=round(r / CEILING_MADS_PER_S, 4))
        return d

    def both_forms(run):
        """run(form)() is one call -> {form: ms, ms_min, ms_max over the rounds' medians}, the ratio and whether the windows meet"""
        forms = ("signed", "alternating")
        med = {f: [] for f in forms}
        for _ in range(args.rounds):
            for f in forms:
                med[f].append(_event_ms(run(f), args.reps)["ms"])
        d = {}
        for f in forms:
            d.update({f + "_ms": round(statistics.median(med[f]), 4), f + "_ms_min": min(med[f]), f + "_ms_max": max(med[f])})
        d["alternating_over_signed"] = round(d["alternating_ms"] / d["signed_ms"], 4)
        d["windows_overlap"] = bool(d["alternating_ms_min"] <= d["signed_ms_max"] and d["signed_ms_min"] <= d["alternating_ms_max"])
        d.update(reps=args.reps, rounds=args.rounds)
        return d

    if args.digits:
        name = "redsec_small_v2"
        be = redsec_amd.Backend(redsec_amd.params(name, n=16), device=0)
        N = be.p.N
        sel = rand(2 * l, 2, N)
        for R in (1, 64, 1024):
            d1, d0, out = rand(R, 2, N), rand(R, 2, N), be.empty(R, 2, N)
            d = both_forms(lambda f: (lambda: be.ring_cmux(d1, d0, sel, basebit, l, out=out, digits=f)))
            emit(dict(what="cmux_digits", set=name, N=N, basebit=basebit, l=l, R=R, mads=R * 2 * l * 2 * N * N, **d))
        E, depth = 1024, 10
        table, sels, out = rand(E, 2, N), rand(depth, 2 * l, 2, N), be.empty(2, N)
        scratch = be.empty(E // 2 + E // 4, 2, N)
        vp = lambda t: C.c_void_p(t.data_ptr())

        def look_of(f):
            fn = be.L.rs_ring_lookup_alt_dev if f == "alternating" else be.L.rs_ring_lookup_dev

            def look():
                rc = fn(be.h, vp(out), vp(table), E, vp(sels), depth, basebit, l, vp(scratch), be._stream())
                assert rc == 0, be.L.rs_last_error()
            return look
        emit(dict(what="lookup_digits", set=name, N=N, basebit=basebit, l=l, entries=E, depth=depth, cmuxes=E - 1,
                  mads=(E - 1) * 2 * l * 2 * N * N, **both_forms(look_of)))
        be.close()

    for name, counts in (() if args.digits else CMUX_RUNS):
        be = redsec_amd.Backend(redsec_amd.params(name, n=16), device=0)     # the calls need no key: the ring is what matters
        N = be.p.N
        sel = rand(2 * l, 2, N)
        for R in counts:
            d1, d0, out = rand(R, 2, N), rand(R, 2, N), be.empty(R, 2, N)
            tm = _event_ms(lambda: be.ring_cmux(d1, d0, sel, basebit, l, out=out), args.reps)
            emit(rate(dict(what="cmux", set=name, N=N, basebit=basebit, l=l, R=R, cmux_ms=tm["ms"], cmux_ms_min=tm["ms_min"],
                           cmux_ms_max=tm["ms_max"], workgroups=2 * (N // 512) * (N // 1024) * 2 * l * R, reps=args.reps),
                      "cmux_ms", R * 2 * l * 2 * N * N))
        if N == 1024:
            # the lookup through the C ABI with scratch allocated once, as a server would hold it
            E, depth = 1024, 10
            table, sels, out = rand(E, 2, N), rand(depth, 2 * l, 2, N), be.empty(2, N)
            scratch = be.empty(E // 2 + E // 4, 2, N)
            vp = lambda t: C.c_void_p(t.data_ptr())

            def look():
                rc = be.L.rs_ring_lookup_dev(be.h, vp(out), vp(table), E, vp(sels), depth, basebit, l, vp(scratch), be._stream())
                assert rc == 0, be.L.rs_last_error()
            tm = _event_ms(look, args.reps)
            emit(rate(dict(what="lookup", set=name, N=N, basebit=basebit, l=l, entries=E, depth=depth, lookup_ms=tm["ms"],
                           lookup_ms_min=tm["ms_min"], lookup_ms_max=tm["ms_max"], cmuxes=E - 1, reps=args.reps),
                      "lookup_ms", (E - 1) * 2 * l * 2 * N * N))
            # ring re-keying beside it: the same inner loop over t rows of one source polynomial
            t = 5
            key, rl, rout = rand(t + 1, 2, N), rand(64, 2, N), be.empty(64, 2, N)
            tm = _event_ms(lambda: be.ring_rekey(rl, key, 4, t, out=rout), args.reps)
            emit(rate(dict(what="rekey", set=name, N=N, basebit=4, t=t, R=64, rekey_ms=tm["ms"], rekey_ms_min=tm["ms_min"],
                           rekey_ms_max=tm["ms_max"], workgroups=2 * (N // 512) * (N // 1024) * t * 64, reps=args.reps),
                      "rekey_ms", 64 * t * 2 * N * N))
            # the noise of a depth-10 lookup under a real selector
            sk = client.SecretKeySet.from_secret(name, *keygen.secret_keys(name, bytes(range(9, 41))))
            db, dl = keygen.ring_cmux_default(name, depth)
            stdev = keygen.rlwe_default_stdev(name)
            sigma = keygen.ring_cmux_sigma(N, db, dl, stdev, depth)
            values = np.random.default_rng(26).integers(-2047, 2048, (E, N))
            trivial = keygen.ring_trivial((values << 20).astype(np.int32))
            dev = torch.from_numpy(trivial).to("cuda:0")
            for index in (0, 693, 1023):
                sel_k = sk.ring_selector(index, depth, mask_seed=bytes(range(160, 192)), noise_seed=bytes((7 * b + index) & 0xFF for b in range(32)))
                got = be.ring_lookup(dev, sel_k).cpu().numpy()
                phase = keygen.rlwe_phase(got[None], sk.tlwe_key)[0]
                err = (phase.view(np.uint32) - trivial[index, 1].view(np.uint32)).view(np.int32) / 2.0 ** 32
                ok = bool(np.array_equal(sk.decrypt_packed_ints(got[None], N), values[index]))
                emit(dict(what="noise", set=name, N=N, basebit=db, l=dl, entries=E, depth=depth, index=index, set_bits=bin(index).count("1"),
                          sigma_row=stdev, ring_cmux_sigma=sigma, rms=float(np.sqrt(np.mean(err * err))), largest=float(np.abs(err).max()),
                          rms_over_sigma=round(float(np.sqrt(np.mean(err * err))) / sigma, 4),
                          largest_over_sigma=round(float(np.abs(err).max()) / sigma, 4), row_decrypts=ok, selector_bytes=sel_k.nbytes))
        be.close()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
