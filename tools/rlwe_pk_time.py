"""Compact RLWE public keys (rs_rlwe_pk_encrypt_dev, rs_rlwe_extract_dev) on one MI355X: times and decrypted noise (one JSON line each).

Times (HIP events on the current stream, one untimed call per shape, then the median and the extremes of --reps calls):
  what = "time", N = 1024 (the REDsec set), 784 / 3,072 / 65,536 messages:
      encrypt_ms          Backend.rlwe_pk_encrypt (ceil(count / N) ciphertexts)
      unpack_ms           Backend.rlwe_unpack = rlwe_extract + keyswitch; extract_ms and keyswitch_ms are its two halves
      regev_ms            section 16's rs_pk_encrypt_dev for the same number of messages under a key of keygen.pk_rows(n) rows, same box
      bytes_sent          8 N ceil(count / N) against regev_bytes_sent = 4 (n + 1) count
  what = "time", N = 4096 and 8192 (redsec_medium / redsec_large at n = 16: neither call needs a key), one ciphertext of N messages:
      encrypt_ms, extract_ms
  masked_adds_per_s       the N^2 masked adds of each of the 2 ceil(count / N) polynomial products over encrypt_ms
Noise (what = "noise"; the key generated on the device, the RLWE public key of its ring secret at the set's bk_stdev): 8,192 messages
encrypted, unpacked and decrypted on redsec_small_v2 and default-128; the deviation and the largest value of the phase error, before
the keyswitch (rs_phase_dev at dim = N on the extracted rows) and after it, beside the formula of INTEGRATION.md section 17
  sigma^2 = alpha^2 (N + 1) + N t (1 - 2^-basebit) sigma_ks^2 + (N / 2) 2^(-2 t basebit) / 12.

usage: python tools/rlwe_pk_time.py [--reps 20] [--out profiles/r19/rlwe_pk_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (784, 3072, 65536)
LARGE = (("redsec_medium", 4096), ("redsec_large", 8192))
NOISE_SETS = ("redsec_small_v2", "default128")
NOISE_MESSAGES = 8192


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


def _sigma(p, alpha, ks_stdev):
    import numpy as np
    N, t, basebit = p.N, p.ks_t, p.ks_basebit
    return float(np.sqrt(alpha ** 2 * (N + 1) + N * t * (1 - 2.0 ** -basebit) * ks_stdev ** 2 + (N / 2) * 2.0 ** (-2 * t * basebit) / 12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    key_seed, mask_seed, noise_seed, rand_seed = bytes(range(32)), bytes(range(64, 96)), bytes(range(100, 132)), bytes(range(200, 232))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    rand = lambda *shape: torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0").to(torch.int32)
    lines = []

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    # ---- N = 1024: the REDsec set under a device-generated key, beside section 16's Regev key ----
    name = "redsec_small_v2"
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    sk, bk, ksk = keygen.generate(be, seed=key_seed)
    del bk, ksk
    n, N = be.p.n, be.p.N
    pk = dev(sk.rlwe_public_key(mask_seed, noise_seed).expand())
    m = keygen.pk_rows(n)
    _, regev = be.encrypt_seeded(sk.lwe_key, torch.zeros(m, dtype=torch.int32, device="cuda:0"), mask_seed, noise_seed, 0, client.SECALPHA, full=True)
    for count in COUNTS:
        mu = rand(count)
        R = -(-count // N)
        rlwe, rows, flat = be.empty(R, 2, N), be.empty(count, N + 1), be.empty(count, n + 1)
        enc = _times_ms(lambda: be.rlwe_pk_encrypt(pk, mu, rand_seed, 0, out=rlwe), args.reps)
        ext = _times_ms(lambda: be.rlwe_extract(rlwe, count, out=rows), args.reps)
        ksw = _times_ms(lambda: be.keyswitch(rows), args.reps)
        unp = _times_ms(lambda: be.rlwe_unpack(rlwe, count), args.reps)
        reg = _times_ms(lambda: be.pk_encrypt(regev, mu, rand_seed, 0, out=flat), args.reps)
        emit(dict(what="time", set=name, n=n, N=N, count=count, ciphertexts=R, reps=args.reps,
                  encrypt_ms=enc["ms"], encrypt_ms_min=enc["ms_min"], encrypt_ms_max=enc["ms_max"],
                  extract_ms=ext["ms"], extract_ms_min=ext["ms_min"], extract_ms_max=ext["ms_max"],
                  keyswitch_ms=ksw["ms"], keyswitch_ms_min=ksw["ms_min"], keyswitch_ms_max=ksw["ms_max"],
                  unpack_ms=unp["ms"], unpack_ms_min=unp["ms_min"], unpack_ms_max=unp["ms_max"],
                  regev_rows=m, regev_ms=reg["ms"], regev_ms_min=reg["ms_min"], regev_ms_max=reg["ms_max"],
                  masked_adds_per_s=round(2 * R * N * N / (enc["ms"] * 1e-3), 1),
                  bytes_sent=8 * N * R, regev_bytes_sent=4 * (n + 1) * count, key_bytes=32 + 4 * N, regev_key_bytes=40 + 4 * m))
        del mu, rlwe, rows, flat
        torch.cuda.empty_cache()
    del regev, pk
    be.close()
    torch.cuda.empty_cache()

    # ---- N = 4096, 8192: one ciphertext ----
    for name, N in LARGE:
        be = redsec_amd.Backend(redsec_amd.params(name, n=16), device=0)
        pk, mu = rand(2, N), rand(N)
        rlwe, rows = be.empty(1, 2, N), be.empty(N, N + 1)
        enc = _times_ms(lambda: be.rlwe_pk_encrypt(pk, mu, rand_seed, 0, 2.0 ** -30, out=rlwe), args.reps)
        ext = _times_ms(lambda: be.rlwe_extract(rlwe, N, out=rows), args.reps)
        emit(dict(what="time", set=name, N=N, count=N, ciphertexts=1, reps=args.reps,
                  encrypt_ms=enc["ms"], encrypt_ms_min=enc["ms_min"], encrypt_ms_max=enc["ms_max"],
                  extract_ms=ext["ms"], extract_ms_min=ext["ms_min"], extract_ms_max=ext["ms_max"],
                  masked_adds_per_s=round(2 * N * N / (enc["ms"] * 1e-3), 1), bytes_sent=8 * N, key_bytes=32 + 4 * N))
        del pk, mu, rlwe, rows
        be.close()
        torch.cuda.empty_cache()

    # ---- decrypted noise of unpacked inputs against the formula ----
    for name in NOISE_SETS:
        (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
        be = redsec_amd.Backend(redsec_amd.params(name), device=0)
        sk, bk, ksk = keygen.generate(be, seed=key_seed)
        del bk, ksk
        N = be.p.N
        pk = sk.rlwe_public_key(mask_seed, noise_seed)
        mu = np.random.default_rng(3).integers(-(1 << 31), 1 << 31, NOISE_MESSAGES, dtype=np.int64).astype(np.int32)
        rlwe = be.rlwe_pk_encrypt(pk, dev(mu), rand_seed, 0)
        rows = be.rlwe_extract(rlwe, NOISE_MESSAGES)
        err = lambda ph: (ph.view(np.uint32) - mu.view(np.uint32)).view(np.int32) / 2.0 ** 32
        before = err(be.phase(rows, sk.tlwe_key).cpu().numpy())
        after = err(sk.phase(be.keyswitch(rows), backend=be))
        enc_sigma, sigma = bk_stdev * float(np.sqrt(N + 1)), _sigma(be.p, bk_stdev, ks_stdev)
        rms = lambda e: float(np.sqrt(np.mean(e * e)))
        emit(dict(what="noise", set=name, n=be.p.n, N=N, messages=NOISE_MESSAGES, alpha=bk_stdev, ks_stdev=ks_stdev,
                  before_keyswitch_rms=rms(before), before_keyswitch_max=float(np.abs(before).max()), formula_alpha_sqrt_N1=enc_sigma,
                  after_keyswitch_rms=rms(after), after_keyswitch_mean=float(after.mean()), after_keyswitch_max=float(np.abs(after).max()),
                  formula_sigma=sigma, rms_over_formula=round(rms(after) / sigma, 4), max_over_formula=round(float(np.abs(after).max()) / sigma, 3)))
        be.close()
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
