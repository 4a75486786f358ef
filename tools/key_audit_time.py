"""Device decryption and the key audit per parameter set (one JSON line per set), and the noise of the project's own bootstraps.

Default mode, for every set at full size: rs_audit_keys_dev and rs_audit_compressed_keys_dev (report only, and with the noise
arrays), rs_phase_dev at B = 65,536 (N = 1024) / 4,096 (redsec_medium) / 1,024 (redsec_large) for dim = n and dim = N, each one
untimed call then the median of --reps synchronous calls (wall clock around the call, which ends with a device synchronisation);
the bytes each reads from HBM and the GB/s that makes; rs_keygen_dev's time from the same process beside it.

--bootstrap-noise: per set, under a key from keygen.generate (the set's deviations), B NAND gates by hand on fresh device
encryptions -- lincomb(a, -1, b, -1, bconst = 1/8), bootstrap_wo_ks(x, 1/8), keyswitch(u) -- and the noise = phase - expected
(+-1/8) after the blind rotation (dim = N, ring key) and after the keyswitch (dim = n): mean, standard deviation, largest |noise|,
in torus units. Recorded, not gated.

usage: python tools/key_audit_time.py [--reps 5] [--out profiles/r11/key_audit_time.jsonl]
       python tools/key_audit_time.py --bootstrap-noise [--out profiles/r11/bootstrap_noise.jsonl]
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


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * statistics.median(ts), 3)


def _gbps(nbytes, ms):
    return round(nbytes / ms / 1e6, 1)


def audit_times(name, reps):
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    p = be.p
    (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    mask_seed, noise_seed = bytes(range(32)), bytes(range(100, 132))
    lwe, tlwe = keygen.secret_keys(name, noise_seed)
    bk, ksk = be.keygen(lwe, tlwe, noise_seed, bk_stdev, ks_stdev)
    keygen_ms = _median_ms(lambda: be.keygen(lwe, tlwe, noise_seed, bk_stdev, ks_stdev, bk=bk, ksk=ksk), reps)
    full_bytes = (bk.numel() + ksk.numel()) * 4
    rep = be.audit_keys(lwe, tlwe, bk, ksk)
    d = dict(what="key_audit", set=name, n=p.n, N=p.N, reps=reps, full_bytes=full_bytes, keygen_ms=keygen_ms, report=rep)
    d["audit_full_ms"] = _median_ms(lambda: be.audit_keys(lwe, tlwe, bk, ksk), reps)
    d["audit_full_bk_ms"] = _median_ms(lambda: be.audit_keys(lwe, tlwe, bk=bk), reps)
    d["audit_full_ksk_ms"] = _median_ms(lambda: be.audit_keys(lwe, tlwe, ksk=ksk), reps)
    d["audit_full_noise_ms"] = _median_ms(lambda: be.audit_keys(lwe, tlwe, bk, ksk, noise=True), reps)
    d["audit_full_read_GBps"] = _gbps(full_bytes, d["audit_full_ms"])
    d["audit_full_ksk_read_GBps"] = _gbps(ksk.numel() * 4, d["audit_full_ksk_ms"])
    d["bk_adds"] = int(p.n * 2 * p.bk_l * p.N * int(tlwe.sum()))
    d["audit_full_bk_Gadds_per_s"] = round(d["bk_adds"] / d["audit_full_bk_ms"] / 1e6, 1)
    del bk, ksk
    torch.cuda.empty_cache()
    bb, kb = be.keygen_compressed(lwe, tlwe, mask_seed, noise_seed, bk_stdev, ks_stdev)
    d["compressed_bytes"] = 32 + (bb.numel() + kb.numel()) * 4
    d["audit_compressed_ms"] = _median_ms(lambda: be.audit_compressed_keys(lwe, tlwe, mask_seed, bb, kb), reps)
    d["audit_compressed_noise_ms"] = _median_ms(lambda: be.audit_compressed_keys(lwe, tlwe, mask_seed, bb, kb, noise=True), reps)
    d["report_compressed"] = be.audit_compressed_keys(lwe, tlwe, mask_seed, bb, kb)
    del bb, kb
    torch.cuda.empty_cache()
    B = 65536 if p.N == 1024 else (4096 if p.N == 4096 else 1024)
    d["phase_B"] = B
    for tag, key in (("n", lwe), ("N", tlwe)):
        ct = torch.randint(-(1 << 31), 1 << 31, (B, len(key) + 1), dtype=torch.int64, device="cuda").to(torch.int32)
        ms = _median_ms(lambda: be.phase(ct, key), reps)
        d["phase_dim_%s_ms" % tag] = ms
        d["phase_dim_%s_read_GBps" % tag] = _gbps(ct.numel() * 4, ms)
        del ct
    d["device"] = torch.cuda.get_device_name(0)
    be.close()
    torch.cuda.empty_cache()
    return d


def bootstrap_noise(name):
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    p = be.p
    (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
    sk, bk, ksk = keygen.generate(be, seed=bytes(range(60, 92)))
    del bk, ksk
    B = 4096 if p.N == 1024 else (1024 if p.N == 4096 else 256)
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 2, B), rng.integers(0, 2, B)
    e8 = 1 << 29
    enc = lambda bits, first: be.encrypt_seeded(sk.lwe_key, torch.from_numpy(np.where(bits, e8, -e8).astype(np.int32)).cuda(),
                                                bytes(range(32)), bytes(range(200, 232)), first=first, stdev=ks_stdev, full=True)[1]
    ca, cb = enc(a, 0), enc(b, B)
    x = be.lincomb(ca, -1, cb, -1, bconst=e8)
    u = be.bootstrap_wo_ks(x, e8)
    c = be.keyswitch(u)
    want = np.where(1 - (a & b), e8, -e8).astype(np.int64)
    d = dict(what="bootstrap_noise", set=name, n=p.n, N=p.N, B=B, gate="NAND", input_stdev=ks_stdev, bk_stdev=bk_stdev, ks_stdev=ks_stdev)
    for tag, ph in (("after_blind_rotate_dim_N", be.phase(u, sk.tlwe_key)), ("after_keyswitch_dim_n", be.phase(c, sk.lwe_key))):
        e = (ph.cpu().numpy().astype(np.int64) - want + (1 << 31)) % (1 << 32) - (1 << 31)
        t = e / 2.0 ** 32
        d[tag] = dict(mean=float(t.mean()), std=float(t.std()), max_abs=float(np.abs(t).max()))
    assert np.array_equal(sk.decrypt_bits(c.cpu().numpy()), 1 - (a & b))
    d["device"] = torch.cuda.get_device_name(0)
    be.close()
    torch.cuda.empty_cache()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bootstrap-noise", action="store_true")
    ap.add_argument("--sets", default=",".join(SETS))
    args = ap.parse_args()
    lines = []
    for name in args.sets.split(","):
        d = bootstrap_noise(name) if args.bootstrap_noise else audit_times(name, args.reps)
        print(json.dumps(d), flush=True)
        lines.append(d)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
