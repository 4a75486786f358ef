"""Compressed evaluation keys per parameter set (one JSON line per set).

For every set at full size: the bytes of the compressed key (mask seed + bodies) and of the full key; rs_keygen_compressed_dev
(Backend.keygen_compressed) and rs_expand_keys_dev (Backend.expand_keys), each one untimed call then the median of --reps
synchronous calls (wall clock around the call, which ends with a device synchronisation); rs_keygen_dev for comparison; and the
wall time of one rs_load_compressed_keys from host bodies against one rs_load_keys from host arrays of the full key (host-to-device
copies, expansion, transforms into the split domain).

usage: python tools/compressed_keys_time.py [--reps 5] [--out profiles/r09/compressed_keys_time.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    lines = []
    mask_seed, noise_seed = bytes(range(32)), bytes(range(100, 132))
    for name in SETS:
        be = redsec_amd.Backend(redsec_amd.params(name), device=0)
        (_, _, _, _, _, _, _, ks_stdev, bk_stdev) = client.PARAM_SETS[name]
        lwe, tlwe = keygen.secret_keys(name, noise_seed)
        bb, kb = be.keygen_compressed(lwe, tlwe, mask_seed, noise_seed, bk_stdev, ks_stdev)
        keygen_c = _median_ms(lambda: be.keygen_compressed(lwe, tlwe, mask_seed, noise_seed, bk_stdev, ks_stdev, bk_body=bb, ksk_body=kb), args.reps)
        bk, ksk = be.expand_keys(mask_seed, bb, kb)
        expand = _median_ms(lambda: be.expand_keys(mask_seed, bb, kb, bk=bk, ksk=ksk), args.reps)
        keygen_full = _median_ms(lambda: be.keygen(lwe, tlwe, mask_seed, bk_stdev, ks_stdev, bk=bk, ksk=ksk), args.reps)
        full_bytes = (bk.numel() + ksk.numel()) * 4
        ck = keygen.CompressedKey(name, be.p.n, mask_seed, bb, kb).numpy()
        del bb, kb
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        be.load_compressed_keys(ck.mask_seed, ck.bk_body, ck.ksk_body)
        load_c = time.perf_counter() - t0
        hb, hk = bk.cpu().numpy(), ksk.cpu().numpy()
        del bk, ksk
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        be.load_keys(hb, hk)
        load_f = time.perf_counter() - t0
        del hb, hk
        d = dict(what="compressed_keys", set=name, n=be.p.n, N=be.p.N, reps=args.reps, compressed_bytes=ck.nbytes, full_bytes=full_bytes,
                 ratio=round(full_bytes / ck.nbytes, 2), expand_ms=expand, expand_write_GBps=round(full_bytes / expand / 1e6, 1),
                 keygen_compressed_ms=keygen_c, keygen_full_ms=keygen_full, load_compressed_host_ms=round(1e3 * load_c, 1),
                 load_full_host_ms=round(1e3 * load_f, 1), device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        lines.append(d)
        be.close()
        del ck
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
