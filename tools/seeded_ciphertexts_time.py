"""Seeded LWE ciphertexts per parameter set and batch size (one JSON line each).

For every set at full size and B in {784, 3072, 24576, 65536}: rs_encrypt_seeded_dev with the full samples and with bodies only
(Backend.encrypt_seeded; synchronous), and rs_expand_ciphertexts_dev (Backend.expand_ciphertexts), each one untimed call then the
median of --reps calls timed by HIP events on the current stream; the rate of written bytes of the expansion (B (n + 1) 4 bytes);
an estimate of the share of the chip's integer issue rate the mask generation uses (about 62 lane operations per ChaCha word,
39 T lane operations per second); the bytes of the TFHE file records (4 n + 16 per sample) against the RSC1 file; and the
host-to-device upload of the full samples against that of the bodies (pinned host memory, HIP events, median of --reps).

usage: python tools/seeded_ciphertexts_time.py [--reps 20] [--out profiles/r10/seeded_ciphertexts_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = ("default128", "redsec_small_v2", "redsec_small", "redsec_medium", "redsec_large")
BATCHES = (784, 3072, 24576, 65536)
LANE_OPS_PER_WORD = 62.0
LANE_OPS_PER_S = 39e12


def _median_ms(fn, reps):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import redsec_amd
    from redsec_amd import client, keygen
    lines = []
    mask_seed, noise_seed = bytes(range(32)), bytes(range(100, 132))
    for name in SETS:
        be = redsec_amd.Backend(redsec_amd.params(name), device=0)
        n = be.p.n
        lwe, _ = keygen.secret_keys(name, noise_seed)
        for B in BATCHES:
            mu = torch.zeros(B, dtype=torch.int32, device="cuda:0")
            body, ct = be.encrypt_seeded(lwe, mu, mask_seed, noise_seed, 0, client.SECALPHA, full=True)
            enc_full = _median_ms(lambda: be.encrypt_seeded(lwe, mu, mask_seed, noise_seed, 0, client.SECALPHA, full=True), args.reps)
            enc_body = _median_ms(lambda: be.encrypt_seeded(lwe, mu, mask_seed, noise_seed, 0, client.SECALPHA), args.reps)
            expand = _median_ms(lambda: be.expand_ciphertexts(mask_seed, body, 0, out=ct), args.reps)
            written = B * (n + 1) * 4
            host_ct = torch.empty(B, n + 1, dtype=torch.int32).pin_memory()
            host_body = torch.empty(B, dtype=torch.int32).pin_memory()
            up_full = _median_ms(lambda: ct.copy_(host_ct, non_blocking=True), args.reps)
            up_body = _median_ms(lambda: body.copy_(host_body, non_blocking=True), args.reps)
            words = B * 16 * ((n + 15) // 16)
            d = dict(what="seeded_ciphertexts", set=name, n=n, B=B, reps=args.reps, encrypt_full_ms=enc_full, encrypt_bodies_ms=enc_body,
                     expand_ms=expand, expand_write_GBps=round(written / expand / 1e6, 1),
                     chacha_issue_fraction_est=round(words * LANE_OPS_PER_WORD / (expand * 1e-3) / LANE_OPS_PER_S, 3),
                     tfhe_file_bytes=B * (4 * n + 16), rsc1_file_bytes=client._RS_HEADER.itemsize + 40 + 4 * B,
                     ratio=round(B * (4 * n + 16) / (client._RS_HEADER.itemsize + 40 + 4 * B), 1),
                     upload_full_ms=up_full, upload_bodies_ms=up_body, device=torch.cuda.get_device_name(0))
            print(json.dumps(d), flush=True)
            lines.append(d)
            del body, ct, mu, host_ct, host_body
            torch.cuda.empty_cache()
        be.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
