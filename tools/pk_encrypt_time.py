"""Public-key encryption (rs_pk_encrypt_dev) per parameter set and batch size (one JSON line each).

For default-128 and the REDsec set, a public key of m = keygen.pk_rows(n) rows generated and expanded on the device, and
B in {1,024, 65,536} ciphertexts with mu: one untimed call per shape, then the median (and the extremes) of --reps calls timed by HIP
events on the current stream. Per case:
  ms                   the fused call
  row_adds_per_s       B m / time: every row is offered to every ciphertext (a masked add; half of them add a row)
  pk_bytes_read        ceil(B / tile) word-tile sweeps of the key: ceil(B / tile) m (n + 1) 4 bytes, what the workgroups load (mostly
                       from L2 / Infinity Cache: the key itself is m (n + 1) 4 bytes)
  int_issue_fraction   the kernel's inner loop issues 1.5 vector instructions per (row, ciphertext, wave of 64 words) -- one v_and_b32
                       per row and one v_add3_u32 per two rows -- so B m ceil((n + 1) / 64) 1.5 wave-instructions, over the chip's
                       32-bit integer issue rate of 1,024 SIMDs x 2.4 GHz / 2 cycles per wave-instruction (= 78.6 T lane-operations/s)
At B = 1,024 the composition of earlier kernels is timed in the same session on the same inputs: linear_fc fed the same selection
bits as byte masks (sign = 1, zero = 1 - bit: 2 m B bytes of secret randomness in device memory) followed by lincomb for mu. Its
words are compared with the fused call's (they must be equal) and `ratio_fused_over_composition` is recorded.

usage: python tools/pk_encrypt_time.py [--reps 20] [--out profiles/r18/pk_encrypt_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = ("default128", "redsec_small_v2")
BATCHES = (1024, 65536)
VALU_PER_ROW_WAVE = 1.5
WAVE_INSTR_PER_S = 1024 * 2.4e9 / 2


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
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import emu_lib
    import redsec_amd
    from redsec_amd import client, keygen
    L = emu_lib.lib()
    L.rs_emu_pk_tile.argtypes = []
    tile = L.rs_emu_pk_tile()
    mask_seed, noise_seed, rand_seed = bytes(range(32)), bytes(range(100, 132)), bytes(range(200, 232))
    lines = []
    for name in SETS:
        be = redsec_amd.Backend(redsec_amd.params(name), device=0)
        n = be.p.n
        m = keygen.pk_rows(n)
        lwe, _ = keygen.secret_keys(name, noise_seed)
        _, pk = be.encrypt_seeded(lwe, torch.zeros(m, dtype=torch.int32, device="cuda:0"), mask_seed, noise_seed, 0, client.SECALPHA, full=True)
        for B in BATCHES:
            mu = torch.randint(-(1 << 31), 1 << 31, (B,), dtype=torch.int64, device="cuda:0").to(torch.int32)
            out = be.empty(B, n + 1)
            ms, lo, hi = _times_ms(lambda: be.pk_encrypt(pk, mu, rand_seed, 0, out=out), args.reps)
            waves = (n + 1 + 63) // 64
            d = dict(what="pk_encrypt", set=name, n=n, m=m, B=B, tile=tile, reps=args.reps, ms=ms, ms_min=lo, ms_max=hi,
                     row_adds_per_s=round(B * m / (ms * 1e-3), 1), pk_bytes=m * (n + 1) * 4,
                     pk_bytes_read=-(-B // tile) * m * (n + 1) * 4,
                     pk_read_GBps=round(-(-B // tile) * m * (n + 1) * 4 / ms / 1e6, 1),
                     int_issue_fraction=round(B * m * waves * VALU_PER_ROW_WAVE / (ms * 1e-3) / WAVE_INSTR_PER_S, 3),
                     device=torch.cuda.get_device_name(0))
            if B == 1024:
                sel = keygen.pk_selection(rand_seed, m, 0, B)
                zero = torch.from_numpy(np.ascontiguousarray(1 - sel.T)).cuda()
                sign = torch.ones_like(zero)
                trivial = torch.zeros(B, n + 1, dtype=torch.int32, device="cuda:0")
                trivial[:, n] = mu
                compose = lambda: be.lincomb(be.linear_fc(pk, sign, zero), 1, trivial, 1)
                cms, clo, chi = _times_ms(compose, args.reps)
                same = bool(torch.equal(compose(), be.pk_encrypt(pk, mu, rand_seed, 0)))
                d.update(composition_ms=cms, composition_ms_min=clo, composition_ms_max=chi, composition_mask_bytes=2 * m * B,
                         words_equal_composition=same, ratio_fused_over_composition=round(ms / cms, 4))
                del zero, sign, trivial
            print(json.dumps(d), flush=True)
            lines.append(d)
            del mu, out
            torch.cuda.empty_cache()
        del pk
        be.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")
    assert all(d.get("words_equal_composition", True) for d in lines), "the fused call and the composition disagree"


if __name__ == "__main__":
    main()
