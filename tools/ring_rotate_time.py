"""Encrypted rotation (rs_ring_rotate_dev, rs_ring_heads_dev, arith.evaluate) on one MI355X, one JSON
line each.

Times are HIP events on the current stream: one untimed call per shape, then the median of --reps calls with the least and the
largest. Random words for selectors and ciphertexts: the arithmetic does not depend on the words.
  what = "rotate": the fused chain (rs_ring_rotate_dev through the C ABI, its scratch allocated beforehand) beside the route the
      library offered before it to the same words, level by level: X^e acc made with torch (roll, the wrapped part negated), then
      Backend.ring_cmux between it and acc -- one call a level with one selector set for all rows, one call a row and level with a
      set per row, which is all ring_cmux takes. Both in this one process on the same inputs, --rounds rounds, the two routes taking
      turns within a round: per route the median of the rounds' medians with the least and the largest of them. route_spread is
      the route's (max - min) / median over the rounds; fused_over_route the ratio of the medians. Points: N = 1024 with R = 1 at
      depth 10, N = 1024 with R = 256 and per-row selectors at depth 10, N = 8192 with R = 1 at depth 13, each at the shape
      keygen.ring_cmux_default gives the set at that depth.
      fraction_of_ceiling: depth R 2l 2 N^2 multiply-adds over fused_ms against 1,024 SIMDs x 64 lanes x 2.4 GHz / 4.3 cycles
      (v_mul_lo_u32 per wave64, MEASUREMENTS.md section 4.1), as tools/ring_cmux_time.py gives it for one CMUX
  what = "evaluate": arith.evaluate's three steps at depth 10 on redsec_small_v2 with keys generated on the device, R = 8 and 256, the
      alternating default shape: circuit_bootstrap_ms (ceil(10 R / 30) calls of Backend.circuit_bootstrap), rotate_ms (one
      Backend.ring_rotate with per-row selectors from one trivial row at stride 0), heads_keyswitch_ms (Backend.ring_heads +
      Backend.keyswitch), and evaluate_ms, the whole call. --eval-reps calls each.

usage: python tools/ring_rotate_time.py [--reps 20] [--rounds 5] [--eval-reps 5] [--out profiles/r31/ring_rotate_time.jsonl]
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
POINTS = (("redsec_small_v2", 1, 10, False), ("redsec_small_v2", 256, 10, True), ("redsec_large", 1, 13, False))


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
    return dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eval-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import arith, keygen
    rand = lambda *shape: torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0").to(torch.int32)
    vp = lambda t: C.c_void_p(t.data_ptr())
    lines = []

    def emit(d):
        d["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(d), flush=True)
        lines.append(d)

    for name, R, depth, per_row in POINTS:
        be = redsec_amd.Backend(redsec_amd.params(name, n=16), device=0)     # the calls need no key: the ring is what matters
        N = be.p.N
        basebit, l = keygen.ring_cmux_default(name, depth)
        rows, sel = rand(R, 2, N), rand(*(((R,) if per_row else ()) + (depth, 2 * l, 2, N)))
        out, scratch, ping = be.empty(R, 2, N), be.empty(R, 2, N), [be.empty(R, 2, N), be.empty(R, 2, N)]
        step = -1

        def fused():
            rc = be.L.rs_ring_rotate_dev(be.h, vp(out), vp(rows), R, 1, vp(sel), depth, int(per_row), step, basebit, l, vp(scratch), be._stream())
            assert rc == 0, be.L.rs_last_error()

        def route():
            acc = rows
            for k in range(depth):
                e = (step << k) % (2 * N)
                s = e % N
                turned = torch.roll(acc, s, dims=-1)
                if s:
                    turned[..., :s].neg_()
                if e >= N:
                    turned.neg_()
                nxt = ping[k & 1]
                if per_row:
                    for r in range(R):
                        be.ring_cmux(turned[r:r + 1], acc[r:r + 1], sel[r, k], basebit, l, out=nxt[r:r + 1])
                else:
                    be.ring_cmux(turned, acc, sel[k], basebit, l, out=nxt)
                acc = nxt
            return acc
        fused()
        same = bool(torch.equal(route(), out))
        med = {"fused": [], "route": []}
        for _ in range(args.rounds):
            for f, fn in (("fused", fused), ("route", route)):
                med[f].append(_event_ms(fn, args.reps)["ms"])
        d = dict(what="rotate", set=name, N=N, R=R, depth=depth, per_row=per_row, basebit=basebit, l=l, step=step, same_words=same,
                 reps=args.reps, rounds=args.rounds)
        for f in med:
            d.update({f + "_ms": round(statistics.median(med[f]), 4), f + "_ms_min": min(med[f]), f + "_ms_max": max(med[f])})
        d["route_spread"] = round((d["route_ms_max"] - d["route_ms_min"]) / d["route_ms"], 4)
        d["fused_spread"] = round((d["fused_ms_max"] - d["fused_ms_min"]) / d["fused_ms"], 4)
        d["fused_over_route"] = round(d["fused_ms"] / d["route_ms"], 4)
        mads = depth * R * 2 * l * 2 * N * N
        d.update(mads=mads, fused_ms_per_level=round(d["fused_ms"] / depth, 4), ceiling_mads_per_s=round(CEILING_MADS_PER_S, 1),
                 fraction_of_ceiling=round(mads / (d["fused_ms"] * 1e-3) / CEILING_MADS_PER_S, 4))
        emit(d)
        be.close()

    name, depth, digits = "redsec_small_v2", 10, "alternating"
    be = redsec_amd.Backend(redsec_amd.params(name), device=0)
    sk, bk, ksk = keygen.generate(be, seed=bytes(range(9, 41)))
    del bk, ksk
    basebit, l, ks_basebit, ks_t = keygen.circuit_bootstrap_default(name, depth, digits=digits)
    dkey = be.upload_selector_key(sk.selector_key(ks_basebit, ks_t, bytes(range(160, 192)), bytes(range(41, 73))))
    N, n = be.p.N, be.p.n
    values = torch.from_numpy(np.where(np.random.default_rng(1).integers(0, 2, 1 << depth) != 0, 1 << 29, -(1 << 29)).astype(np.int32)).to("cuda:0")
    for R in (8, 256):
        idx = np.random.default_rng(R).integers(0, 1 << depth, R)
        bits = np.array([[(i >> k) & 1 for i in idx] for k in range(depth)])
        ct = torch.from_numpy(sk.encrypt_bits(bits.ravel(), seed=7)).to("cuda:0").reshape(depth, R, n + 1)
        flat = ct.permute(1, 0, 2).contiguous().reshape(R * depth, n + 1)
        sel = be.empty(R, depth, 2 * l, 2, N)
        srows = sel.view(R * depth, 2 * l, 2, N)
        table = torch.zeros(1, 2, N, dtype=torch.int32, device="cuda:0")
        table[0, 1, :1 << depth] = values
        state = {}

        def boot():
            for first in range(0, R * depth, arith.CIRCUIT_BOOTSTRAP_BITS):
                last = min(first + arith.CIRCUIT_BOOTSTRAP_BITS, R * depth)
                be.circuit_bootstrap(flat[first:last], basebit, l, dkey, ks_basebit, ks_t, out=srows[first:last])

        def rotate():
            state["turned"] = be.ring_rotate(table, sel, -1, basebit, l, stride=0, per_row=True, digits=digits)

        def finish():
            state["out"] = be.keyswitch(be.ring_heads(state["turned"], 1))

        def whole():
            state["whole"] = arith.evaluate(be, ct, values, dkey, 1, basebit, l, ks_basebit, ks_t, digits=digits)
        d = dict(what="evaluate", set=name, N=N, n=n, R=R, depth=depth, digits=digits, basebit=basebit, l=l, ks_basebit=ks_basebit, ks_t=ks_t,
                 circuit_bootstrap_calls=-(-R * depth // arith.CIRCUIT_BOOTSTRAP_BITS), bootstraps=R * depth * l, reps=args.eval_reps)
        for key, fn in (("circuit_bootstrap", boot), ("rotate", rotate), ("heads_keyswitch", finish), ("evaluate", whole)):
            tm = _event_ms(fn, args.eval_reps)
            d.update({key + "_ms": tm["ms"], key + "_ms_min": tm["ms_min"], key + "_ms_max": tm["ms_max"]})
        got = sk.decrypt_bits(state["whole"], backend=be)
        d["decrypts"] = bool(np.array_equal(got, (values.cpu().numpy()[idx] > 0).astype(np.int64)))
        emit(d)
    be.close()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
