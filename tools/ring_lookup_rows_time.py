"""Batched encrypted lookup (rs_ring_lookup_rows_dev, arith.evaluate) on one MI355X, one JSON line each.

Times are HIP events on the current stream: one untimed call per shape, then the median of --reps calls. Random words for selectors
and ciphertexts: the arithmetic does not depend on the words.
  what = "lookup_rows": the fused call (rs_ring_lookup_rows_dev through the C ABI, its scratch allocated beforehand) beside the route
      the library offered before it to the same words: R calls of rs_ring_lookup_dev through the C ABI, one per row on that row's
      selector set, their scratch allocated beforehand too. Both in this one process on the same inputs, --rounds rounds, the two
      routes taking turns within a round: per route the median of the rounds' medians with the least and the largest of them.
      route_spread is the route's (max - min) / median over the rounds; fused_over_route the ratio of the medians; `faster` says
      whether the fused window lies wholly below the route's. same_words is checked in this process before anything is timed.
      Points: N = 1024 at (7, 3) with a shared table and per-row selectors, R = 256 with E = 8 (depth 3) and E = 64 (depth 6), and
      R = 1 with E = 64; N = 8192 at (6, 4), R = 16, E = 8.
      fraction_of_ceiling: R (E - 1) 2l 2 N^2 multiply-adds over fused_ms against 1,024 SIMDs x 64 lanes x 2.4 GHz / 4.3 cycles
      (v_mul_lo_u32 per wave64, MEASUREMENTS.md section 4.1), as tools/ring_cmux_time.py gives it for one CMUX
  what = "evaluate": arith.evaluate's steps at depth 13, width 1 (eight table rows of 1,024 entries: three bits choose the row, ten
      rotate it) on redsec_small_v2 with keys generated on the device, R = 8 and 256, the alternating default shape:
      circuit_bootstrap_ms (one Backend.circuit_bootstrap_batch), lookup_ms (one Backend.ring_lookup_rows), lookup_loop_ms (the R
      calls of Backend.ring_lookup it replaces), rotate_ms, heads_keyswitch_ms and evaluate_ms, the whole call. With
      --before-arith FILE also evaluate_before_ms: the evaluate of that file (the arith.py of the parent commit) on the same
      backend, keys and inputs, and whether it gives the same words. --eval-reps calls each.

usage: python tools/ring_lookup_rows_time.py [--reps 20] [--rounds 5] [--eval-reps 3] [--parts lookup,evaluate] [--before-arith FILE]
                                             [--out profiles/r33/ring_lookup_rows_time.jsonl]
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
# (set, basebit, l, R, entries, depth)
POINTS = (("redsec_small_v2", 7, 3, 256, 8, 3), ("redsec_small_v2", 7, 3, 256, 64, 6), ("redsec_small_v2", 7, 3, 1, 64, 6),
          ("redsec_large", 6, 4, 16, 8, 3))


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
    ap.add_argument("--eval-reps", type=int, default=3)
    ap.add_argument("--parts", default="lookup,evaluate")
    ap.add_argument("--before-arith", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts = args.parts.split(",")
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
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")

    for name, basebit, l, R, E, depth in (POINTS if "lookup" in parts else ()):
        be = redsec_amd.Backend(redsec_amd.params(name, n=16), device=0)     # the calls need no key: the ring is what matters
        N = be.p.N
        table, sel = rand(E, 2, N), rand(R, depth, 2 * l, 2, N)
        first = (E + 1) // 2
        per_row_scratch = first + (first + 1) // 2
        out, scratch = be.empty(R, 2, N), be.empty(R * per_row_scratch, 2, N)
        out1, scratch1 = be.empty(R, 2, N), be.empty(per_row_scratch, 2, N)

        def fused():
            rc = be.L.rs_ring_lookup_rows_dev(be.h, vp(out), vp(table), E, 0, 1, R, vp(sel), depth, 1, basebit, l, vp(scratch), be._stream())
            assert rc == 0, be.L.rs_last_error()

        def route():
            st = be._stream()
            for r in range(R):
                rc = be.L.rs_ring_lookup_dev(be.h, vp(out1[r]), vp(table), E, vp(sel[r]), depth, basebit, l, vp(scratch1), st)
                assert rc == 0, be.L.rs_last_error()
        fused()
        route()
        torch.cuda.synchronize()
        same = bool(torch.equal(out1, out))
        med = {"fused": [], "route": []}
        for _ in range(args.rounds):
            for f, fn in (("fused", fused), ("route", route)):
                med[f].append(_event_ms(fn, args.reps)["ms"])
        launches = sum(2 + (2 if (rows & 1) and rows > 1 else 0) for rows in _levels(E, depth))
        d = dict(what="lookup_rows", set=name, N=N, R=R, entries=E, depth=depth, basebit=basebit, l=l, same_words=same, reps=args.reps,
                 rounds=args.rounds, fused_launches=2 * depth, route_launches=R * launches)
        for f in med:
            d.update({f + "_ms": round(statistics.median(med[f]), 4), f + "_ms_min": min(med[f]), f + "_ms_max": max(med[f])})
        d["route_spread"] = round((d["route_ms_max"] - d["route_ms_min"]) / d["route_ms"], 4)
        d["fused_spread"] = round((d["fused_ms_max"] - d["fused_ms_min"]) / d["fused_ms"], 4)
        d["fused_over_route"] = round(d["fused_ms"] / d["route_ms"], 4)
        d["faster"] = bool(d["fused_ms_max"] < d["route_ms_min"])
        mads = R * (E - 1) * 2 * l * 2 * N * N
        d.update(mads=mads, fused_ms_per_level=round(d["fused_ms"] / depth, 4), ceiling_mads_per_s=round(CEILING_MADS_PER_S, 1),
                 fraction_of_ceiling=round(mads / (d["fused_ms"] * 1e-3) / CEILING_MADS_PER_S, 4))
        emit(d)
        be.close()

    if "evaluate" in parts:
        before = None
        if args.before_arith:
            import importlib.util
            spec = importlib.util.spec_from_file_location("redsec_amd._arith_before", args.before_arith)
            before = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(before)
        name, depth, low, digits = "redsec_small_v2", 13, 10, "alternating"
        be = redsec_amd.Backend(redsec_amd.params(name), device=0)
        sk, bk, ksk = keygen.generate(be, seed=bytes(range(9, 41)))
        del bk, ksk
        basebit, l, ks_basebit, ks_t = keygen.circuit_bootstrap_default(name, depth, digits=digits)
        dkey = be.upload_selector_key(sk.selector_key(ks_basebit, ks_t, bytes(range(160, 192)), bytes(range(41, 73))))
        N, n = be.p.N, be.p.n
        values = torch.from_numpy(np.where(np.random.default_rng(1).integers(0, 2, 1 << depth) != 0, 1 << 29, -(1 << 29)).astype(np.int32)).to("cuda:0")
        table = torch.zeros(1 << (depth - low), 2, N, dtype=torch.int32, device="cuda:0")
        table[:, 1, :] = values.view(-1, N)
        for R in (8, 256):
            idx = np.random.default_rng(R).integers(0, 1 << depth, R)
            bits = np.array([[(i >> k) & 1 for i in idx] for k in range(depth)])
            ct = torch.from_numpy(sk.encrypt_bits(bits.ravel(), seed=7)).to("cuda:0").reshape(depth, R, n + 1)
            flat = ct.permute(1, 0, 2).contiguous().reshape(R * depth, n + 1)
            sel = be.empty(R, depth, 2 * l, 2, N)
            chosen, chosen_loop = be.empty(R, 2, N), be.empty(R, 2, N)
            state = {}

            def boot():
                be.circuit_bootstrap_batch(flat, basebit, l, dkey, ks_basebit, ks_t, out=sel.view(R * depth, 2 * l, 2, N))

            def lookup():
                be.ring_lookup_rows(table, sel[:, low:].contiguous(), basebit=basebit, l=l, out=chosen, digits=digits)

            def lookup_loop():
                for r in range(R):
                    be.ring_lookup(table, sel[r, low:], basebit, l, out=chosen_loop[r], digits=digits)

            def rotate():
                state["turned"] = be.ring_rotate(chosen, sel[:, :low].contiguous(), -1, basebit, l, stride=1, per_row=True, digits=digits)

            def finish():
                state["out"] = be.keyswitch(be.ring_heads(state["turned"], 1))

            def whole():
                state["whole"] = arith.evaluate(be, ct, values, dkey, 1, basebit, l, ks_basebit, ks_t, digits=digits)

            def whole_before():
                state["before"] = before.evaluate(be, ct, values, dkey, 1, basebit, l, ks_basebit, ks_t, digits=digits)
            d = dict(what="evaluate", set=name, N=N, n=n, R=R, depth=depth, low=low, table_rows=1 << (depth - low), digits=digits, basebit=basebit,
                     l=l, ks_basebit=ks_basebit, ks_t=ks_t, bootstraps=R * depth * l, reps=args.eval_reps)
            steps = [("circuit_bootstrap", boot), ("lookup", lookup), ("lookup_loop", lookup_loop), ("rotate", rotate), ("heads_keyswitch", finish),
                     ("evaluate", whole)] + ([("evaluate_before", whole_before)] if before else [])
            for key, fn in steps:
                tm = _event_ms(fn, args.eval_reps)
                d.update({key + "_ms": tm["ms"], key + "_ms_min": tm["ms_min"], key + "_ms_max": tm["ms_max"]})
            d["lookup_same_words"] = bool(torch.equal(chosen, chosen_loop))
            if before:
                d["same_words_as_before"] = bool(torch.equal(state["whole"], state["before"]))
            got = sk.decrypt_bits(state["whole"], backend=be)
            d["decrypts"] = bool(np.array_equal(got, (values.cpu().numpy()[idx] > 0).astype(np.int64)))
            emit(d)
        be.close()


def _levels(entries, depth):
    rows = entries
    for _ in range(depth):
        yield rows
        rows = (rows + 1) // 2


if __name__ == "__main__":
    main()
