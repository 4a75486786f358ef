"""Batched circuit bootstrapping (rs_circuit_bootstrap_batch_dev, rs_ring_selector_batch_dev) on one
MI355X, one process, one JSON line each.

Times are HIP events on the current stream: one untimed call per shape, then --rounds rounds of --reps calls per route, the routes
taking turns within a round; per route the median of the rounds' medians with the least and the largest of them.
  what = "selectors": the selectors arith.evaluate needs on redsec_small_v2 with keys generated on the device, the alternating
      default shape at depth 10, for R depth = 80 and 2,560 bits: `old`, the loop of Backend.circuit_bootstrap over 30 bits at a
      time (what evaluate did before), beside `batch`, ONE Backend.circuit_bootstrap_batch. same_words is asserted here, in the
      timed process. old_over_batch is the ratio of the medians; window_below says whether the batch route's whole min .. max
      window lies below the old route's. expected_ratio is what the set's bootstrap throughput of 142 k/s suggests for the
      bootstraps alone (README), not a measurement.
  what = "keyswitch": rs_ring_selector_batch_dev alone at rows = 30, 240, 960, 3,840 and 12,800 (l = 1: count is the row count),
      n_src = 350, the ks shape of the default above, in both kernels through RS_SEL_FORM in two contexts of this process, and the
      form the unforced plan takes. mads = rows 4 N (n_src + 1) ks_t against the v_mul_lo_u32 ceiling of 1,024 SIMDs x 64 lanes x
      2.4 GHz / 4.3 cycles; key_mb_per_row_block the key words one row block reads; atomic_gb the bytes the chunked kernel adds.
  what = "evaluate": arith.evaluate, the whole call, at depth 10 for R = 8 and 256 (beside the table of section 26), with the one
      batch call's share timed alone.

usage: python tools/circuit_bootstrap_batch_time.py [--parts selectors,keyswitch,evaluate] [--reps 10] [--rounds 5]
                                                    [--out profiles/r32/circuit_bootstrap_batch_time.jsonl]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CEILING_MADS_PER_S = 1024 * 64 * 2.4e9 / 4.3
BOOTSTRAPS_PER_S = 142e3                 # README: throughput of redsec_small_v2 at a full batch
NAME, DEPTH, DIGITS = "redsec_small_v2", 10, "alternating"
ROWS = (30, 240, 960, 3840, 12800)


def _event_ms(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def _turns(routes, reps, rounds):
    """{name: fn} -> {name_ms, name_ms_min, name_ms_max}: the routes take turns within a round"""
    import torch
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    med = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            med[k].append(_event_ms(fn, reps))
    out = {}
    for k, v in med.items():
        out.update({k + "_ms": round(statistics.median(v), 4), k + "_ms_min": round(min(v), 4), k + "_ms_max": round(max(v), 4)})
    return out


@contextlib.contextmanager
def _forced(form):
    old = os.environ.get("RS_SEL_FORM")
    if form is None:
        os.environ.pop("RS_SEL_FORM", None)
    else:
        os.environ["RS_SEL_FORM"] = form          # read once, in rs_create
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("RS_SEL_FORM", None)
        else:
            os.environ["RS_SEL_FORM"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="selectors,keyswitch,evaluate")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts = args.parts.split(",")
    import numpy as np
    import torch
    import redsec_amd
    from redsec_amd import arith, keygen
    rand = lambda *shape: torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0").to(torch.int32)
    lines = []

    def emit(d):
        d.update(device=torch.cuda.get_device_name(0), reps=args.reps, rounds=args.rounds)
        print(json.dumps(d), flush=True)
        lines.append(d)

    basebit, l, ks_basebit, ks_t = keygen.circuit_bootstrap_default(NAME, DEPTH, digits=DIGITS)

    if "keyswitch" in parts:
        p = redsec_amd.params(NAME)
        N, n_src = p.N, p.n
        bes = {}
        for form in ("chunked", "wide", None):
            with _forced(form):
                bes[form] = redsec_amd.Backend(redsec_amd.params(NAME, n=16), device=0)   # needs no key: the ring and n_src are what matter
        key = rand(2, n_src + 1, ks_t, 2, N)
        for rows in ROWS:
            ct = rand(rows, n_src + 1)
            outs = {f: bes[f].empty(rows, 2, 2, N) for f in ("chunked", "wide")}
            routes = {f: (lambda f=f: bes[f].ring_selector_batch(ct, basebit, 1, key, ks_basebit, ks_t, out=outs[f])) for f in ("chunked", "wide")}
            tm = _turns(routes, args.reps, args.rounds)
            assert torch.equal(outs["chunked"], outs["wide"])
            took = {f: bes[f].last_selector() for f in ("chunked", "wide")}
            assert took["chunked"]["form"] == "chunked" and took["wide"]["form"] == "wide"
            bes[None].ring_selector_batch(ct, basebit, 1, key, ks_basebit, ks_t, out=outs["wide"])
            plan = bes[None].last_selector()
            mads = rows * 4 * N * (n_src + 1) * ks_t
            d = dict(what="keyswitch", set=NAME, N=N, n_src=n_src, rows=rows, ks_basebit=ks_basebit, ks_t=ks_t, same_words=True,
                     plan_form=plan["form"], plan_workgroups=plan["workgroups"], chunked_workgroups=took["chunked"]["workgroups"],
                     wide_workgroups=took["wide"]["workgroups"], mads=mads, ceiling_mads_per_s=round(CEILING_MADS_PER_S, 1),
                     key_mb_per_row_block=round(2 * (n_src + 1) * ks_t * 2 * N * 4 / 1e6, 2),
                     wide_key_gb=round(-(-rows // 16) * 2 * (n_src + 1) * ks_t * 2 * N * 4 / 1e9, 3),
                     atomic_gb=round(rows * 4 * N * -(-(n_src + 1) // 8) * 4 / 1e9, 3), store_mb=round(rows * 4 * N * 4 / 1e6, 1))
            d.update(tm)
            for f in ("chunked", "wide"):
                d[f + "_mads_per_s"] = round(mads / (d[f + "_ms"] * 1e-3), 1)
                d[f + "_fraction_of_ceiling"] = round(mads / (d[f + "_ms"] * 1e-3) / CEILING_MADS_PER_S, 4)
            d["chunked_over_wide"] = round(d["chunked_ms"] / d["wide_ms"], 3)
            d["plan_is_the_faster"] = bool((d["wide_ms"] < d["chunked_ms"]) == (plan["form"] == "wide"))
            emit(d)
            del ct, outs
        for be in bes.values():
            be.close()
        torch.cuda.empty_cache()

    if "selectors" in parts or "evaluate" in parts:
        be = redsec_amd.Backend(redsec_amd.params(NAME), device=0)
        sk, bk, ksk = keygen.generate(be, seed=bytes(range(9, 41)))
        del bk, ksk
        dkey = be.upload_selector_key(sk.selector_key(ks_basebit, ks_t, bytes(range(160, 192)), bytes(range(41, 73))))
        N, n = be.p.N, be.p.n

        def encrypted(R):
            idx = np.random.default_rng(R).integers(0, 1 << DEPTH, R)
            bits = np.array([[(i >> k) & 1 for i in idx] for k in range(DEPTH)])
            ct = torch.from_numpy(sk.encrypt_bits(bits.ravel(), seed=7)).to("cuda:0").reshape(DEPTH, R, n + 1)
            return idx, ct, ct.permute(1, 0, 2).contiguous().reshape(R * DEPTH, n + 1)

        if "selectors" in parts:
            for R in (8, 256):
                count = R * DEPTH
                _, _, flat = encrypted(R)
                sel = {k: be.empty(count, 2 * l, 2, N) for k in ("old", "batch")}

                def old():
                    for first in range(0, count, arith.CIRCUIT_BOOTSTRAP_BITS):
                        last = min(first + arith.CIRCUIT_BOOTSTRAP_BITS, count)
                        be.circuit_bootstrap(flat[first:last], basebit, l, dkey, ks_basebit, ks_t, out=sel["old"][first:last])

                def batch():
                    be.circuit_bootstrap_batch(flat, basebit, l, dkey, ks_basebit, ks_t, out=sel["batch"])
                tm = _turns({"old": old, "batch": batch}, args.reps, args.rounds)
                same = bool(torch.equal(sel["old"], sel["batch"]))
                assert same, "the batch call's selectors differ from those of the calls of 30 bits"
                d = dict(what="selectors", set=NAME, N=N, n=n, bits=count, basebit=basebit, l=l, ks_basebit=ks_basebit, ks_t=ks_t,
                         bootstraps=count * l, old_calls=-(-count // arith.CIRCUIT_BOOTSTRAP_BITS), same_words=same,
                         keyswitch_form=be.last_selector()["form"])
                d.update(tm)
                d["old_over_batch"] = round(d["old_ms"] / d["batch_ms"], 3)
                d["window_below"] = bool(d["batch_ms_max"] < d["old_ms_min"])
                d["bootstraps_ms_at_142k_per_s"] = round(count * l / BOOTSTRAPS_PER_S * 1e3, 2)
                d["expected_ratio"] = round(d["old_ms"] / d["bootstraps_ms_at_142k_per_s"], 2)
                emit(d)
                del sel

        if "evaluate" in parts:
            values = torch.from_numpy(np.where(np.random.default_rng(1).integers(0, 2, 1 << DEPTH) != 0, 1 << 29, -(1 << 29)).astype(np.int32)).to("cuda:0")
            for R in (8, 256):
                idx, ct, flat = encrypted(R)
                state = {}
                sel = be.empty(R * DEPTH, 2 * l, 2, N)

                def boot():
                    be.circuit_bootstrap_batch(flat, basebit, l, dkey, ks_basebit, ks_t, out=sel)

                def whole():
                    state["whole"] = arith.evaluate(be, ct, values, dkey, 1, basebit, l, ks_basebit, ks_t, digits=DIGITS)
                d = dict(what="evaluate", set=NAME, N=N, n=n, R=R, depth=DEPTH, digits=DIGITS, basebit=basebit, l=l, ks_basebit=ks_basebit,
                         ks_t=ks_t, bootstraps=R * DEPTH * l)
                d.update(_turns({"circuit_bootstrap_batch": boot, "evaluate": whole}, args.reps, args.rounds))
                got = sk.decrypt_bits(state["whole"], backend=be)
                d["decrypts"] = bool(np.array_equal(got, (values.cpu().numpy()[idx] > 0).astype(np.int64)))
                emit(d)
                del sel
        be.close()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
