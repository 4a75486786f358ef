"""Sparse bootstraps (rs_bootstrap_sparse_dev) on one MI355X: what skipping the dead output channels of
nets/cifar/binarynet's conv6 is worth. One JSON line per measurement; HIP events on the current stream, one untimed run, then the
median and the extremes of --reps runs (default 5).

  what = "image"    one bundled CIFAR-10 image through EncryptedCifar on REDsec's shipped set (the benchmark's cifar leg: real keys of
                    seed 7, image 13), with skip_dead as the line says; `tree` names the checkout whose package and library
                    ran: "this tree", or with --tree PATH a checkout of the PARENT commit built by its own recipe (there the
                    dense leg is the only one: the parent has no skip_dead).
  what = "stage"    the conv6 and maxpool6 stages alone on the slabs the image run produced: Backend.bootstrap (dense) against
                    Backend.bootstrap_sparse with the stage's live list; rows, live rows, and rs_last_launch of both.
  what = "verdict"  written when a parent image line is in the output file already: the sparse image against the parent's median
                    and its own min-to-max spread (the one timing condition: not slower than the parent beyond that spread).

usage: python tools/sparse_time.py [--reps 5] [--legs dense,sparse,stages] [--tree PARENT_CHECKOUT] [--out profiles/r22/sparse_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return dict(ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), runs=[round(t, 3) for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="dense,sparse,stages")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    tree = os.path.abspath(a.tree) if a.tree else ROOT
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch
    import redsec_amd
    from redsec_amd import client, nets
    import plain_model as pm
    lib = "this tree" if tree == ROOT else "parent"
    sparse_api = hasattr(redsec_amd.Backend, "bootstrap_sparse")
    sk = client.SecretKeySet("redsec_small_v2", seed=7)
    be = redsec_amd.Backend(redsec_amd.params("redsec_small_v2"), device=0)
    be.load_keys(sk.bk, sk.ksk)
    net = pm.CifarNet("binarynet")
    labels, pix = pm.load_cifar_images()
    ct = torch.from_numpy(sk.encrypt_image(pix[13], seed=4)).cuda(0)
    lines = []

    def emit(rec):
        rec = dict(rec, reps=a.reps, device=torch.cuda.get_device_name(0))
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    outs = {}
    for leg, skip in (("dense", False), ("sparse", True)):
        if leg not in legs or (skip and not sparse_api):
            continue
        enc = nets.EncryptedCifar(be, net, skip_dead=True) if skip else nets.EncryptedCifar(be, net)
        t = _times_ms(lambda: outs.__setitem__(leg, enc.run(ct)), a.reps)
        emit(dict(what="image", net="binarynet", params="redsec_small_v2", mode=be.mode(), skip_dead=skip, tree=lib, **t))
    if "dense" in outs and "sparse" in outs:
        assert torch.equal(outs["dense"], outs["sparse"]), "skip_dead changed the logit ciphertexts"
    if "stages" in legs and sparse_api:
        enc = nets.EncryptedCifar(be, net, skip_dead=True)
        taps = []
        enc.run(ct, taps=taps)
        for name in ("conv6", "maxpool6"):
            rec = [r for r in taps if r["name"] == name][0]
            pre, mu, live = rec["inputs"][0], rec["mu"], enc.live[name]
            out = be.empty(*pre.shape)
            dense = _times_ms(lambda: be.bootstrap(pre, mu, out=out), a.reps)
            form_dense = be.last_launch()
            ref = out.clone()
            sparse = _times_ms(lambda: be.bootstrap_sparse(pre, mu, live, out=out), a.reps)
            form_sparse = be.last_launch()
            assert torch.equal(out, ref), name
            emit(dict(what="stage", stage=name, rows=int(pre.shape[0]), live=int(live.numel()), tree=lib,
                      dense=dense, sparse=sparse, launch_dense=form_dense, launch_sparse=form_sparse,
                      sparse_over_dense=round(sparse["ms"] / dense["ms"], 4)))
        del taps
    be.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        old = [json.loads(l) for l in open(a.out)] if os.path.exists(a.out) else []
        allrec = old + lines
        parent = [r for r in allrec if r.get("what") == "image" and r.get("tree") != "this tree" and not r.get("skip_dead")]
        mine = [r for r in allrec if r.get("what") == "image" and r.get("tree") == "this tree" and r.get("skip_dead")]
        if parent and mine and not any(r.get("what") == "verdict" for r in allrec):
            p, s = parent[-1], mine[-1]
            spread = round(p["ms_max"] - p["ms_min"], 3)
            lines.append(dict(what="verdict", parent_ms=p["ms"], parent_spread_ms=spread, skip_dead_ms=s["ms"],
                              gain_ms=round(p["ms"] - s["ms"], 3), gain_percent=round(100.0 * (p["ms"] - s["ms"]) / p["ms"], 2),
                              not_slower_beyond_parent_spread=bool(s["ms"] <= p["ms"] + spread)))
            print(json.dumps(lines[-1]))
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
