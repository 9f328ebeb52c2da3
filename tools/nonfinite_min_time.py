#!/usr/bin/env python3
"""Device time of the reduced separation kernels, for comparing two builds of the library (RowMin, bern_device.h: every
value that enters a row's minimum is also tested for finiteness -- what does that cost?).

    OBTG_LIB=<a build of the library> python tools/nonfinite_min_time.py --label parent --out a.json
    python tools/nonfinite_min_time.py --label this --out b.json
    python tools/nonfinite_min_time.py --merge a.json b.json ... --out profiles/nonfinite_min_time.json

One process times one library (OBTG_LIB chooses it; default: the tree's): temporal_sep_min_dev and temporal_sep_active_dev
(k = 2) on the finite-difference batch of the benchmark's C3 shape (64 vehicles, 2-D, degree 10, 1153 rows) and of C5's
(the same at DEG_ELEV 100), and one_vs_many_min_dev at the two shapes of tests/golden/sequential.npz (3-D degree 5, 36 fixed
trajectories; 2-D degree 5, 999) with the planner's n_x + 1 candidates, DEG_ELEV 10.  Per call the median over --reps launches
(after --warmup) of the launch's device time: HIP events of the library's kernel statistics, id temporal_sep.  --merge puts
several such files side by side: the spread between two runs of the same library is the margin the other one gets.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def merge(paths, out):
    runs = [json.load(open(p)) for p in paths]
    cases = {}
    for r in runs:
        for name, ms in r["median_ms"].items():
            cases.setdefault(name, {}).setdefault(r["label"], []).append(ms)
    table = {}
    for name, by in cases.items():
        row = {lab: dict(runs_ms=v, mean_ms=round(float(np.mean(v)), 5)) for lab, v in by.items()}
        for lab, v in by.items():
            row[lab]["spread_rel"] = round(float((max(v) - min(v)) / np.mean(v)), 4)
        labs = sorted(by)
        if len(labs) == 2:
            a, b = ("parent", "this") if set(labs) == {"parent", "this"} else labs
            row["%s_over_%s" % (b, a)] = round(row[b]["mean_ms"] / row[a]["mean_ms"], 4)
        table[name] = row
    meta = dict(tool="tools/nonfinite_min_time.py", device=runs[0]["device"], reps=runs[0]["reps"], warmup=runs[0]["warmup"],
                libraries={r["label"]: r["bern_kernels_hash"] for r in runs},
                note="each run is a process of its own, the libraries alternating; median over the run's launches of the kernel's "
                     "device time (HIP events, kernel id temporal_sep); spread_rel = (max - min) / mean over the runs of one library")
    with open(out, "w") as f:
        json.dump(dict(meta=meta, cases=table), f, indent=1)
    print(json.dumps(table, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--label", default="this")
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    dev = _capi.default_device()
    med = {}

    def timed(ctx, name, call):
        for _ in range(args.warmup):
            call()
        ctx.sync()
        ctx.set_profiling(True, only="temporal_sep")
        v = []
        for _ in range(args.reps):
            ctx.reset_kernel_stats()
            call()
            ctx.sync()
            v.append(sum(ms for ms, _ in ctx.kernel_stats().values()))
        ctx.set_profiling(False)
        med[name] = round(float(np.median(v)), 5)
        print("%-44s %.5f ms (min %.5f, max %.5f)" % (name, med[name], min(v), max(v)), flush=True)

    for name in ("C3", "C5"):
        cfg = synth.CONFIGS[name]
        N, d, n, R = cfg["N"], cfg["d"], cfg["n"], cfg["R"]
        Yb = synth.fd_batch(synth.swarm_control_points(N, d, n, seed=1234))
        B = Yb.shape[0]
        ctx = _capi.Context(N, d, n, R, device=dev)
        P = ctx.num_pairs
        dY = torch.from_numpy(Yb).cuda()
        out = torch.empty((B, P * 2), dtype=torch.float64, device="cuda")
        idx = torch.empty((B, P * 2), dtype=torch.int32, device="cuda")
        timed(ctx, "%s temporal_sep_min_dev, R = %d, B = %d" % (name, R, B),
              lambda: ctx.temporal_sep_min_dev(dY.data_ptr(), B, 0.9, out.data_ptr()))
        timed(ctx, "%s temporal_sep_active_dev k = 2, R = %d, B = %d" % (name, R, B),
              lambda: ctx.temporal_sep_active_dev(dY.data_ptr(), B, 0.9, 2, out.data_ptr(), idx.data_ptr()))
        assert bool(torch.isfinite(out).all())
        ctx.close()
    for dim, deg, K in ((3, 5, 36), (2, 5, 999)):
        B = dim * (deg - 1) + 1
        rng = np.random.default_rng(100 * dim + K)
        one, many = rng.uniform(-5, 5, (B, dim, deg + 1)), rng.uniform(-5, 5, (K, dim, deg + 1))
        ctx = _capi.Context(1, dim, deg, 10, device=dev)
        d_one, d_many = torch.from_numpy(one).cuda(), torch.from_numpy(many).cuda()
        out = torch.empty((B, K), dtype=torch.float64, device="cuda")
        timed(ctx, "one_vs_many_min_dev %d-D deg %d, R = 10, B = %d, K = %d" % (dim, deg, B, K),
              lambda: ctx.one_vs_many_min_dev(d_one.data_ptr(), B, d_many.data_ptr(), K, 1.0, out.data_ptr()))
        assert bool(torch.isfinite(out).all())
        ctx.close()
    with open(args.out, "w") as f:
        json.dump(dict(label=args.label, device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
                       bern_kernels_hash=_capi.source_hash("bern_kernels"), median_ms=med), f, indent=1)


if __name__ == "__main__":
    main()
