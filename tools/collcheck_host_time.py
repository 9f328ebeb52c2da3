#!/usr/bin/env python3
"""Time of obtg_coll_check / obtg_coll_check2poly as the caller sees them, for comparing two builds of the library (the
host looks at every coordinate before it picks the planar kernels: what does that cost?).

    OBTG_LIB=<a build of the library> python tools/collcheck_host_time.py --label parent --out a.json
    python tools/collcheck_host_time.py --label this --out b.json
    python tools/collcheck_host_time.py --merge a.json b.json ... --out profiles/collcheck_host_time.json

One process times one library (OBTG_LIB chooses it; default: the tree's): config 5's pair list as
tests/test_gpu_collcheck.py::test_c5_pair_list_in_one_call passes it (96 planar curves of 11 control points, 4560 pairs,
max_nodes 2000) and the 64 curves x 64 polygons of tools/collcheck_time.py.  Per call the median over --reps calls (after
--warmup) of the entry point's wall time (operands in, results out, synchronised) and of its launch's device time (HIP events
of the library's kernel statistics, id min_dist).  --merge puts several such files side by side: the spread between two runs
of the same library is the margin the other one gets.
"""
import argparse
import json
import os
import sys
import time

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
        row = {lab: dict(runs_ms=v, mean_ms=round(float(np.mean(v)), 5), spread_rel=round(float((max(v) - min(v)) / np.mean(v)), 4))
               for lab, v in by.items()}
        if set(by) == {"parent", "this"}:
            row["this_over_parent"] = round(row["this"]["mean_ms"] / row["parent"]["mean_ms"], 4)
        table[name] = row
    meta = dict(tool="tools/collcheck_host_time.py", device=runs[0]["device"], reps=runs[0]["reps"], warmup=runs[0]["warmup"],
                libraries={r["label"]: r["source_hash"] for r in runs},
                note="each run is a process of its own, the libraries alternating; median over the run's calls; wall = the host "
                     "entry point, kernel = HIP events around its launch (kernel id min_dist); spread_rel = (max - min) / mean "
                     "over the runs of one library")
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
    g = np.load(os.path.join(REPO, "tests", "golden", "c5.npz"))
    curves = np.zeros((96, 3, 11))
    curves[:, :2] = np.vstack((g["Y"], g["Yobs"])).reshape(96, 2, 11)
    pa, pb = np.triu_indices(96, 1)
    polys = synth.polygon_obstacles(64, seed=1234)
    ppts, poff = synth.pack_polys(polys)
    pc, pp = np.repeat(np.arange(64), len(polys)).astype(np.int32), np.tile(np.arange(len(polys)), 64).astype(np.int32)
    ctx = _capi.scratch_context()
    med = {}
    for name, call in (("C5 pair list, obtg_coll_check, 4560 pairs", lambda: ctx.coll_check(curves, pa, pb, max_nodes=2000)),
                       ("64 curves x 64 polygons, obtg_coll_check2poly, 4096 pairs",
                        lambda: ctx.coll_check2poly(curves[:64], ppts, poff, pc, pp, max_nodes=2000))):
        for _ in range(args.warmup):
            call()
        ctx.set_profiling(True, only="min_dist")
        wall, kern = [], []
        for _ in range(args.reps):
            ctx.reset_kernel_stats()
            t0 = time.perf_counter()
            call()
            wall.append(1e3 * (time.perf_counter() - t0))
            ctx.sync()
            kern.append(sum(ms for ms, _ in ctx.kernel_stats().values()))
        ctx.set_profiling(False)
        med[name + ", wall"] = round(float(np.median(wall)), 5)
        med[name + ", kernel"] = round(float(np.median(kern)), 5)
        print("%-62s wall %.5f ms (min %.5f, max %.5f), kernel %.5f ms" % (name, med[name + ", wall"], min(wall), max(wall), med[name + ", kernel"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(label=args.label, device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
                       source_hash=_capi.source_hash("all"), median_ms=med), f, indent=1)


if __name__ == "__main__":
    main()
