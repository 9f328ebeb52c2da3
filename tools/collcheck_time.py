#!/usr/bin/env python3
"""The collision checks beside the _minDist searches on the same pair lists, on the MI355X.

    python tools/collcheck_time.py [--reps 20] [--out profiles/collcheck_time.json]

One process, the calls interleaved (coll, minDist, coll, ...), medians over --reps timed calls after --warmup of each:
  * obtg_coll_check against obtg_min_dist on config 5's pair list (64 vehicles + 32 curve obstacles, degree 10, K = 11:
    4560 pairs) -- obtg_min_dist was the only way to ask "do these trajectories touch?" on the device;
  * obtg_coll_check2poly against obtg_min_dist2poly on the 4096-pair list of `bench.py --mode mindist` (64 vehicles
    against 64 polygon obstacles).
Wall time of the host entry point (curves and pair lists in, results out, everything synchronised) and device time of its
launch (HIP events of the library's kernel-stats instrumentation, id min_dist), gjkNew calls per pair, nodes per second of
kernel time, the deepest search, and the restatement's cost on one CPU core (tests/collcheck_ref.py, on a sample).
Condition: on each list the collision check is not slower than the _minDist call beside it (exit status 1 otherwise).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def lists():
    from optimalbeziertrajectorygeneration_amd import synth
    N, M, n = 64, 32, 10
    Yc = np.vstack((synth.swarm_control_points(N, 2, n, seed=1234), synth.curve_obstacles(M, 2, n, seed=1234)))
    curves = np.zeros((N + M, 3, n + 1))
    curves[:, :2, :] = Yc.reshape(N + M, 2, n + 1)
    pa, pb = synth.all_pairs(N + M)
    polys = synth.polygon_obstacles(64, seed=1234)
    ppts, poff = synth.pack_polys(polys)
    pc = np.repeat(np.arange(N), len(polys)).astype(np.int32)
    pp = np.tile(np.arange(len(polys)), N).astype(np.int32)
    return curves, pa, pb, N, ppts, poff, pc, pp


def timed(ctx, fns, reps, warmup):
    """fns: name -> callable; interleaved; -> name -> (last result, wall ms list, kernel ms list)"""
    out = {k: [None, [], []] for k in fns}
    for _ in range(warmup):
        for k, f in fns.items():
            out[k][0] = f()
    ctx.set_profiling(True, only="min_dist")
    for _ in range(reps):
        for k, f in fns.items():
            ctx.reset_kernel_stats()
            t0 = time.perf_counter()
            out[k][0] = f()
            out[k][1].append(1e3 * (time.perf_counter() - t0))
            ctx.sync()
            out[k][2].append(sum(ms for ms, _ in ctx.kernel_stats().values()))
    ctx.set_profiling(False)
    return out


def summary(name, r, wall, kern, n_pairs):
    kms = float(np.median(kern))
    return dict(call=name, pairs=int(n_pairs), wall_ms_median=round(float(np.median(wall)), 4), wall_ms_min=round(float(np.min(wall)), 4),
                wall_ms_max=round(float(np.max(wall)), 4), kernel_ms_median=round(kms, 4), kernel_ms_min=round(float(np.min(kern)), 4),
                kernel_ms_max=round(float(np.max(kern)), 4), gjk_calls=int(r["gjk_calls"].sum()),
                gjk_calls_per_pair=round(float(r["gjk_calls"].mean()), 3), nodes=int(r["nodes"].sum()),
                nodes_per_s_kernel=round(float(r["nodes"].sum()) / (kms * 1e-3), 1) if kms > 0 else None,
                pairs_ending_at_the_root=int((r["gjk_calls"] == 1).sum()), longest_search_nodes=int(r["nodes"].max()),
                deepest=int(r["depth"].max()), status_counts={str(s): int((r["status"] == s).sum()) for s in np.unique(r["status"])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "collcheck_time.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps: at least 20 timed calls")
    from optimalbeziertrajectorygeneration_amd import _capi
    import collcheck_ref as R
    curves, pa, pb, N, ppts, poff, pc, pp = lists()
    ctx = _capi.scratch_context()
    budget = 2000           # nodes per pair, bench.py --mode mindist's budget, for both families
    rows, ok = [], True
    for title, fns, n_pairs in (
            ("C5 pair list, K = 11", {"obtg_coll_check": lambda: ctx.coll_check(curves, pa, pb, max_nodes=budget),
                                      "obtg_min_dist": lambda: ctx.min_dist(curves, pa, pb, eps=1e-9, max_depth=128, max_nodes=budget)}, len(pa)),
            ("64 curves x 64 polygons", {"obtg_coll_check2poly": lambda: ctx.coll_check2poly(curves[:N], ppts, poff, pc, pp, max_nodes=budget),
                                         "obtg_min_dist2poly": lambda: ctx.min_dist2poly(curves[:N], ppts, poff, pc, pp, eps=1e-6, max_depth=128, max_nodes=budget)}, len(pc))):
        t = timed(ctx, fns, args.reps, args.warmup)
        pair = [summary(k, t[k][0], t[k][1], t[k][2], n_pairs) for k in fns]
        coll, md = pair
        verdict = dict(list=title, wall_ratio_min_dist_over_coll=round(md["wall_ms_median"] / coll["wall_ms_median"], 2),
                       kernel_ratio_min_dist_over_coll=round(md["kernel_ms_median"] / coll["kernel_ms_median"], 2) if coll["kernel_ms_median"] else None,
                       coll_not_slower=bool(coll["wall_ms_median"] <= md["wall_ms_median"] and coll["kernel_ms_median"] <= md["kernel_ms_median"]))
        ok = ok and verdict["coll_not_slower"]
        for row in pair + [verdict]:
            print(json.dumps(row), flush=True)
        rows.append(dict(calls=pair, verdict=verdict))
    # the restatement on one CPU core, a strided sample of each list
    s1 = np.arange(0, len(pa), max(1, len(pa) // args.cpu_sample))
    t0 = time.perf_counter()
    r1 = R.coll_check_pairs(curves, pa[s1], pb[s1], max_nodes=budget)
    t1 = time.perf_counter() - t0
    s2 = np.arange(0, len(pc), max(1, len(pc) // args.cpu_sample))
    t0 = time.perf_counter()
    r2 = R.coll_check2poly_pairs(curves[:N], ppts, poff, pc[s2], pp[s2], max_nodes=budget)
    t2 = time.perf_counter() - t0
    cpu = dict(what="tests/collcheck_ref.py (Python over the C oracle's gjkNew and split), one core, strided sample",
               curve_curve=dict(pairs=len(s1), seconds=round(t1, 3), gjk_calls=int(r1["gjk_calls"].sum()), ms_per_pair=round(1e3 * t1 / len(s1), 4),
                                whole_list_ms_extrapolated=round(1e3 * t1 / len(s1) * len(pa), 1)),
               curve_polygon=dict(pairs=len(s2), seconds=round(t2, 3), gjk_calls=int(r2["gjk_calls"].sum()), ms_per_pair=round(1e3 * t2 / len(s2), 4),
                                  whole_list_ms_extrapolated=round(1e3 * t2 / len(s2) * len(pc), 1)))
    print(json.dumps(cpu), flush=True)
    resources = None
    rp = os.path.join(REPO, "profiles", "collcheck_kernel_resources.txt")
    if os.path.exists(rp):
        resources = open(rp).read().splitlines()
    meta = dict(tool="tools/collcheck_time.py", reps=args.reps, warmup=args.warmup, max_nodes=budget, source_hash=_capi.source_hash("all"),
                coll_kernels_hash=_capi.source_hash("coll_kernels"), gjk_kernels_hash=_capi.source_hash("gjk_kernels"),
                note="medians of interleaved calls in one process; wall = host entry point, kernel = HIP events around the call's launch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, lists=rows, cpu_restatement=cpu, kernel_resources=resources), f, indent=1)
    if not ok:
        raise SystemExit("a collision check was slower than the _minDist call beside it")


if __name__ == "__main__":
    main()
