#!/usr/bin/env python3
"""obtg_one_vs_many_min_spans_dev beside obtg_one_vs_many_min_dev at the sequential planner's sizes, on the MI355X.

    python tools/aligned_time.py [--reps 30] [--out profiles/aligned_one_vs_many.json]

B = n_x + 1 candidates of the vehicle being planned (n_x = dim x (degree - 1) free coordinates) against K fixed
trajectories, 3-D, degree 3 and 5, K in {100, 1000}, DEG_ELEV = 10.  The aligned call gets staggered spans -- sorted
uniform pairs in [0, 10] for the K trajectories and one seeded span for the vehicle being planned (two random intervals are
disjoint with probability 1/3; the share each size really has is reported); its baseline is the
call that existed before it, obtg_one_vs_many_min_dev on the SAME curves (every span equal), timed in the same process,
the two calls interleaved.  Per call: the median over --reps repeats (after --warmup) of the device time of its launch
(HIP events of the library's kernel-stats instrumentation, id temporal_sep) and of the whole call between two stream
events (the aligned call also checks and copies its host span arrays).  The aligned kernel on equal spans (no split
taken) is timed as well: what the span test itself costs.  The CPU figure is tests/aligned_ref.py on one core.
No condition is asserted: there was no figure for this kernel before.
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


def stats(v):
    return dict(median=round(float(np.median(v)), 5), min=round(float(np.min(v)), 5), max=round(float(np.max(v)), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "aligned_one_vs_many.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps: at least 20 timed calls")
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    import aligned_ref as A
    dim, R, max_sep = 3, 10, 0.9
    rows = []
    for deg in (3, 5):
        B = dim * (deg - 1) + 1
        ctx = _capi.Context(1, dim, deg, R, device=_capi.default_device())
        for K in (100, 1000):
            rng = np.random.default_rng(1000 * deg + K)
            one = rng.uniform(-5, 5, size=(B, dim, deg + 1))
            many = rng.uniform(-5, 5, size=(K, dim, deg + 1))
            so = np.tile(np.sort(rng.uniform(0, 10, 2)), (B, 1))              # the candidates are ONE vehicle: one span
            sm = np.sort(rng.uniform(0, 10, size=(K, 2)), axis=1)
            sm[:, 1] = np.maximum(sm[:, 1], sm[:, 0] + 0.1)
            so[:, 1] = np.maximum(so[:, 1], so[:, 0] + 3.0)
            eq_o, eq_m = np.tile((0.0, 10.0), (B, 1)), np.tile((0.0, 10.0), (K, 1))
            d_one, d_many = torch.from_numpy(one).cuda(), torch.from_numpy(many).cuda()
            outs = {k: torch.empty((B, K), dtype=torch.float64, device="cuda") for k in ("equal", "aligned", "aligned_equal_spans")}
            calls = {
                "equal": lambda: ctx.one_vs_many_min_dev(d_one.data_ptr(), B, d_many.data_ptr(), K, max_sep, outs["equal"].data_ptr()),
                "aligned": lambda: ctx.one_vs_many_min_spans_dev(d_one.data_ptr(), so, B, d_many.data_ptr(), sm, K, max_sep,
                                                                 outs["aligned"].data_ptr(), no_overlap=1.0e6),
                "aligned_equal_spans": lambda: ctx.one_vs_many_min_spans_dev(d_one.data_ptr(), eq_o, B, d_many.data_ptr(), eq_m, K, max_sep,
                                                                             outs["aligned_equal_spans"].data_ptr(), no_overlap=1.0e6)}
            stream = torch.cuda.current_stream()
            for _ in range(args.warmup):
                for f in calls.values():
                    f()
            ctx.sync()
            torch.cuda.synchronize()
            assert torch.equal(outs["equal"], outs["aligned_equal_spans"])
            kern, call = {k: [] for k in calls}, {k: [] for k in calls}
            ctx.set_profiling(True, only="temporal_sep")
            for _ in range(args.reps):
                for k, f in calls.items():
                    ctx.reset_kernel_stats()
                    f()
                    ctx.sync()
                    kern[k].append(sum(ms for ms, _ in ctx.kernel_stats().values()))
            ctx.set_profiling(False)
            for _ in range(args.reps):                # the whole call, host side included: wall time to a finished stream
                for k, f in calls.items():
                    ctx.sync()
                    t0 = time.perf_counter()
                    f()
                    ctx.sync()
                    call[k].append(1e3 * (time.perf_counter() - t0))
            apart = float((outs["aligned"] == 1.0e6).float().mean().item())
            n = min(args.cpu_pairs, K)
            t0 = time.perf_counter()
            cpu = A.one_vs_many(one[:1], so[:1], many[:n], sm[:n], R, max_sep, 1.0e6)
            t_cpu = time.perf_counter() - t0
            got = outs["aligned"][0, :n].cpu().numpy()
            assert np.allclose(got, cpu[0], rtol=1e-9, atol=1e-9 * np.abs(cpu).max())
            row = dict(dim=dim, degree=deg, deg_elev=R, B=B, K=K, pairs=B * K, share_without_overlap=round(apart, 4),
                       kernel_ms={k: stats(v) for k, v in kern.items()}, call_wall_ms={k: stats(v) for k, v in call.items()},
                       kernel_ratio_aligned_over_equal=round(float(np.median(kern["aligned"]) / np.median(kern["equal"])), 3),
                       kernel_ratio_aligned_equal_spans_over_equal=round(float(np.median(kern["aligned_equal_spans"]) / np.median(kern["equal"])), 3),
                       call_ratio_aligned_over_equal=round(float(np.median(call["aligned"]) / np.median(call["equal"])), 3),
                       pairs_per_s_kernel_aligned=round(B * K / (np.median(kern["aligned"]) * 1e-3), 1),
                       cpu_restatement=dict(pairs=n, seconds=round(t_cpu, 4), pairs_per_s=round(n / t_cpu, 1)))
            print(json.dumps(row), flush=True)
            rows.append(row)
        ctx.close()
    meta = dict(tool="tools/aligned_time.py", reps=args.reps, warmup=args.warmup, obtg_source_hash=_capi.source_hash("all"),
                bern_kernels_hash=_capi.source_hash("bern_kernels"), device=torch.cuda.get_device_name(0),
                note="medians of interleaved calls in one process; kernel = HIP events around the call's launch, call_wall = host "
                     "clock from the call to a finished stream; baseline `equal` = obtg_one_vs_many_min_dev on the same curves")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, sizes=rows), f, indent=1)


if __name__ == "__main__":
    main()
