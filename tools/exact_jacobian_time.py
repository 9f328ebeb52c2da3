#!/usr/bin/env python3
"""Per provider call: method='exact' against method='fd' (the structured finite-difference providers), on the MI355X.

    python tools/exact_jacobian_time.py [--reps 20] [--out profiles/exact_jacobian_time.json]

Shapes: Example1 (2 Dubins cars, 2-D, degree 10, time-optimal with prescribed speeds), C2 (8 vehicles, 3-D, degree 10,
accel objective) and a C3-shaped problem (64 vehicles, 2-D, degree 10).  For each provider: wall time of the call (it
returns a dense NumPy Jacobian: everything synchronised) and the device time of its kernels (HIP events of the library's
kernel-stats instrumentation, every launch of the call), medians over --reps calls after two warm-up calls, and the largest
scale-aware difference between the two Jacobians.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def problems():
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    ex1 = BezOptimization(numVeh=2, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, maxAngRate=1,
                          initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)], initSpeeds=[1, 1], finalSpeeds=[1, 1],
                          initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2])
    rng = np.random.default_rng(0)
    p0, p1 = rng.uniform(0, 20, (8, 3)), rng.uniform(0, 20, (8, 3))
    c2 = BezOptimization(numVeh=8, dimension=3, degree=10, minimizeGoal='Accel', maxSep=0.9, maxSpeed=4, tf=10.0,
                         initPoints=p0, finalPoints=p1)
    q0, q1 = rng.uniform(0, 60, (64, 2)), rng.uniform(0, 60, (64, 2))
    c3 = BezOptimization(numVeh=64, dimension=2, degree=10, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=8, maxAngRate=2,
                         tf=10.0, initPoints=q0, finalPoints=q1)
    return [("Example1", ex1, ('temporalSeparationJacobian', 'maxSpeedJacobian', 'maxAngularRateJacobian')),
            ("C2", c2, ('temporalSeparationJacobian', 'maxSpeedJacobian', 'objectiveGradient')),
            ("C3", c3, ('temporalSeparationJacobian', 'maxSpeedJacobian', 'maxAngularRateJacobian', 'objectiveGradient'))]


def device_ms(bezopt):
    tot = 0.0
    for c in bezopt._ctxs.values():
        c.sync()
        tot += sum(ms for ms, _ in c.kernel_stats().values())
    return tot


def profiling(bezopt, on):
    for c in bezopt._ctxs.values():
        c.set_profiling(on)
        c.reset_kernel_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "exact_jacobian_time.json"))
    args = ap.parse_args()
    from optimalbeziertrajectorygeneration_amd import _capi
    rows = []
    for name, bezopt, provs in problems():
        x = bezopt.generateGuess(std=0.3, seed=1)
        for prov in provs:
            fn = getattr(bezopt, prov)
            res = {}
            for method in ('fd', 'exact'):
                for _ in range(2):
                    J = fn(x, method=method)
                profiling(bezopt, True)          # (the contexts a call uses exist after the warm-up)
                wall, dev = [], []
                for _ in range(args.reps):
                    for c in bezopt._ctxs.values():
                        c.reset_kernel_stats()
                    t0 = time.perf_counter()
                    J = fn(x, method=method)
                    wall.append(time.perf_counter() - t0)
                    dev.append(device_ms(bezopt))
                profiling(bezopt, False)
                res[method] = (J, float(np.median(wall)) * 1e3, float(np.median(dev)))
            Jf, Je = res['fd'][0], res['exact'][0]
            diff = float(np.nanmax(np.abs(Je - Jf)) / max(np.nanmax(np.abs(Jf)), 1e-300))
            row = dict(shape=name, provider=prov, rows=int(np.size(Jf) // max(np.size(x), 1)), n_x=int(np.size(x)),
                       fd_wall_ms=round(res['fd'][1], 4), fd_kernel_ms=round(res['fd'][2], 4),
                       exact_wall_ms=round(res['exact'][1], 4), exact_kernel_ms=round(res['exact'][2], 4),
                       wall_speedup=round(res['fd'][1] / res['exact'][1], 2), max_scale_aware_diff=diff)
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    meta = dict(tool="tools/exact_jacobian_time.py", reps=args.reps, source_hash=_capi.source_hash("all"),
                jac_kernels_hash=_capi.source_hash("jac_kernels"), note="medians; kernel ms = HIP events around every launch of the call")
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
