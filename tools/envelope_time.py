#!/usr/bin/env python3
"""The envelope Jacobian of the true-minimum rows on the MI355X: its launches beside the value launch, and one
Jacobian call of each provider.

    python tools/envelope_time.py [--reps 15] [--out profiles/envelope_time.json]

Two shapes: C3 (64 vehicles, degree 10, 2016 pairs) and example10's swarm (3 vehicles, degree 5, 3 pairs), both at B = 1,
eps_rel = 1e-12 (BezOptimization.TRUE_MIN_EPS_REL).  One process; the three launch forms are timed INTERLEAVED -- value,
fused, two-launch, value, ... -- so that clock and neighbour drift fall on all of them alike.  A sample is the HIP-event
time of --inner back-to-back calls on one stream divided by --inner (a single 10 us launch is below what an event pair
resolves); medians and min / max over --reps samples after --warmup.
  * value:       obtg_temporal_sep_true_min_dev (val, t_star, status)
  * fused:       obtg_temporal_sep_true_min_jac_dev, the search kernel with the Jacobian epilogue, one launch
  * two_launch:  the same entry point on a context created under OBTG_TRUE_MIN_JAC_FUSED=0: value launch + block launch
Then temporalSeparationJacobian(x, method='fd') and (x, method='envelope') of a BezOptimization of the same shape: wall
time per call (median of --calls) and, in a second pass with kernel stats on, device time and launches per call.
Reported, not gated."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def sample(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def summary(ms):
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size))


def launches(N, d, n, Y, a):
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    dev = torch.device("cuda", 0)
    ctxs = {}
    for name, env in (("fused", None), ("two_launch", "0")):
        if env is not None:
            os.environ["OBTG_TRUE_MIN_JAC_FUSED"] = env
        ctxs[name] = _capi.Context(N, d, n, 0, device=0)
        os.environ.pop("OBTG_TRUE_MIN_JAC_FUSED", None)
        ctxs[name].set_stream(torch.cuda.current_stream().cuda_stream)
    P = ctxs["fused"].num_pairs
    dY = torch.from_numpy(np.ascontiguousarray(Y[None])).to(dev)
    out, ts = torch.empty((1, P), dtype=torch.float64, device=dev), torch.empty((1, P), dtype=torch.float64, device=dev)
    st = torch.empty((1, P), dtype=torch.int32, device=dev)
    jac = {k: torch.empty((1, P, d, n + 1), dtype=torch.float64, device=dev) for k in ctxs}
    eps = 1e-12
    fns = {"value": lambda: ctxs["fused"].temporal_sep_true_min_dev(dY.data_ptr(), 1, 0.9, out.data_ptr(), ts.data_ptr(), st.data_ptr(),
                                                                    eps_rel=eps)}
    for k in ctxs:
        fns[k] = (lambda k=k: ctxs[k].temporal_sep_true_min_jac_dev(dY.data_ptr(), 1, 0.9, out.data_ptr(), jac[k].data_ptr(),
                                                                    ts.data_ptr(), st.data_ptr(), eps_rel=eps))
    for _ in range(a.warmup):
        for f in fns.values():
            sample(f, a.inner)
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, f in fns.items():
            ms[k].append(sample(f, a.inner))
    r = {k: summary(v) for k, v in ms.items()}
    r.update(pairs=P, degree=n, B=1, inner=a.inner, jac_bytes=int(P * d * (n + 1) * 8),
             same_bits=bool(torch.equal(jac["fused"].view(torch.int64), jac["two_launch"].view(torch.int64))),
             status_not_ok=int((st != 0).sum().item()), interior_minima=int(((ts > 0) & (ts < 1)).sum().item()))
    for c in ctxs.values():
        c.use_own_stream()
        c.close()
    return r


def providers(bo, x, a):
    r = {}
    ctx = bo._ctx(False)
    for method in ("fd", "envelope"):
        fn = lambda: bo.temporalSeparationJacobian(x, method=method)      # noqa: E731
        fn()
        wall = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            wall.append(1e3 * (time.perf_counter() - t0))
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        fn()
        st = ctx.kernel_stats()
        ctx.set_profiling(False)
        r[method] = dict(wall=summary(wall), kernel_ms=float(sum(ms for ms, _ in st.values())),
                         launches=int(sum(k for _, k in st.values())))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "envelope_time.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    res = {"device": torch.cuda.get_device_name(0), "eps_rel": 1e-12, "source_hash": _capi.source_hash("extrema_kernels")}
    # C3: 64 vehicles crossing a circle
    ang = 2.0 * np.pi * np.arange(64) / 64
    ring = np.stack([50.0 + 45.0 * np.cos(ang), 50.0 + 45.0 * np.sin(ang)], axis=1)
    c3 = BezOptimization(numVeh=64, dimension=2, degree=10, minimizeGoal='Euclidean', maxSep=0.9, tf=10.0,
                         initPoints=[tuple(p) for p in ring], finalPoints=[tuple(p) for p in 100.0 - ring],
                         separationRows='true_min')
    ex10 = BezOptimization(numVeh=3, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=1.0, tf=10.0,
                           initPoints=[(0.0, 0.0), (0.0, 4.0), (3.0, -1.0)], finalPoints=[(6.0, 4.0), (6.0, 0.0), (3.0, 5.0)],
                           separationRows='true_min')
    for name, bo, seed in (("C3", c3, 1234), ("example10", ex10, 2)):
        x = bo.generateGuess(std=0.3, seed=seed)
        m = bo.model
        r = launches(m['numVeh'], m['dim'], m['deg'], bo.reshapeVector(x), a)
        r["n_x"] = int(x.size)
        r["providers"] = providers(bo, x, a)
        res[name] = r
        print(json.dumps({name: r}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
