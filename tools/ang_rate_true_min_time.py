#!/usr/bin/env python3
"""The true angular-rate rows on the MI355X: the value launch, both Jacobian forms, one Jacobian call of each provider, and
-- beside them, on the same box in the same process -- obtg_speed_true_min and obtg_ang_rate's launch at DEG_ELEV 0 and 100,
the rows they replace.

    python tools/ang_rate_true_min_time.py [--reps 15] [--out profiles/ang_rate_true_min.json]

Shape: C3 (64 vehicles, degree 10, d = 2) on the finite-difference batch of one iterate, B = 1153 rows (n_x + 1),
eps_rel = 1e-12 (BezOptimization.TRUE_MIN_EPS_REL).  The launch forms are timed INTERLEAVED -- value, fused, two-launch,
speed true minimum, angular rate R = 0, R = 100, value, ... -- so that clock and neighbour drift fall on all of them alike.
A sample is the HIP-event time of --inner back-to-back calls on one stream divided by --inner; medians and min / max over
--reps samples after --warmup.
  * value:       obtg_ang_rate_true_min_dev (val, t_star, status; 2 N items per batch row)
  * fused:       obtg_ang_rate_true_min_jac_dev, the search kernel with the Jacobian epilogue, one launch
  * two_launch:  the same entry point on a context created under OBTG_TRUE_MIN_JAC_FUSED=0: value launch + block launch
  * speed_true_min: obtg_speed_true_min_dev on the same batch (N items per batch row)
  * ang_R0 / ang_R100: obtg_ang_rate_dev on contexts with DEG_ELEV 0 / 100 (N (4(n+R)+1) rows per batch row)
Then maxAngularRateJacobian(x, method='fd') and (x, method='envelope') of a BezOptimization(angRateRows='true_min') of the
same shape: wall time per call (median of --calls) and, in a second pass with kernel stats on, device time and launches per
call.  `fused_within_spread` says whether the fused form's median is not above the two-launch form's by more than the spread
(max - min) of the two -- the rule under which the fused form ships.  Reported, not gated."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BOUND, EPS, RATE = 30.0, 1e-12, 1.0


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


def launches(N, d, n, Yb, tf, a):
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    dev = torch.device("cuda", 0)
    B = Yb.shape[0]
    ctxs = {}
    for name, env, R in (("fused", None, 0), ("two_launch", "0", 0), ("ang_R100", None, 100)):
        if env is not None:
            os.environ["OBTG_TRUE_MIN_JAC_FUSED"] = env
        ctxs[name] = _capi.Context(N, d, n, R, device=0)
        os.environ.pop("OBTG_TRUE_MIN_JAC_FUSED", None)
        ctxs[name].set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(np.ascontiguousarray(Yb)).to(dev)
    dtf = torch.full((B,), float(tf), dtype=torch.float64, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    out, ts, jtf = f64(B, N, 2), f64(B, N, 2), f64(B, N, 2)
    st = torch.empty((B, N, 2), dtype=torch.int32, device=dev)
    s_out, s_ts = f64(B, N), f64(B, N)
    s_st = torch.empty((B, N), dtype=torch.int32, device=dev)
    jac = {k: f64(B, N, 2, d, n + 1) for k in ("fused", "two_launch")}
    rows = {0: f64(B, N * (4 * n + 1)), 100: f64(B, N * (4 * (n + 100) + 1))}
    fns = {"value": lambda: ctxs["fused"].ang_rate_true_min_dev(dY.data_ptr(), dtf.data_ptr(), B, RATE, out.data_ptr(),
                                                                ts.data_ptr(), st.data_ptr(), eps_rel=EPS)}
    for k in ("fused", "two_launch"):
        fns[k] = (lambda k=k: ctxs[k].ang_rate_true_min_jac_dev(dY.data_ptr(), dtf.data_ptr(), B, RATE, out.data_ptr(),
                                                                jac[k].data_ptr(), jtf.data_ptr(), ts.data_ptr(), st.data_ptr(), eps_rel=EPS))
    fns["speed_true_min"] = lambda: ctxs["fused"].speed_true_min_dev(dY.data_ptr(), dtf.data_ptr(), B, BOUND, True, s_out.data_ptr(),
                                                                     s_ts.data_ptr(), s_st.data_ptr(), eps_rel=EPS)
    fns["ang_R0"] = lambda: ctxs["fused"].ang_rate_dev(dY.data_ptr(), dtf.data_ptr(), B, RATE, rows[0].data_ptr())
    fns["ang_R100"] = lambda: ctxs["ang_R100"].ang_rate_dev(dY.data_ptr(), dtf.data_ptr(), B, RATE, rows[100].data_ptr())
    for _ in range(a.warmup):
        for f in fns.values():
            sample(f, a.inner)
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, f in fns.items():
            ms[k].append(sample(f, a.inner))
    r = {k: summary(v) for k, v in ms.items()}
    spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in ("fused", "two_launch"))
    r.update(vehicles=N, degree=n, B=B, inner=a.inner, jac_bytes=int(B * N * 2 * d * (n + 1) * 8),
             fused_within_spread=bool(r["fused"]["median_ms"] <= r["two_launch"]["median_ms"] + spread),
             rows_bytes_R0=int(rows[0].numel() * 8), rows_bytes_R100=int(rows[100].numel() * 8),
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
        fn = lambda: bo.maxAngularRateJacobian(x, method=method)      # noqa: E731
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
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ang_rate_true_min.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    res = {"device": torch.cuda.get_device_name(0), "eps_rel": EPS, "max_rate": RATE, "speed_bound": BOUND, "source_hash": _capi.source_hash("extrema_kernels")}
    # C3: 64 vehicles crossing a circle
    ang = 2.0 * np.pi * np.arange(64) / 64
    ring = np.stack([50.0 + 45.0 * np.cos(ang), 50.0 + 45.0 * np.sin(ang)], axis=1)
    bo = BezOptimization(numVeh=64, dimension=2, degree=10, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=BOUND, maxAngRate=RATE,
                         tf=10.0, initPoints=[tuple(p) for p in ring], finalPoints=[tuple(p) for p in 100.0 - ring],
                         angRateRows='true_min')
    x = bo.generateGuess(std=0.3, seed=1234)
    X, _ = bo._fd_rows(x)
    r = launches(64, 2, 10, bo.reshapeVectors(X), bo.model['tf'], a)
    r["n_x"] = int(x.size)
    r["providers"] = providers(bo, x, a)
    res["C3"] = r
    print(json.dumps({"C3": r}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
