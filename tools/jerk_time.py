#!/usr/bin/env python3
"""The jerk-bound rows on the MI355X beside the acceleration and speed rows they are modelled on -- the acceleration and speed
calls from a library built from the PARENT commit, in the same process, alternating.

    python tools/jerk_time.py --parent-dir DIR [--reps 15] [--out profiles/jerk_rows_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/jerk_time.py --parent-dir DIR --trace

DIR holds `_capi.py` and `libobtg_hip.so` of a build of the parent commit (the binding is loaded as a module of its own, so
both libraries live in one process).  Shape: C3 (64 vehicles, degree 10, d = 2) on the finite-difference batch of one
iterate, B = 1153 rows (n_x + 1), bound 30, eps_rel = 1e-12.  Timed INTERLEAVED -- jerk R = 0, acceleration R = 0 (parent),
speed R = 0 (parent), the same at R = 100, then the true-minimum Jacobians -- so that clock and neighbour drift fall on all
of them alike.  A sample is the HIP-event time of --inner back-to-back calls on one stream divided by --inner; medians and
min / max over --reps samples after --warmup.  The output bytes and the staging of a jerk call are those of the acceleration
and speed calls beside it; the difference is the further derivatives' arithmetic.

The true-minimum Jacobians are timed on TWO batches, and the file says which is which: `ends` is the iterate's own batch
(straight lines with N(0, 0.3) on the control points: the noise's end coefficients, which are pure squares, are the rows'
smallest), `search` the same batch with 300 cos(pi i / n) added to every vehicle's first coordinate, whose third differences
peak inside the span and stand above the noise's (an amplitude of 9 does not: the rows stay answered at the ends).  For each batch and family the count of rows whose minimiser is inside (0, 1) --
the rows that went through the search -- is recorded next to the time (`*_interior_minima`, of B x 64 rows).
--trace: no timing, --reps calls of each in the same order, for a profiler's kernel trace.
Reported, not gated."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BOUND, EPS = 30.0, 1e-12
N, D, DEG = 64, 2, 10


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


def parent_binding(path):
    spec = importlib.util.spec_from_file_location("obtg_parent_capi", os.path.join(path, "_capi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-dir", required=True)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jerk_rows_time.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    par = parent_binding(os.path.abspath(a.parent_dir))
    assert os.path.realpath(par.LIB_PATH) != os.path.realpath(_capi.LIB_PATH)
    dev = torch.device("cuda", 0)
    ang = 2.0 * np.pi * np.arange(N) / N
    ring = np.stack([50.0 + 45.0 * np.cos(ang), 50.0 + 45.0 * np.sin(ang)], axis=1)
    bo = BezOptimization(numVeh=N, dimension=D, degree=DEG, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=BOUND, tf=10.0,
                         initPoints=[tuple(p) for p in ring], finalPoints=[tuple(p) for p in 100.0 - ring], maxJerk=BOUND)
    x = bo.generateGuess(std=0.3, seed=1234)
    X, _ = bo._fd_rows(x)
    Yb = bo.reshapeVectors(X)
    B = Yb.shape[0]
    new = {R: _capi.Context(N, D, DEG, R, device=0) for R in (0, 100)}
    old = {R: par.Context(N, D, DEG, R, device=0) for R in (0, 100)}
    for c in list(new.values()) + list(old.values()):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(np.ascontiguousarray(Yb)).to(dev)
    dtf = torch.full((B,), float(bo.model['tf']), dtype=torch.float64, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    bump = Yb.copy()
    bump[:, 0::D, :] += 300.0 * np.cos(np.pi * np.arange(DEG + 1) / DEG)
    dYs = {"ends": dY, "search": torch.from_numpy(np.ascontiguousarray(bump)).to(dev)}
    rows = {(k, R): f64(B, N * (2 * DEG + R + 1)) for k in ("jerk", "accel", "speed") for R in (0, 100)}
    out, ts, jtf = f64(B, N), f64(B, N), f64(B, N)
    st = torch.empty((B, N), dtype=torch.int32, device=dev)
    jac = {k: f64(B, N, D, DEG + 1) for k in ("jerk", "accel", "speed")}
    fns = {}
    for R in (0, 100):
        fns["jerk_R%d" % R] = (lambda R=R: new[R].jerk_dev(dY.data_ptr(), dtf.data_ptr(), B, BOUND, rows[("jerk", R)].data_ptr()))
        fns["accel_R%d_parent" % R] = (lambda R=R: old[R].accel_dev(dY.data_ptr(), dtf.data_ptr(), B, BOUND, rows[("accel", R)].data_ptr()))
        fns["speed_R%d_parent" % R] = (lambda R=R: old[R].speed_dev(dY.data_ptr(), dtf.data_ptr(), B, BOUND, True, rows[("speed", R)].data_ptr()))
    for which, d_ in dYs.items():
        fns["jerk_true_min_jac_" + which] = (lambda d_=d_: new[0].jerk_true_min_jac_dev(
            d_.data_ptr(), dtf.data_ptr(), B, BOUND, out.data_ptr(), jac["jerk"].data_ptr(), jtf.data_ptr(), ts.data_ptr(), st.data_ptr(), eps_rel=EPS))
        fns["accel_true_min_jac_%s_parent" % which] = (lambda d_=d_: old[0].accel_true_min_jac_dev(
            d_.data_ptr(), dtf.data_ptr(), B, BOUND, out.data_ptr(), jac["accel"].data_ptr(), jtf.data_ptr(), ts.data_ptr(), st.data_ptr(), eps_rel=EPS))
        fns["speed_true_min_jac_%s_parent" % which] = (lambda d_=d_: old[0].speed_true_min_jac_dev(
            d_.data_ptr(), dtf.data_ptr(), B, BOUND, True, out.data_ptr(), jac["speed"].data_ptr(), jtf.data_ptr(), ts.data_ptr(), st.data_ptr(), eps_rel=EPS))
    if a.trace:
        for _ in range(a.reps):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        print("traced %d calls of each of %s" % (a.reps, ", ".join(fns)))
    else:
        for _ in range(a.warmup):
            for f in fns.values():
                sample(f, a.inner)
        ms = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, f in fns.items():
                ms[k].append(sample(f, a.inner))
        r = {k: summary(v) for k, v in ms.items()}
        for k, f in fns.items():                       # which rows went through the search, per timed true-minimum call
            if "true_min" in k:
                f()
                torch.cuda.synchronize()
                r[k]["interior_minima"] = int(((ts > 0) & (ts < 1)).sum().item())
                r[k]["status_not_ok"] = int((st != 0).sum().item())
                r[k]["items"] = int(ts.numel())
        r.update(vehicles=N, degree=DEG, dim=D, B=B, n_x=int(x.size), inner=a.inner, rows_bytes_R0=int(rows[("jerk", 0)].numel() * 8),
                 rows_bytes_R100=int(rows[("jerk", 100)].numel() * 8), jac_bytes=int(jac["jerk"].numel() * 8))
        res = {"device": torch.cuda.get_device_name(0), "eps_rel": EPS, "bound": BOUND, "C3": r,
               "source_hash": {u: _capi.source_hash(u) for u in ("bern_kernels", "extrema_kernels")},
               "parent_source_hash": {u: par.source_hash(u) for u in ("bern_kernels", "extrema_kernels")}}
        print(json.dumps(res["C3"]))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", a.out)
    for c in list(new.values()) + list(old.values()):
        c.use_own_stream()
        c.close()


if __name__ == "__main__":
    main()
