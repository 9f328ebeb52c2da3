#!/usr/bin/env python3
"""The keep-in rows on the MI355X beside the acceleration rows, their yardstick: the same kernel body (true_min_body,
wave_search) on a polynomial twice as long, 2n + 1 coefficients where a keep-in row has n + 1.

    python tools/keep_in_probe.py [--reps 15] [--inner 10] [--out profiles/keep_in.json]

Shape: C3 (64 vehicles, degree 10, d = 2) on the finite-difference batch of one iterate, B = 1153 rows (n_x + 1); the region
is a box, 4 faces per vehicle: 295 168 keep-in items per call against 73 792 acceleration items.  eps_rel = 1e-12
(BezOptimization.TRUE_MIN_EPS_REL).  The box is laid through the swarm (half the span of the vehicles' end points), so that
margins of both signs are in the batch; how many items have their minimiser inside (0, 1) is reported for both families.
Every figure is KERNEL time: obtg_kernel_stats' device time of all launches of --inner calls, divided by --inner, in a
sample of its own; --reps samples per call, the calls INTERLEAVED -- keep-in rows, keep-in true minima, those with blocks,
acceleration true minima, those with blocks, the two keep-in searches again on a box no vehicle comes near (`_far_box`: the
same minimisers under a tolerance eps_rel s several times larger, so shorter searches), keep-in rows, ... -- so that clock and
neighbour drift fall on all of them alike.  Reported: median, min and max, and the median per item."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EPS, ACCEL = 1e-12, 3.0


def summary(ms, items):
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size), items=int(items),
                median_ns_per_item=float(np.median(ms)) * 1e6 / items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keep_in.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization, _keep_in_tables
    N, d, n = 64, 2, 10
    ang = 2.0 * np.pi * np.arange(N) / N
    ring = np.stack([50.0 + 45.0 * np.cos(ang), 50.0 + 45.0 * np.sin(ang)], axis=1)
    box = (np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]), np.array([72.5, -27.5, 72.5, -27.5]))
    bo = BezOptimization(numVeh=N, dimension=2, degree=n, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=30.0, maxAngRate=1.0,
                         tf=10.0, initPoints=[tuple(p) for p in ring], finalPoints=[tuple(p) for p in 100.0 - ring],
                         maxAccel=ACCEL, keepIn=box)
    x = bo.generateGuess(std=0.3, seed=1234)
    X, _ = bo._fd_rows(x)
    Yb = np.ascontiguousarray(bo.reshapeVectors(X))
    B = Yb.shape[0]
    H, VF = _keep_in_tables(box, N, d)
    P_ = VF.shape[0]
    dev = torch.device("cuda", 0)
    ctx = _capi.Context(N, d, n, 0, device=0)
    ctx.set_keep_in(H, VF)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    # the same items against a box no vehicle comes near: the same minimisers, but b enters the coefficients' scale s, so the
    # tolerance eps_rel s is several times larger and the items that go to the wave search stay there for fewer nodes
    far = _capi.Context(N, d, n, 0, device=0)
    far.set_keep_in(_keep_in_tables((box[0], np.array([300.0, 200.0, 300.0, 200.0])), N, d)[0], VF)
    far.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(Yb).to(dev)
    dtf = torch.full((B,), 10.0, dtype=torch.float64, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    rows, out, ts, jac = f64(B, P_, n + 1), f64(B, P_), f64(B, P_), f64(B, P_, d, n + 1)
    st = torch.empty((B, P_), dtype=torch.int32, device=dev)
    out_a, ts_a, jtf_a, jac_a = f64(B, N), f64(B, N), f64(B, N), f64(B, N, d, n + 1)
    st_a = torch.empty((B, N), dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()      # noqa: E731
    out_f, ts_f = f64(B, P_), f64(B, P_)
    fns = {
        "keep_in_dev": (ctx, lambda: ctx.keep_in_dev(p(dY), B, p(rows)), B * P_),
        "keep_in_true_min_dev": (ctx, lambda: ctx.keep_in_true_min_dev(p(dY), B, p(out), p(ts), p(st), eps_rel=EPS), B * P_),
        "keep_in_true_min_jac_dev": (ctx, lambda: ctx.keep_in_true_min_jac_dev(p(dY), B, p(out), p(jac), p(ts), p(st), eps_rel=EPS), B * P_),
        "accel_true_min_dev": (ctx, lambda: ctx.accel_true_min_dev(p(dY), p(dtf), B, ACCEL, p(out_a), p(ts_a), p(st_a), eps_rel=EPS), B * N),
        "accel_true_min_jac_dev": (ctx, lambda: ctx.accel_true_min_jac_dev(p(dY), p(dtf), B, ACCEL, p(out_a), p(jac_a), p(jtf_a), p(ts_a),
                                                                           p(st_a), eps_rel=EPS), B * N),
        "keep_in_true_min_dev_far_box": (far, lambda: far.keep_in_true_min_dev(p(dY), B, p(out_f), p(ts_f), p(st), eps_rel=EPS), B * P_),
        "keep_in_true_min_jac_dev_far_box": (far, lambda: far.keep_in_true_min_jac_dev(p(dY), B, p(out_f), p(jac), p(ts_f), p(st), eps_rel=EPS),
                                             B * P_),
    }
    for c in (ctx, far):
        c.set_profiling(True)

    def sample(c, fn):
        c.reset_kernel_stats()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        stats = c.kernel_stats()
        assert sum(k for _, k in stats.values()) == stats["speed"][1] == a.inner, stats      # one launch per call, under "speed"
        return stats["speed"][0] / a.inner
    for _ in range(a.warmup):
        for c, f, _ in fns.values():
            sample(c, f)
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, (c, f, _) in fns.items():
            ms[k].append(sample(c, f))
    t_f = ts_f.cpu().numpy()
    # (the far-box calls last: st and jac hold the near box's again for the counts below)
    fns["keep_in_true_min_jac_dev"][1]()
    for c in (ctx, far):
        c.set_profiling(False)
    torch.cuda.synchronize()
    res = {k: summary(v, fns[k][2]) for k, v in ms.items()}
    t_k, t_a, v_k = ts.cpu().numpy(), ts_a.cpu().numpy(), out.cpu().numpy()
    shape = dict(keep_in=dict(items=int(t_k.size), interior_minimisers=int(((t_k > 0) & (t_k < 1)).sum()), negative_margins=int((v_k < 0).sum()),
                              status_ok=int((st.cpu().numpy() == 0).sum())),
                 keep_in_far_box=dict(items=int(t_f.size), interior_minimisers=int(((t_f > 0) & (t_f < 1)).sum())),
                 accel=dict(items=int(t_a.size), interior_minimisers=int(((t_a > 0) & (t_a < 1)).sum()), status_ok=int((st_a.cpu().numpy() == 0).sum())))
    for c in (ctx, far):
        c.use_own_stream()
        c.close()
    ratio = {k + far_: res["keep_in_true_min" + k + far_]["median_ns_per_item"] / res["accel_true_min" + k]["median_ns_per_item"]
             for k in ("_dev", "_jac_dev") for far_ in ("", "_far_box")}
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _capi.source_hash("extrema_kernels"), "eps_rel": EPS,
              "C3": dict(vehicles=N, degree=n, B=int(B), faces_per_vehicle=4, inner=a.inner, kernel_time=res, batch=shape,
                         ratio_keep_in_over_accel_per_item=ratio),
              "not_measured": ["call time on the host side (HIP events around the calls)", "hardware counters (no rocprofv3 pass was made)",
                               "degrees other than 10, 3-D, the workspace route"]}
    print(json.dumps(result["C3"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
