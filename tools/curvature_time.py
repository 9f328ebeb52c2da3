#!/usr/bin/env python3
"""The curvature rows on the MI355X beside the angular-rate rows, their yardstick: the same num / den coefficients, and a
single-polynomial search where the curvature rows search two polynomials at once under a bound with square roots.

    python tools/curvature_time.py [--reps 15] [--inner 10] [--out profiles/curvature_time.json]

Shape: C3 (64 vehicles, degree 10, d = 2) on the finite-difference batch of one iterate, B = 1153 rows (n_x + 1), 147 584 items
per call, eps_rel = 1e-12 (BezOptimization.TRUE_MIN_EPS_REL), max_curv = 0.5, max_rate = 1.  The four calls are timed
INTERLEAVED -- curvature value, curvature with blocks, angular-rate value, angular-rate with blocks, curvature value, ... --
so that clock and neighbour drift fall on all of them alike.  Per call two figures:
  * call_ms:   HIP-event time of --inner back-to-back calls on one stream, divided by --inner (median, min, max of --reps)
  * kernel_ms: obtg_kernel_stats' device time of the launches of one call, in a pass of its own with profiling on
Node counts: the angular-rate search reports them (obtg_bern_extrema's nodes on obtg_ang_rate_poly's rows); the curvature
entry points have no such output, so the figure is a PROXY: rule_nodes below, the device's rule restated in float64 on the
device's own coefficients (obtg_curvature_poly), on the 128 items of the batch's base row -- see "not_measured"."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EPS, CURV, RATE = 1e-12, 0.5, 1.0


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


def _kappa(n, d):
    if not d > 0.0:
        return float("nan")
    k = n / (d * np.sqrt(d))
    return k if np.isfinite(k) else float("nan")


def _bound(num, den):
    """extrema_kernels.hip PlanarCurv::ratio / curv_node_bound for a clamped row, in float64 (g's fma is a product and a sum here)"""
    pos = num > 0.0
    if not pos.any():
        return 0.0
    dmin, dmax = den.min(), den.max()
    if not dmin > 0.0:
        return float("inf")
    d0 = 0.5 * (dmin + dmax)
    s0 = np.sqrt(d0)
    a, c = 1.5 * s0, -0.5 * (d0 * s0)
    if not a * dmin + c > 0.0:
        return float("inf")
    return float((num[pos] / (a * den[pos] + c)).max())


def _halves(c):
    left, right, row = [c[0]], [c[-1]], c
    while len(row) > 1:
        row = 0.5 * row[:-1] + 0.5 * row[1:]
        left.append(row[0])
        right.append(row[-1])
    return np.array(left), np.array(right[::-1])


def rule_nodes(num, den, W, eps, max_nodes=100000):
    """Sub-curves the device's rule examines on one clamped item (curv_first, curv_wave_search under PlanarCurv: the same incumbent, bound, closing
    test and order of descent), restated in float64 on the device's own coefficients: a count, not the device's counter."""
    if not num.any():
        return 1
    U = 0.0
    for k in (_kappa(num[0], den[0]), _kappa(num[-1], den[-1])):
        U = k if k > U else U
    if not _bound(num, den) - U > eps * max(W, abs(U)):
        return 1
    nodes, stack, cur = 1, [], (num, den)
    while cur is not None and nodes + 2 <= max_nodes:
        (nl, nr), (dl, dr) = _halves(cur[0]), _halves(cur[1])
        nodes += 2
        km = _kappa(nl[-1], dl[-1])
        U = km if km > U else U
        tol = eps * max(W, abs(U))
        kids = [(b, n_, d_) for b, n_, d_ in ((_bound(nl, dl), nl, dl), (_bound(nr, dr), nr, dr)) if b - U > tol]
        if len(kids) == 2:
            if len(stack) == 32:
                break
            first = 0 if kids[0][0] >= kids[1][0] else 1
            stack.append(kids[1 - first])
            cur = kids[first][1:]
        elif kids:
            cur = kids[0][1:]
        else:
            cur = None
            while stack:
                b, n_, d_ = stack.pop()
                if b - U > tol:
                    cur = (n_, d_)
                    break
    return nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "curvature_time.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    N, d, n = 64, 2, 10
    ang = 2.0 * np.pi * np.arange(N) / N
    ring = np.stack([50.0 + 45.0 * np.cos(ang), 50.0 + 45.0 * np.sin(ang)], axis=1)
    bo = BezOptimization(numVeh=N, dimension=2, degree=n, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=30.0, maxAngRate=RATE,
                         tf=10.0, initPoints=[tuple(p) for p in ring], finalPoints=[tuple(p) for p in 100.0 - ring],
                         angRateRows='true_min', maxCurvature=CURV)
    x = bo.generateGuess(std=0.3, seed=1234)
    X, _ = bo._fd_rows(x)
    Yb = np.ascontiguousarray(bo.reshapeVectors(X))
    B = Yb.shape[0]
    dev = torch.device("cuda", 0)
    ctx = _capi.Context(N, d, n, 0, device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(Yb).to(dev)
    dtf = torch.full((B,), 10.0, dtype=torch.float64, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    out, ts, jtf, jac = f64(B, N, 2), f64(B, N, 2), f64(B, N, 2), f64(B, N, 2, 2, n + 1)
    st = {k: torch.empty((B, N, 2), dtype=torch.int32, device=dev) for k in ("curvature", "ang_rate")}
    P = lambda t: t.data_ptr()      # noqa: E731
    fns = {
        "curvature_true_min_dev": lambda: ctx.curvature_true_min_dev(P(dY), B, CURV, P(out), P(ts), P(st["curvature"]), eps_rel=EPS),
        "curvature_true_min_jac_dev": lambda: ctx.curvature_true_min_jac_dev(P(dY), B, CURV, P(out), P(jac), P(ts), P(st["curvature"]), eps_rel=EPS),
        "ang_rate_true_min_dev": lambda: ctx.ang_rate_true_min_dev(P(dY), P(dtf), B, RATE, P(out), P(ts), P(st["ang_rate"]), eps_rel=EPS),
        "ang_rate_true_min_jac_dev": lambda: ctx.ang_rate_true_min_jac_dev(P(dY), P(dtf), B, RATE, P(out), P(jac), P(jtf), P(ts),
                                                                           P(st["ang_rate"]), eps_rel=EPS),
    }
    for _ in range(a.warmup):
        for f in fns.values():
            sample(f, a.inner)
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, f in fns.items():
            ms[k].append(sample(f, a.inner))
    res = {k: dict(call=summary(v)) for k, v in ms.items()}
    ctx.set_profiling(True)
    for k, f in fns.items():
        ctx.reset_kernel_stats()
        f()
        torch.cuda.synchronize()
        stats = ctx.kernel_stats()
        res[k]["kernel_ms"] = float(sum(t for t, _ in stats.values()))
        res[k]["launches"] = int(sum(c for _, c in stats.values()))
    ctx.set_profiling(False)
    torch.cuda.synchronize()
    status = {k: {str(code): int((v == code).sum().item()) for code in range(4)} for k, v in st.items()}
    # node counts: the angular-rate rows' from the device, the curvature rows' from the yardstick on the base row
    ctx.use_own_stream()
    rows = ctx.ang_rate_poly(Yb, 10.0, RATE)
    e = ctx.bern_extrema(rows.reshape(-1, 2 * n + 1), eps_rel=EPS, eps_abs=0.0)
    nodes_ang = dict(mean=float(e["nodes"].mean()), max=int(e["nodes"].max()), items=int(e["nodes"].size), source="obtg_bern_extrema")
    poly = ctx.curvature_poly(Yb[:1])[0]                      # the device's own coefficients of the base row: [N][2][2n+1]
    cn = [rule_nodes(sg * poly[v, 0], poly[v, 1], CURV, EPS) for v in range(N) for sg in (1.0, -1.0)]
    nodes_curv = dict(mean=float(np.mean(cn)), max=int(max(cn)), items=len(cn),
                      source="tools/curvature_time.py rule_nodes: the device's rule restated in float64 on obtg_curvature_poly's rows, base row")
    base_ang = e["nodes"].reshape(B, N, 2)[0]
    nodes_ang["base_row_mean"] = float(base_ang.mean())
    ctx.close()
    ratio = {k: res["curvature_true_min" + k]["call"]["median_ms"] / res["ang_rate_true_min" + k]["call"]["median_ms"] for k in ("_dev", "_jac_dev")}
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _capi.source_hash("extrema_kernels"), "eps_rel": EPS,
              "max_curv": CURV, "max_rate": RATE,
              "C3": dict(vehicles=N, degree=n, B=int(B), items=int(B * N * 2), inner=a.inner, calls=res, status=status,
                         nodes=dict(ang_rate=nodes_ang, curvature=nodes_curv), ratio_curvature_over_ang_rate=ratio),
              "not_measured": ["the curvature search's node counts on the device (the entry points have no nodes output): a float64 "
                               "restatement of its rule on the base row's 128 items stands in, a proxy",
                               "hardware counters (no rocprofv3 pass was made)", "degrees other than 10, the workspace path"]}
    print(json.dumps(result["C3"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
