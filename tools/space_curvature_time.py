#!/usr/bin/env python3
"""The space-curvature rows on the MI355X beside two calls whose code this family did not touch, their yardsticks: the planar
curvature rows (two polynomials per level, one square root per lane and child less) and the acceleration rows (one
polynomial, obtg_bern_extrema's search), on the same number of items in the same process.

    python tools/space_curvature_time.py [--reps 15] [--inner 10] [--out profiles/space_curvature_time.json]

Shape: C2 (8 vehicles in space, degree 10) on the finite-difference batch of one iterate, B = 217 rows (n_x + 1), 1736 items
per call, eps_rel = 1e-12 (BezOptimization.TRUE_MIN_EPS_REL), max_curv = 0.5.  The planar call runs 4 vehicles (two items
each) of the same degree on 217 rows of their finite-difference batch: 1736 items.  The four calls are timed INTERLEAVED --
space curvature value, with blocks, planar curvature value, acceleration value, space curvature value, ... -- so that clock
and neighbour drift fall on all of them alike.  Per call two figures:
  * call_ms:   HIP-event time of --inner back-to-back calls on one stream, divided by --inner (median, min, max of --reps)
  * kernel_ms: obtg_kernel_stats' device time of the launches of one call, in a pass of its own with profiling on
Node counts: the entry points have no such output; rule_nodes restates the device's rule in float64 on the device's own
coefficients (obtg_space_curvature_poly, obtg_curvature_poly) of the batch's base row -- a PROXY, see "not_measured"."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from curvature_time import sample, summary, rule_nodes as planar_rule_nodes, _halves  # noqa: E402

EPS, CURV, ACCEL = 1e-12, 0.5, 50.0


def _kappa(c):
    if not c[3] > 0.0:
        return float("nan")
    k = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) / (c[3] * np.sqrt(c[3]))
    return k if np.isfinite(k) else float("nan")


def _bound(co):
    """extrema_kernels.hip SpaceCurv3::ratio / curv_node_bound in float64 (g's fma is a product and a sum here)"""
    nu = np.sqrt(co[0] ** 2 + co[1] ** 2 + co[2] ** 2)
    if not nu.any():
        return 0.0
    dmin, dmax = co[3].min(), co[3].max()
    if not dmin > 0.0:
        return float("inf")
    d0 = 0.5 * (dmin + dmax)
    s0 = np.sqrt(d0)
    a, c = 1.5 * s0, -0.5 * (d0 * s0)
    if not a * dmin + c > 0.0:
        return float("inf")
    return float((nu / (a * co[3] + c)).max())


def rule_nodes(co, W, eps, max_nodes=100000):
    """Sub-curves the device's rule examines on one item (curv_first, curv_wave_search under SpaceCurv3: the same incumbent, bound, closing test and
    order of descent), restated in float64 on the device's own coefficients co[4][K]: a count, not the device's counter."""
    if not co[:3].any():
        return 1
    U = 0.0
    for k in (_kappa(co[:, 0]), _kappa(co[:, -1])):
        U = k if k > U else U
    if not _bound(co) - U > eps * max(W, U):
        return 1
    nodes, stack, cur = 1, [], co
    while cur is not None and nodes + 2 <= max_nodes:
        halves = [_halves(r) for r in cur]
        left, right = np.array([h[0] for h in halves]), np.array([h[1] for h in halves])
        nodes += 2
        km = _kappa(left[:, -1])
        U = km if km > U else U
        tol = eps * max(W, U)
        kids = [(b, c) for b, c in ((_bound(left), left), (_bound(right), right)) if b - U > tol]
        if len(kids) == 2:
            if len(stack) == 32:
                break
            first = 0 if kids[0][0] >= kids[1][0] else 1
            stack.append(kids[1 - first])
            cur = kids[first][1]
        elif kids:
            cur = kids[0][1]
        else:
            cur = None
            while stack:
                b, c = stack.pop()
                if b - U > tol:
                    cur = c
                    break
    return nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "space_curvature_time.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    sys.path.insert(0, os.path.join(REPO, "examples"))
    from example2_swarm_3d import crossing_swarm
    N, n = 8, 10
    init, final = crossing_swarm(N)
    bo = BezOptimization(numVeh=N, dimension=3, degree=n, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=30.0, tf=10.0,
                         initPoints=init, finalPoints=final, maxSpaceCurvature=CURV)
    x = bo.generateGuess(std=0.2, seed=2)
    X, _ = bo._fd_rows(x)
    Yb = np.ascontiguousarray(bo.reshapeVectors(X))
    B = Yb.shape[0]
    # the planar yardstick's batch: the x and y rows of the first N / 2 vehicles, B rows of their finite-difference batch
    Y2 = np.ascontiguousarray(synth.fd_batch(np.concatenate([Yb[0, 3 * v:3 * v + 2] for v in range(N // 2)]), B=B))
    dev = torch.device("cuda", 0)
    c3, c2 = _capi.Context(N, 3, n, 0, device=0), _capi.Context(N // 2, 2, n, 0, device=0)
    for c in (c3, c2):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
    dY, dY2 = torch.from_numpy(Yb).to(dev), torch.from_numpy(Y2).to(dev)
    dtf = torch.full((B,), 10.0, dtype=torch.float64, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    out, ts, jac = f64(B, N), f64(B, N), f64(B, N, 3, n + 1)
    st = {k: torch.empty((B, N), dtype=torch.int32, device=dev) for k in ("space_curvature", "curvature", "accel")}
    P = lambda t: t.data_ptr()      # noqa: E731
    fns = {
        "space_curvature_true_min_dev": (c3, lambda: c3.space_curvature_true_min_dev(P(dY), B, CURV, P(out), P(ts), P(st["space_curvature"]), eps_rel=EPS)),
        "space_curvature_true_min_jac_dev": (c3, lambda: c3.space_curvature_true_min_jac_dev(P(dY), B, CURV, P(out), P(jac), P(ts),
                                                                                             P(st["space_curvature"]), eps_rel=EPS)),
        "curvature_true_min_dev": (c2, lambda: c2.curvature_true_min_dev(P(dY2), B, CURV, P(out), P(ts), P(st["curvature"]), eps_rel=EPS)),
        "accel_true_min_dev": (c3, lambda: c3.accel_true_min_dev(P(dY), P(dtf), B, ACCEL, P(out), P(ts), P(st["accel"]), eps_rel=EPS)),
    }
    for _ in range(a.warmup):
        for _, f in fns.values():
            sample(f, a.inner)
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, (_, f) in fns.items():
            ms[k].append(sample(f, a.inner))
    res = {k: dict(call=summary(v)) for k, v in ms.items()}
    for k, (c, f) in fns.items():
        c.set_profiling(True)
        c.reset_kernel_stats()
        f()
        torch.cuda.synchronize()
        stats = c.kernel_stats()
        res[k]["kernel_ms"] = float(sum(t for t, _ in stats.values()))
        res[k]["launches"] = int(sum(n_ for _, n_ in stats.values()))
        c.set_profiling(False)
    torch.cuda.synchronize()
    status = {k: {str(code): int((v == code).sum().item()) for code in range(4)} for k, v in st.items()}
    for c in (c3, c2):
        c.use_own_stream()
    poly3 = c3.space_curvature_poly(Yb[:1])[0]                 # [N][4][2n+1]
    poly2 = c2.curvature_poly(Y2[:1])[0]                       # [N/2][2][2n+1]
    n3 = [rule_nodes(poly3[v], CURV, EPS) for v in range(N)]
    n2 = [planar_rule_nodes(sg * poly2[v, 0], poly2[v, 1], CURV, EPS) for v in range(N // 2) for sg in (1.0, -1.0)]
    nodes = dict(space_curvature=dict(mean=float(np.mean(n3)), max=int(max(n3)), items=len(n3)),
                 curvature=dict(mean=float(np.mean(n2)), max=int(max(n2)), items=len(n2)),
                 source="rule_nodes: the device's rules restated in float64 on the device's own coefficients, base row")
    for c in (c3, c2):
        c.close()
    med = lambda k: res[k]["call"]["median_ms"]      # noqa: E731
    ratio = {"space_over_planar_curvature": med("space_curvature_true_min_dev") / med("curvature_true_min_dev"),
             "space_over_accel": med("space_curvature_true_min_dev") / med("accel_true_min_dev"),
             "blocks_over_values": med("space_curvature_true_min_jac_dev") / med("space_curvature_true_min_dev")}
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _capi.source_hash("extrema_kernels"), "eps_rel": EPS,
              "max_curv": CURV, "accel_bound": ACCEL,
              "C2": dict(vehicles=N, degree=n, B=int(B), items=int(B * N), planar_vehicles=N // 2, inner=a.inner, calls=res,
                         status=status, nodes=nodes, ratio=ratio),
              "not_measured": ["the searches' node counts on the device (the entry points have no nodes output): a float64 "
                               "restatement of the rules on the base row's items stands in, a proxy",
                               "hardware counters (no rocprofv3 pass was made)",
                               "degrees other than 10, the workspace form, batches larger than C2's 1736 items"]}
    print(json.dumps(result["C2"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
