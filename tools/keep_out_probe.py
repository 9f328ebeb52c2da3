#!/usr/bin/env python3
"""The keep-out rows on the MI355X beside the keep-in true margins of the same tree: a minimum over t of a maximum over faces
(k_keep_out: the wave on one item from its first node on) beside a minimum over t of one polynomial (true_min_body: one lane
per item, the wave search only for the items that need it).

    python tools/keep_out_probe.py [--reps 15] [--inner 10] [--out profiles/keep_out.json]

Shape: C3 (64 vehicles, degree 10, d = 2) on the finite-difference batch of one iterate, B = 1153 rows (n_x + 1), against 8
square obstacles of 4 faces, 6 wide, on a circle of radius 20 about the centre the swarm crosses: 590 336 keep-out items per
call; the keep-in yardstick is a box of 4 faces, 295 168 items.  eps_rel = 1e-12 (BezOptimization.TRUE_MIN_EPS_REL).  The far
variant moves every obstacle 300 away: every root closes at node 1.  Every figure is KERNEL time: obtg_kernel_stats' device
time of all launches of --inner calls, divided by --inner, in a sample of its own; --reps samples per call, the calls
INTERLEAVED, so that clock and neighbour drift fall on all of them alike.  Reported: median, min and max, the median per
item, and the node histogram of the near obstacles (mean, maximum, share of items that close at the root)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EPS = 1e-12


def summary(ms, items):
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size), items=int(items),
                median_ns_per_item=float(np.median(ms)) * 1e6 / items)


def squares(shift=0.0, count=8, radius=20.0, half=3.0):
    ang = 2.0 * np.pi * (np.arange(count) + 0.5) / count
    A = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    out = []
    for cx, cy in zip(50.0 + shift + radius * np.cos(ang), 50.0 + radius * np.sin(ang)):
        out.append((A, np.array([cx + half, cy + half, -(cx - half), -(cy - half)])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keep_out.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization, _keep_in_tables, _keep_out_tables
    N, d, n = 64, 2, 10
    ang = 2.0 * np.pi * np.arange(N) / N
    ring = np.stack([50.0 + 45.0 * np.cos(ang), 50.0 + 45.0 * np.sin(ang)], axis=1)
    box = (np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]), np.array([72.5, -27.5, 72.5, -27.5]))
    bo = BezOptimization(numVeh=N, dimension=2, degree=n, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=30.0, maxAngRate=1.0,
                         tf=10.0, initPoints=[tuple(p) for p in ring], finalPoints=[tuple(p) for p in 100.0 - ring])
    x = bo.generateGuess(std=0.3, seed=1234)
    X, _ = bo._fd_rows(x)
    Yb = np.ascontiguousarray(bo.reshapeVectors(X))
    B = Yb.shape[0]
    Hk, VF = _keep_in_tables(box, N, d)
    near_t, far_t = _keep_out_tables(squares(), N, d), _keep_out_tables(squares(300.0), N, d)
    P_, Pk = near_t[2].shape[0], VF.shape[0]
    dev = torch.device("cuda", 0)
    ctx, far = _capi.Context(N, d, n, 0, device=0), _capi.Context(N, d, n, 0, device=0)
    ctx.set_keep_in(Hk, VF)
    ctx.set_keep_out(*near_t)
    far.set_keep_out(*far_t)
    for c in (ctx, far):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(Yb).to(dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
    out, ts, lam, bnd, jac = f64(B, P_), f64(B, P_), f64(B, P_), f64(B, P_), f64(B, P_, d, n + 1)
    face, nodes, st = i32(B, P_, 2), i32(B, P_), i32(B, P_)
    out_f, nodes_f = f64(B, P_), i32(B, P_)
    out_k, ts_k, st_k = f64(B, Pk), f64(B, Pk), i32(B, Pk)
    p = lambda t: t.data_ptr()      # noqa: E731
    fns = {
        "keep_out_true_min_dev": (ctx, lambda: ctx.keep_out_true_min_dev(p(dY), B, p(out), p(ts), p(face), p(lam), p(bnd), p(nodes), p(st),
                                                                         eps_rel=EPS), B * P_),
        "keep_out_true_min_jac_dev": (ctx, lambda: ctx.keep_out_true_min_jac_dev(p(dY), B, p(out), p(jac), p(ts), p(face), p(lam), p(bnd),
                                                                                 p(nodes), p(st), eps_rel=EPS), B * P_),
        "keep_out_true_min_dev_far": (far, lambda: far.keep_out_true_min_dev(p(dY), B, p(out_f), d_nodes=p(nodes_f), eps_rel=EPS), B * P_),
        "keep_in_true_min_dev": (ctx, lambda: ctx.keep_in_true_min_dev(p(dY), B, p(out_k), p(ts_k), p(st_k), eps_rel=EPS), B * Pk),
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
    for c in (ctx, far):
        c.set_profiling(False)
    torch.cuda.synchronize()
    res = {k: summary(v, fns[k][2]) for k, v in ms.items()}
    nd, ndf, t_, v_, f_ = nodes.cpu().numpy(), nodes_f.cpu().numpy(), ts.cpu().numpy(), out.cpu().numpy(), face.cpu().numpy()
    inside = (t_ > 0) & (t_ < 1)
    shape = dict(keep_out=dict(items=int(nd.size), nodes_mean=float(nd.mean()), nodes_max=int(nd.max()), closed_at_the_root=int((nd == 1).sum()),
                               nodes_mean_of_searched_items=float(nd[nd > 1].mean()) if (nd > 1).any() else 0.0,
                               interior_minimisers=int(inside.sum()), kinks=int((f_[..., 1] >= 0).sum()), penetrating=int((v_ < 0).sum()),
                               status_ok=int((st.cpu().numpy() == 0).sum())),
                 keep_out_far=dict(items=int(ndf.size), nodes_mean=float(ndf.mean()), nodes_max=int(ndf.max())))
    for c in (ctx, far):
        c.use_own_stream()
        c.close()
    ki = res["keep_in_true_min_dev"]["median_ns_per_item"]
    ratio = {k: res[k]["median_ns_per_item"] / ki for k in res if k != "keep_in_true_min_dev"}
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _capi.source_hash("keepout_kernels"), "eps_rel": EPS,
              "C3": dict(vehicles=N, degree=n, B=int(B), obstacles=8, faces_per_obstacle=4, inner=a.inner, kernel_time=res, batch=shape,
                         ratio_over_keep_in_true_min_per_item=ratio),
              "not_measured": ["call time on the host side (HIP events around the calls)", "hardware counters (no rocprofv3 pass was made): "
                               "what binds the kernel -- issue, LDS or the dependent chain -- is argued from the resource file and these "
                               "times only", "degrees other than 10, 3-D", "a finishing step at kinks (not built)"]}
    print(json.dumps(result["C3"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
