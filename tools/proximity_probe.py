#!/usr/bin/env python3
"""The proximity rows on the MI355X beside the true-minimum separation rows, their yardstick: the same search (wave_search) on
the same polynomial up to sign and offset -- a `reach` row with the full window IS the separation row's search -- so a
full-window batch should sit near 1 and a windowed batch pays the window's cuts, d (n + 1)^2 multiply-adds per vehicle row.

    python tools/proximity_probe.py [--reps 15] [--inner 10] [--out profiles/proximity.json]

Shape, per dimension d = 2 and 3: 12 vehicles at degree 10, B = 1153 rows (SLSQP's finite-difference batch of a 64-vehicle planar
problem), P = 64 items -- the first 64 of the 66 vehicle pairs -- 73 792 items per call; beside them, in the same run,
obtg_temporal_sep_true_min[_jac] on the same rows' first 1118 (66 pairs: 73 788 items).  eps_rel = 1e-12
(BezOptimization.TRUE_MIN_EPS_REL).  Four proximity batches: reach and within, each with the full window and with the window
(0.25, 0.75).  The radius is the median end-point distance, so margins of both signs are in the batch.  Every figure is KERNEL
time: obtg_kernel_stats' device time of all launches of --inner calls, divided by --inner, in a sample of its own; --reps
samples per call, the calls INTERLEAVED so that clock and neighbour drift fall on all of them alike.  Reported: median, min and
max, the median per item, and the ratios of the per-item medians to the separation calls'."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EPS = 1e-12
N, DEG, B, P, B_SEP = 12, 10, 1153, 64, 1118


def summary(ms, items):
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size), items=int(items),
                median_ns_per_item=float(np.median(ms)) * 1e6 / items)


def measure(dim, a):
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    rng = np.random.RandomState(100 + dim)
    base = np.cumsum(rng.uniform(-1.0, 1.0, (N * dim, DEG + 1)), axis=1) + rng.uniform(-3.0, 3.0, (N * dim, 1))
    Yb = np.ascontiguousarray(base[None] + 1e-3 * rng.standard_normal((B, N * dim, DEG + 1)))
    pairs = [(i, j) for i in range(N - 1) for j in range(i + 1, N)][:P]
    ends = base.reshape(N, dim, -1)[:, :, 0]
    rho = float(np.median([np.linalg.norm(ends[i] - ends[j]) for i, j in pairs]))
    dev = torch.device("cuda", 0)
    dY = torch.from_numpy(Yb).to(dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
    p = lambda t: t.data_ptr()      # noqa: E731
    val, ts, bd, jac = f64(B, P), f64(B, P), f64(B, P), f64(B, P, dim, DEG + 1)
    nd, st = i32(B, P), i32(B, P)
    n_pairs = N * (N - 1) // 2
    val_s, ts_s, jac_s, st_s = f64(B_SEP, n_pairs), f64(B_SEP, n_pairs), f64(B_SEP, n_pairs, dim, DEG + 1), i32(B_SEP, n_pairs)
    ctxs, fns = [], {}
    for kind, kname in ((_capi.PROX_REACH, "reach"), (_capi.PROX_WITHIN, "within")):
        for win, wname in (((0.0, 1.0), "full"), ((0.25, 0.75), "windowed")):
            c = _capi.Context(N, dim, DEG, 0, device=0)
            c.set_proximity([(i, j, kind) for i, j in pairs], [(rho, win[0], win[1])] * P)
            ctxs.append(c)
            fns["proximity_true_dev_%s_%s" % (kname, wname)] = (
                c, lambda c=c: c.proximity_true_dev(p(dY), B, p(val), p(ts), p(bd), p(nd), p(st), eps_rel=EPS), B * P)
            fns["proximity_true_jac_dev_%s_%s" % (kname, wname)] = (
                c, lambda c=c: c.proximity_true_dev(p(dY), B, p(val), p(ts), p(bd), p(nd), p(st), p(jac), eps_rel=EPS), B * P)
    sep = _capi.Context(N, dim, DEG, 0, device=0)
    ctxs.append(sep)
    fns["temporal_sep_true_min_dev"] = (sep, lambda: sep.temporal_sep_true_min_dev(p(dY), B_SEP, rho, p(val_s), p(ts_s), p(st_s), eps_rel=EPS),
                                        B_SEP * n_pairs)
    fns["temporal_sep_true_min_jac_dev"] = (sep, lambda: sep.temporal_sep_true_min_jac_dev(p(dY), B_SEP, rho, p(val_s), p(jac_s), p(ts_s), p(st_s),
                                                                                           eps_rel=EPS), B_SEP * n_pairs)
    for c in ctxs:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.set_profiling(True)

    def sample(c, fn):
        c.reset_kernel_stats()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        stats = c.kernel_stats()
        assert sum(k for _, k in stats.values()) == a.inner, stats          # one launch per call
        return sum(ms for ms, _ in stats.values()) / a.inner
    for _ in range(a.warmup):
        for c, f, _ in fns.values():
            sample(c, f)
    ms = {k: [] for k in fns}
    shape = {}
    for _ in range(a.reps):
        for k, (c, f, _) in fns.items():
            ms[k].append(sample(c, f))
    for k, (c, f, _) in fns.items():                 # what each batch holds, from one more call
        if k.startswith("proximity_true_dev"):
            f()
            torch.cuda.synchronize()
            v, n_ = val.cpu().numpy(), nd.cpu().numpy()
            shape[k] = dict(negative_rows=int((v < 0).sum()), searches_that_split=int((n_ > 1).sum()), mean_nodes=float(n_.mean()),
                            status_ok=int((st.cpu().numpy() == 0).sum()))
    for c in ctxs:
        c.set_profiling(False)
        c.use_own_stream()
        c.close()
    res = {k: summary(v, fns[k][2]) for k, v in ms.items()}
    ratio = {k: res[k]["median_ns_per_item"] / res["temporal_sep_true_min" + ("_jac" if "_jac_" in k else "") + "_dev"]["median_ns_per_item"]
             for k in res if k.startswith("proximity")}
    return dict(vehicles=N, degree=DEG, dim=dim, B=B, items_per_row=P, radius=rho, inner=a.inner, kernel_time=res, batch=shape,
                ratio_proximity_over_temporal_sep_per_item=ratio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "proximity.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _capi.source_hash("extrema_kernels"), "eps_rel": EPS,
              "dim2": measure(2, a), "dim3": measure(3, a),
              "not_measured": ["call time on the host side (HIP events around the calls)", "hardware counters (no rocprofv3 pass was made)",
                               "degrees other than 10, the workspace route, point targets"]}
    for k in ("dim2", "dim3"):
        print(k, json.dumps(result[k]["ratio_proximity_over_temporal_sep_per_item"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
