#!/usr/bin/env python3
"""The true arc-length objective on the MI355X, beside the control-polygon objective it stands next to.

    python tools/arc_length_probe.py [--reps 15] [--out profiles/arc_length.json]

Shape: C3 (64 vehicles, degree 10, d = 2) on the finite-difference batch of one iterate, B = 1153 rows (n_x + 1) -- 73 792
curves -- at eps_rel = 1e-12, the optimiser's setting.  Timed INTERLEAVED in one process: obtg_arc_length_obj_dev without and
with the gradient, and obtg_euclidean_obj (host entry, the only form it has; its kernel time is what is compared) on the same
batch, so that clock and neighbour drift fall on all alike.  Two figures per call:
    call     the HIP-event time of --inner back-to-back calls on one stream divided by --inner (the _dev calls only);
    kernel   obtg_kernel_stats of the call's kernel id over the same calls, in a pass of its own with events on that id alone
             (arc_length: the search kernel and the row sum together; bern: k_euclid).
Medians and min / max over --reps samples after --warmup.  Also recorded: the panel estimates per curve (mean, max) and the
statuses, from obtg_bern_arc_length_dev on the same curves.  The kernels' registers are the compiler's report, kept beside
this file's output as profiles/arc_length_kernel_resources.txt.  Reported, not gated."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EPS = 1e-12
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "arc_length.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    dev = torch.device("cuda", 0)
    ang = 2.0 * np.pi * np.arange(N) / N
    ring = np.stack([50.0 + 45.0 * np.cos(ang), 50.0 + 45.0 * np.sin(ang)], axis=1)
    bo = BezOptimization(numVeh=N, dimension=D, degree=DEG, minimizeGoal='arcLength', maxSep=0.9, maxSpeed=30.0, tf=10.0,
                         initPoints=[tuple(p) for p in ring], finalPoints=[tuple(p) for p in 100.0 - ring])
    x = bo.generateGuess(std=0.3, seed=1234)
    X, _ = bo._fd_rows(x)
    Yb = np.ascontiguousarray(bo.reshapeVectors(X))
    B = Yb.shape[0]
    c = _capi.Context(N, D, DEG, 0, device=0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(Yb).to(dev)
    out = torch.empty(B, dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    grad = torch.empty((B, N * D, DEG + 1), dtype=torch.float64, device=dev)
    fns = {"arc_length_obj": (lambda: c.arc_length_obj_dev(dY.data_ptr(), B, out.data_ptr(), st.data_ptr(), eps_rel=EPS), "arc_length"),
           "arc_length_obj_grad": (lambda: c.arc_length_obj_dev(dY.data_ptr(), B, out.data_ptr(), st.data_ptr(), grad.data_ptr(), eps_rel=EPS), "arc_length"),
           "euclidean_obj": (lambda: c.euclidean_obj(Yb), "bern")}
    for _ in range(a.warmup):
        for f, _k in fns.values():
            sample(f, a.inner)
    call = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, (f, _k) in fns.items():
            call[k].append(sample(f, a.inner))
    kern = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, (f, kid) in fns.items():
            c.set_profiling(True, only=kid)
            c.reset_kernel_stats()
            for _ in range(a.inner):
                f()
            torch.cuda.synchronize()
            ms, launches = c.kernel_stats()[kid]
            c.set_profiling(False)
            kern[k].append(ms / a.inner)
            assert launches == a.inner * (2 if kid == "arc_length" else 1), (k, launches)
    r = {k: dict(kernel=summary(kern[k])) for k in fns}
    for k in ("arc_length_obj", "arc_length_obj_grad"):
        r[k]["call"] = summary(call[k])
    # what the search did on these curves
    M = B * N
    ln, er = (torch.empty(M, dtype=torch.float64, device=dev) for _ in range(2))
    nd, s2 = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(2))
    c.bern_arc_length_dev(dY.data_ptr(), M, D, DEG + 1, ln.data_ptr(), er.data_ptr(), nd.data_ptr(), s2.data_ptr(), eps_rel=EPS)
    torch.cuda.synchronize()
    nodes = nd.cpu().numpy()
    eu = c.euclidean_obj(Yb)
    r.update(vehicles=N, degree=DEG, dim=D, B=B, curves=M, inner=a.inner, eps_rel=EPS,
             nodes_mean=float(nodes.mean()), nodes_max=int(nodes.max()), status_not_ok=int((s2 != 0).sum().item()),
             length_over_polygon_row0=float(out[0].item() / eu[0]), grad_bytes=int(grad.numel() * 8))
    res = {"device": torch.cuda.get_device_name(0), "C3": r, "resources": "profiles/arc_length_kernel_resources.txt",
           "source_hash": {u: _capi.source_hash(u) for u in ("arclen_kernels", "bern_kernels")}}
    print(json.dumps(res["C3"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
    c.use_own_stream()
    c.close()


if __name__ == "__main__":
    main()
