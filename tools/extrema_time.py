#!/usr/bin/env python3
"""The true-extrema launches on the MI355X, beside the existing route to a tight separation value.

    python tools/extrema_time.py [--reps 20] [--out profiles/extrema_time.json]

One process, HIP events (torch.cuda.Event on the stream the context is bound to), medians and min / max over --reps timed
launches after --warmup:
  * obtg_bern_extrema_dev on 1 M random rows of K = 21 (coefficients uniform in [-10, 10]), eps_rel = 1e-9;
  * obtg_temporal_sep_true_min_dev at the C3 shape (64 vehicles, degree 10, B = 1153) and the C5 shape (64 vehicles + 32
    point obstacles = 96 objects, degree 10, B = 1153), each beside obtg_temporal_sep_min_dev at R = 0 and at R = 100 on
    the same Y.
With every launch: the histogram of sub-curves examined per row and the share of rows that end at node 1.
Reported, not gated."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def events(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(reps))


def node_stats(nodes):
    nodes = np.asarray(nodes).ravel()
    edges = [0, 1, 2, 4, 8, 16, 32, 64, 128, 1 << 30]
    hist = np.histogram(nodes, bins=edges)[0]
    return dict(rows=int(nodes.size), share_node1=float((nodes <= 1).mean()), median=float(np.median(nodes)), max=int(nodes.max()),
                histogram={"%d-%d" % (edges[i], edges[i + 1] - 1) if i + 2 < len(edges) else ">=%d" % edges[i]: int(h)
                           for i, h in enumerate(hist)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "extrema_time.json"))
    a = ap.parse_args()
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "eps_rel": 1e-9, "source_hash": _capi.source_hash("all")}

    # ---- obtg_bern_extrema on 1 M rows of K = 21
    M, K = 1 << 20, 21
    rng = np.random.default_rng(1234)
    dc = torch.from_numpy(rng.uniform(-10.0, 10.0, (M, K))).to(dev)
    dv, dt, db = (torch.empty(M, dtype=torch.float64, device=dev) for _ in range(3))
    dn, ds = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(2))
    ctx = _capi.scratch_context()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    t = events(lambda: ctx.bern_extrema_dev(dc.data_ptr(), M, K, dv.data_ptr(), dt.data_ptr(), db.data_ptr(), dn.data_ptr(),
                                            ds.data_ptr()), a.reps, a.warmup)
    t.update(rows=M, K=K, nodes=node_stats(dn.cpu().numpy()), status_not_ok=int((ds != 0).sum().item()))
    t["rows_per_s"] = M / (1e-3 * t["median_ms"])
    res["bern_extrema_1M_K21"] = t
    ctx.use_own_stream()
    print(json.dumps({"bern_extrema_1M_K21": t}))

    # ---- the fused consumer at the C3 and C5 shapes
    for name, n_obs in (("C3", 0), ("C5", 32)):
        N, d, n, B, max_sep = 64, 2, 10, 1153, 0.9
        Y = synth.swarm_control_points(N, d, n, seed=1234)
        Yb = synth.fd_batch(Y, B=B)
        obs = np.random.default_rng(7).uniform(0.0, 100.0, (n_obs, d)) if n_obs else None
        c = _capi.Context(N, d, n, 0, point_obs=obs, device=0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        P = c.num_pairs
        dY = torch.from_numpy(np.ascontiguousarray(Yb)).to(dev)
        out, ts = torch.empty((B, P), dtype=torch.float64, device=dev), torch.empty((B, P), dtype=torch.float64, device=dev)
        st = torch.empty((B, P), dtype=torch.int32, device=dev)
        mn = torch.empty((B, P), dtype=torch.float64, device=dev)
        r = {"B": B, "pairs": P, "objects": N + n_obs, "degree": n}
        r["true_min"] = events(lambda: c.temporal_sep_true_min_dev(dY.data_ptr(), B, max_sep, out.data_ptr(), ts.data_ptr(),
                                                                   st.data_ptr()), a.reps, a.warmup)
        r["true_min_value_only"] = events(lambda: c.temporal_sep_true_min_dev(dY.data_ptr(), B, max_sep, out.data_ptr()),
                                          a.reps, a.warmup)
        r["status_not_ok"] = int((st != 0).sum().item())
        for R in (0, 100):
            c.set_deg_elev(R)
            r["min_R%d" % R] = events(lambda: c.temporal_sep_min_dev(dY.data_ptr(), B, max_sep, mn.data_ptr()), a.reps, a.warmup)
            gap = (out - mn)
            r["min_R%d" % R]["largest_gap_to_true_min"] = float(gap.max().item())
            r["min_R%d" % R]["smallest_gap_to_true_min"] = float(gap.min().item())
        c.set_deg_elev(0)
        # node counts: the unfused route on the same rows (a sample of the batch's rows: the coefficients do go to memory here)
        rows = min(B, 64)
        full = torch.empty((rows, P * (2 * n + 1)), dtype=torch.float64, device=dev)
        c.temporal_sep_dev(dY.data_ptr(), rows, max_sep, full.data_ptr())
        nd = torch.empty(rows * P, dtype=torch.int32, device=dev)
        vv = torch.empty(rows * P, dtype=torch.float64, device=dev)
        c.bern_extrema_dev(full.data_ptr(), rows * P, 2 * n + 1, vv.data_ptr(), d_nodes=nd.data_ptr())
        torch.cuda.synchronize()
        r["nodes_first_%d_rows" % rows] = node_stats(nd.cpu().numpy())
        r["fused_equals_unfused_bits"] = bool(torch.equal(vv.view(torch.int64), out[:rows].reshape(-1).view(torch.int64)))
        c.use_own_stream()
        c.close()
        res[name] = r
        print(json.dumps({name: r}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
