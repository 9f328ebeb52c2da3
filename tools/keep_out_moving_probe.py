#!/usr/bin/env python3
"""The moving keep-out rows on the MI355X beside the static rows of the same tree and of the parent commit.

    python tools/keep_out_moving_probe.py --parent-lib PATH/libobtg_hip.so [--reps 15] [--inner 10] [--out profiles/keep_out_moving.json]

Batch: tools/keep_out_probe.py's near batch -- C3 (64 vehicles, degree 10, d = 2), the finite-difference batch of one iterate,
B = 1153 rows, 8 squares of 4 faces on a circle of radius 20 about the centre the swarm crosses: 590 336 items per call,
eps_rel = 1e-12.  For the moving call every square moves along a straight line (degree 1) across the ring, through the centre
to the opposite place, on a span of 12.5 against the vehicles' tf = 10 (r = 0.8, the same for every row: the batch is the
static probe's).  Three calls, INTERLEAVED sample by sample:
    static   obtg_keep_out_true_min_dev of this tree;
    parent   the same call of the library built from the parent commit (--parent-lib), in a child process of its own (a process
             holds one library), asked for one sample at a time;
    moving   obtg_keep_out_moving_true_min_dev of this tree.
Every figure is KERNEL time: obtg_kernel_stats' device time of --inner calls divided by --inner, a sample of its own.
Reported: median, min and max per call, whether the static median lies within the parent's own min-max spread, the moving call
as a ratio to the static one, and the node histograms of both (a moving square meets other vehicles than a parked one)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

EPS = 1e-12
SPAN = 12.5


def batch():
    """(Yb[B][N d][n + 1], static tables, motion tables, tf[B]) of the probe"""
    from keep_out_probe import squares
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization, _keep_out_tables
    N, d, n = 64, 2, 10
    ang = 2.0 * np.pi * np.arange(N) / N
    ring = np.stack([50.0 + 45.0 * np.cos(ang), 50.0 + 45.0 * np.sin(ang)], axis=1)
    bo = BezOptimization(numVeh=N, dimension=2, degree=n, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=30.0, maxAngRate=1.0,
                         tf=10.0, initPoints=[tuple(p) for p in ring], finalPoints=[tuple(p) for p in 100.0 - ring])
    x = bo.generateGuess(std=0.3, seed=1234)
    X, _ = bo._fd_rows(x)
    Yb = np.ascontiguousarray(bo.reshapeVectors(X))
    sq = squares()
    tables = _keep_out_tables(sq, N, d)
    a8 = 2.0 * np.pi * (np.arange(8) + 0.5) / 8
    # square o starts where it stands and ends at the opposite place of the ring: the offset runs from 0 to -2 (its centre - (50, 50))
    Q = np.concatenate([np.array([[0.0, -40.0 * np.cos(t)], [0.0, -40.0 * np.sin(t)]]).reshape(-1) for t in a8])
    motion = (Q, np.arange(0, 17, 2, dtype=np.int32), np.full(8, SPAN))
    return N, d, n, Yb, tables, motion, np.full(Yb.shape[0], 10.0)


def summary(ms):
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size))


def histogram(nodes):
    nodes = np.asarray(nodes)
    edges = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 1 << 30]
    return dict(mean=float(nodes.mean()), max=int(nodes.max()), closed_at_the_root=int((nodes == 1).sum()),
                counts={"%d..%d" % (lo, hi - 1) if hi < (1 << 30) else "%d.." % lo: int(((nodes >= lo) & (nodes < hi)).sum())
                        for lo, hi in zip(edges[:-1], edges[1:])})


def worker(inner):
    """The child: this tree's Python on the parent's library (OBTG_LIB), the static call alone; one sample per line read."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    for name in [k for k in _capi._SIGNATURES if "moving" in k or "motion" in k]:
        del _capi._SIGNATURES[name]                     # (the parent's library does not have them)
    N, d, n, Yb, tables, _, _ = batch()
    B, P = Yb.shape[0], tables[2].shape[0]
    dev = torch.device("cuda", 0)
    ctx = _capi.Context(N, d, n, 0, device=0)
    ctx.set_keep_out(*tables)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(Yb).to(dev)
    out = [torch.empty((B, P), dtype=torch.float64, device=dev) for _ in range(4)]
    face, nodes, st = (torch.empty((B, P, 2) if k == 0 else (B, P), dtype=torch.int32, device=dev) for k in range(3))
    ctx.set_profiling(True)
    print("ready %s" % _capi.source_hash("keepout_kernels"), flush=True)
    for line in sys.stdin:
        if line.strip() != "sample":
            break
        ctx.reset_kernel_stats()
        for _ in range(inner):
            ctx.keep_out_true_min_dev(dY.data_ptr(), B, out[0].data_ptr(), out[1].data_ptr(), face.data_ptr(), out[2].data_ptr(),
                                      out[3].data_ptr(), nodes.data_ptr(), st.data_ptr(), eps_rel=EPS)
        torch.cuda.synchronize()
        print("%.9f" % (ctx.kernel_stats()["speed"][0] / inner), flush=True)
    ctx.use_own_stream()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--parent-lib", default=None, help="libobtg_hip.so built from the parent commit")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keep_out_moving.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.inner)
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    child = None
    if a.parent_lib:
        env = dict(os.environ, OBTG_LIB=os.path.abspath(a.parent_lib))
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--inner", str(a.inner)], env=env,
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        ready = child.stdout.readline().split()
        assert ready and ready[0] == "ready", ready
    N, d, n, Yb, tables, motion, tf = batch()
    B, P = Yb.shape[0], tables[2].shape[0]
    dev = torch.device("cuda", 0)
    ctx = _capi.Context(N, d, n, 0, device=0)
    ctx.set_keep_out(*tables)
    ctx.set_keep_out_motion(*motion)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dY, dtf = torch.from_numpy(Yb).to(dev), torch.from_numpy(tf).to(dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
    p = lambda t: t.data_ptr()      # noqa: E731
    s_out, s_nodes, s_st = [f64(B, P) for _ in range(4)], i32(B, P), i32(B, P)
    m_out, m_nodes, m_st = [f64(B, P) for _ in range(4)], i32(B, P), i32(B, P)
    face = i32(B, P, 2)
    fns = {
        "static": lambda: ctx.keep_out_true_min_dev(p(dY), B, p(s_out[0]), p(s_out[1]), p(face), p(s_out[2]), p(s_out[3]), p(s_nodes),
                                                    p(s_st), eps_rel=EPS),
        "moving": lambda: ctx.keep_out_moving_true_min_dev(p(dY), p(dtf), B, p(m_out[0]), p(m_out[1]), p(face), p(m_out[2]), p(m_out[3]),
                                                           p(m_nodes), p(m_st), eps_rel=EPS),
    }
    ctx.set_profiling(True)

    def sample(name):
        if name == "parent":
            child.stdin.write("sample\n")
            child.stdin.flush()
            return float(child.stdout.readline())
        ctx.reset_kernel_stats()
        for _ in range(a.inner):
            fns[name]()
        torch.cuda.synchronize()
        stats = ctx.kernel_stats()
        assert sum(k for _, k in stats.values()) == stats["speed"][1] == a.inner, stats      # one launch per call, under "speed"
        return stats["speed"][0] / a.inner
    order = ["static"] + (["parent"] if child else []) + ["moving"]
    for _ in range(a.warmup):
        for k in order:
            sample(k)
    ms = {k: [] for k in order}
    for _ in range(a.reps):
        for k in order:
            ms[k].append(sample(k))
    if child:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
    ctx.set_profiling(False)
    torch.cuda.synchronize()
    res = {k: summary(v) for k, v in ms.items()}
    ns, nm = s_nodes.cpu().numpy(), m_nodes.cpu().numpy()
    ok = int((s_st.cpu().numpy() == 0).sum()), int((m_st.cpu().numpy() == 0).sum())
    ctx.use_own_stream()
    ctx.close()
    K = n + 1
    per_coord = 1 * 2 // 2 + (n - 1)                         # m (m + 1) / 2 + (n - m) cross-lane levels, m = 1
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _capi.source_hash("keepout_kernels"),
              "parent_source_hash": ready[1] if child else None, "eps_rel": EPS,
              "batch": dict(vehicles=N, degree=n, B=int(B), obstacles=8, faces_per_obstacle=4, items=int(B * P), inner=a.inner,
                            motion_degree=1, motion_span=SPAN, tf=10.0),
              "kernel_time": res,
              "static_within_parent_spread": (res["parent"]["min_ms"] <= res["static"]["median_ms"] <= res["parent"]["max_ms"]) if child else None,
              "moving_over_static": res["moving"]["median_ms"] / res["static"]["median_ms"],
              "nodes": dict(static=histogram(ns), moving=histogram(nm), status_ok=dict(static=ok[0], moving=ok[1])),
              "expectation": dict(prologue_levels_per_coordinate=per_coord, split_levels_per_coordinate=K - 1,
                                  text="the prologue is m (m + 1) / 2 + (n - m) = %d cross-lane levels per coordinate against the "
                                       "mean number of splits per item of %d levels each, so a few percent on the same node counts "
                                       "(supposed, not measured); the moving squares meet other vehicles than the parked ones, so the "
                                       "node histograms differ and the ratio per NODE is the one to read" % (per_coord, K - 1),
                                  moving_over_static_per_node=(res["moving"]["median_ms"] / float(nm.sum())) / (res["static"]["median_ms"] / float(ns.sum()))),
              "not_measured": ["hardware counters (no rocprofv3 pass was made)", "3-D", "degrees other than 10, motion degrees other than 1",
                               "the _jac call", "call time on the host side"]}
    print(json.dumps({k: result[k] for k in ("kernel_time", "static_within_parent_spread", "moving_over_static")}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
