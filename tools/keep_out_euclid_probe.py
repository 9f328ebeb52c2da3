#!/usr/bin/env python3
"""The Euclidean keep-out rows on the MI355X beside the faces rows of the same tree and of the parent commit.

    python tools/keep_out_euclid_probe.py --parent-lib PATH/libobtg_hip.so [--reps 15] [--inner 10] [--out profiles/keep_out_euclid.json]

Batch: tools/keep_out_probe.py's near batch, as tools/keep_out_moving_probe.py takes it -- C3 (64 vehicles, degree 10, d = 2),
the finite-difference batch of one iterate, B = 1153 rows, 8 squares of 4 faces (4 corners each): 590 336 items per call,
eps_rel = 1e-12.  Three calls, INTERLEAVED sample by sample:
    faces    obtg_keep_out_true_min_dev of this tree;
    parent   the same call of the library built from the parent commit (--parent-lib), in a child process of its own (a process
             holds one library), asked for one sample at a time;
    euclid   obtg_keep_out_euclid_true_min_dev of this tree.
Every figure is KERNEL time: obtg_kernel_stats' device time of --inner calls divided by --inner, a sample of its own.
Reported: median, min and max per call, whether the faces median lies within the parent's own min-max spread (the check that
the faces kernel was not disturbed), nodes per item under both metrics and the Euclidean call's time per node as a ratio to
the faces call's."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from keep_out_moving_probe import EPS, batch, histogram, summary  # noqa: E402


def worker(inner):
    """The child: this tree's Python on the parent's library (OBTG_LIB), the faces call alone; one sample per line read."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    for name in [k for k in _capi._SIGNATURES if "euclid" in k or k == "obtg_keep_out_features"]:
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keep_out_euclid.json"))
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
    N, d, n, Yb, tables, _, _ = batch()
    B, P = Yb.shape[0], tables[2].shape[0]
    dev = torch.device("cuda", 0)
    ctx = _capi.Context(N, d, n, 0, device=0)
    ctx.set_keep_out(*tables)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(Yb).to(dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
    p = lambda t: t.data_ptr()      # noqa: E731
    f_out, f_nodes, f_st = [f64(B, P) for _ in range(4)], i32(B, P), i32(B, P)
    e_out, e_nodes, e_st = [f64(B, P) for _ in range(3)], i32(B, P), i32(B, P)
    face, faces3, dirv = i32(B, P, 2), i32(B, P, 3), f64(B, P, d)
    fns = {
        "faces": lambda: ctx.keep_out_true_min_dev(p(dY), B, p(f_out[0]), p(f_out[1]), p(face), p(f_out[2]), p(f_out[3]), p(f_nodes),
                                                   p(f_st), eps_rel=EPS),
        "euclid": lambda: ctx.keep_out_euclid_true_min_dev(p(dY), B, p(e_out[0]), p(e_out[1]), p(faces3), p(dirv), p(e_out[2]), p(e_nodes),
                                                           p(e_st), eps_rel=EPS),
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
    order = ["faces"] + (["parent"] if child else []) + ["euclid"]
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
    nf, ne = f_nodes.cpu().numpy(), e_nodes.cpu().numpy()
    vf, ve = f_out[0].cpu().numpy(), e_out[0].cpu().numpy()
    ok = int((f_st.cpu().numpy() == 0).sum()), int((e_st.cpu().numpy() == 0).sum())
    ctx.use_own_stream()
    ctx.close()
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _capi.source_hash("keepout_kernels"),
              "parent_source_hash": ready[1] if child else None, "eps_rel": EPS,
              "batch": dict(vehicles=N, degree=n, B=int(B), obstacles=8, faces_per_obstacle=4, features_per_obstacle=4, items=int(B * P),
                            inner=a.inner),
              "kernel_time": res,
              "faces_within_parent_spread": (res["parent"]["min_ms"] <= res["faces"]["median_ms"] <= res["parent"]["max_ms"]) if child else None,
              "euclid_over_faces": res["euclid"]["median_ms"] / res["faces"]["median_ms"],
              "euclid_over_faces_per_node": (res["euclid"]["median_ms"] / float(ne.sum())) / (res["faces"]["median_ms"] / float(nf.sum())),
              "nodes": dict(faces=histogram(nf), euclid=histogram(ne), status_ok=dict(faces=ok[0], euclid=ok[1])),
              "rows": dict(euclid_above_faces_by_1e_6=int((ve > vf + 1e-6).sum()), largest_gain=float((ve - vf).max()),
                           euclid_below_faces=float((ve - vf).min())),
              "not_measured": ["hardware counters (no rocprofv3 pass was made)", "3-D and obstacles with many features (the octahedron's 48)",
                               "degrees other than 10", "the _jac call", "call time on the host side, the tables' first build included"]}
    print(json.dumps({k: result[k] for k in ("kernel_time", "faces_within_parent_spread", "euclid_over_faces", "euclid_over_faces_per_node")}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
