#!/usr/bin/env python3
"""The HOST-CALL time of the keep-out _jac entry points on the MI355X, this tree beside the library of the parent commit.

    python tools/keep_out_host_path_probe.py --parent-lib PATH/libobtg_hip.so [--reps 9] [--first CALL] [--append] [--out profiles/keep_out_host_path.json]

The kernels of the two libraries are the same instructions; what a change of the host path can move is the call around them:
uploads, workspace reservations, downloads.  Timed is the wall clock of one Python call (time.perf_counter around it; the call
ends with its one synchronise) of
    keep_out_true_min_jac, keep_out_euclid_true_min_jac, keep_out_moving_true_min_jac, pair_keep_out_true_min_jac
at B = 1 (the SLSQP callback's shape, where the host path dominates; a sample is the mean of --inner-one calls) and at
B = 1153, the finite-difference batch of tools/keep_out_probe.py (C3: 64 vehicles, degree 10, d = 2; 8 squares of 4 faces; the
motion of tools/keep_out_moving_probe.py; the pairs against a square of half-width 1.5: 2016 pairs a row; a sample is one call).
Both libraries run under THIS tree's Python: the parent's in a child process of its own (a process holds one library), asked
for one sample at a time, so the samples of the two are INTERLEAVED one by one; which of the two goes first alternates from
round to round, and --first says which call a round begins with (a rotation of the four), so that a sample's place in the
round cannot pass for a difference between the libraries.  The criterion is the project's usual one: the
new median within the parent's own min-max spread, per call and B."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

EPS = 1e-12
CALLS = ("keep_out_true_min_jac", "keep_out_euclid_true_min_jac", "keep_out_moving_true_min_jac", "pair_keep_out_true_min_jac")
HALF = 1.5


class Runner(object):
    """The four calls on the library this process loaded"""

    def __init__(self, inner_one):
        import torch  # noqa: F401  (both processes load the same modules)
        from keep_out_moving_probe import batch
        from optimalbeziertrajectorygeneration_amd import _capi
        self._capi, self.inner_one = _capi, inner_one
        N, d, n, Yb, tables, motion, tf = batch()
        self.Y, self.tf, self.shape = Yb, tf, dict(vehicles=N, degree=n, d=d, B=int(Yb.shape[0]), obstacle_items=int(tables[2].shape[0]),
                                                   pairs=N * (N - 1) // 2)
        region = np.array([[1.0, 0.0, HALF], [0.0, 1.0, HALF], [-1.0, 0.0, HALF], [0.0, -1.0, HALF]])
        # a context per family: the Euclidean call refuses a context with a motion
        self.ctx = {name: _capi.Context(N, d, n, 0, device=0) for name in CALLS}
        for name in CALLS[:3]:
            self.ctx[name].set_keep_out(*tables)
        self.ctx[CALLS[2]].set_keep_out_motion(*motion)
        self.ctx[CALLS[3]].set_pair_keep_out(region)

    def hash(self):
        return self._capi.source_hash("all")

    def sample(self, name, B):
        Y, call = self.Y[:B], getattr(self.ctx[name], name)
        args = (Y, self.tf[:B]) if "moving" in name else (Y,)
        inner = self.inner_one if B == 1 else 1
        t0 = time.perf_counter()
        for _ in range(inner):
            r = call(*args, eps_rel=EPS)
        dt = (time.perf_counter() - t0) / inner
        assert np.isfinite(r["val"]).all() and r["jac"].shape[:2] == r["val"].shape
        return dt * 1e3

    def close(self):
        for c in self.ctx.values():
            c.close()


def worker(inner_one):
    """The child: this tree's Python on the parent's library (OBTG_LIB); one sample per line read"""
    run = Runner(inner_one)
    print("ready %s" % run.hash(), flush=True)
    for line in sys.stdin:
        word = line.split()
        if len(word) != 3 or word[0] != "sample":
            break
        print("%.9f" % run.sample(word[1], int(word[2])), flush=True)
    run.close()


def summary(ms):
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=int(ms.size))


def write(path, result, append):
    """The file holds {"runs": [...]}: one entry per run of the probe; append: keep the runs the file has (same two libraries only)"""
    runs = []
    if append and os.path.exists(path):
        with open(path) as f:
            runs = json.load(f)["runs"]
        assert all((r["source_hash"], r["parent_source_hash"]) == (result["source_hash"], result["parent_source_hash"]) for r in runs)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"runs": runs + [result]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner-one", type=int, default=50, help="calls per sample at B = 1")
    ap.add_argument("--parent-lib", required=True, help="libobtg_hip.so built from the parent commit")
    ap.add_argument("--first", default=CALLS[0], choices=CALLS, help="the call each round begins with (the order is a rotation of CALLS)")
    ap.add_argument("--append", action="store_true", help="add this run to the runs --out already holds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keep_out_host_path.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.inner_one)
    import torch
    env = dict(os.environ, OBTG_LIB=os.path.abspath(a.parent_lib))
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--parent-lib", a.parent_lib, "--inner-one",
                              str(a.inner_one)], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    ready = child.stdout.readline().split()
    assert ready and ready[0] == "ready", ready
    run = Runner(a.inner_one)

    def parent(name, B):
        child.stdin.write("sample %s %d\n" % (name, B))
        child.stdin.flush()
        return float(child.stdout.readline())
    sizes = (1, run.shape["B"])
    order = CALLS[CALLS.index(a.first):] + CALLS[:CALLS.index(a.first)]
    ms = {(who, name, B): [] for who in ("new", "parent") for name in CALLS for B in sizes}
    for rep in range(a.warmup + a.reps):
        for name in order:
            for B in sizes:
                sides = (("new", run.sample), ("parent", parent))
                for who, fn in (sides if rep % 2 == 0 else sides[::-1]):        # which side goes first alternates by round
                    t = fn(name, B)
                    if rep >= a.warmup:
                        ms[(who, name, B)].append(t)
    child.stdin.write("quit\n")
    child.stdin.flush()
    child.wait(timeout=120)
    calls, within = {}, True
    for name in CALLS:
        for B in sizes:
            new, par = summary(ms[("new", name, B)]), summary(ms[("parent", name, B)])
            ok = par["min_ms"] <= new["median_ms"] <= par["max_ms"]
            within = within and ok
            calls["%s B=%d" % (name, B)] = dict(new=new, parent=par, new_median_within_parent_spread=bool(ok),
                                                new_over_parent_median=new["median_ms"] / par["median_ms"],
                                                parent_spread_over_median=(par["max_ms"] - par["min_ms"]) / par["median_ms"])
    result = {"device": torch.cuda.get_device_name(0), "source_hash": run.hash(), "parent_source_hash": ready[1], "eps_rel": EPS, "order_of_a_round": list(order), "side_first": "alternates by round",
              "what": "wall clock of one Python call in ms (host call: uploads, reservations, launch, downloads, one synchronise); "
                      "B = 1: the mean of %d calls a sample" % a.inner_one,
              "batch": dict(run.shape, pair_region_half_width=HALF), "calls": calls, "every_new_median_within_parent_spread": bool(within),
              "not_measured": ["kernel time (the kernels are the same instructions)", "the _dev entry points", "3-D",
                               "the value calls and the free-curve calls"]}
    run.close()
    print(json.dumps({k: (v["new"]["median_ms"], v["parent"]["median_ms"], v["new_median_within_parent_spread"]) for k, v in calls.items()}))
    write(a.out, result, a.append)


if __name__ == "__main__":
    main()
