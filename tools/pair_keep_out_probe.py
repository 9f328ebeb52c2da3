#!/usr/bin/env python3
"""The vehicle-pair separation rows on the MI355X beside the static keep-out rows on the SAME relative curves, and beside the
moving rows at their own shape (tools/keep_out_moving_probe.py).

    python tools/pair_keep_out_probe.py [--reps 15] [--inner 10] [--out profiles/pair_keep_out.json]

Batch: C3's swarm (64 vehicles, degree 10, d = 2, tools/keep_out_moving_probe.py's problem), the first B = 293 rows of the
finite-difference batch of one iterate, every pair of vehicles: P = 2016, 590 688 items per call, faces metric, the region a
square of half-width 2, eps_rel = 1e-12.  Four calls, INTERLEAVED sample by sample:
    pair            obtg_pair_keep_out_true_min_dev on the vehicles' control points;
    pair_static     obtg_keep_out_true_min_dev on a context of 2016 vehicles whose control points are the PRECOMPUTED rel of the
                    pair call, the region their one obstacle: the same searches, node for node (asserted);
    moving          obtg_keep_out_moving_true_min_dev at the shape of DESIGN.md 4.25 (B = 1153, 8 squares: 590 336 items);
    moving_static   obtg_keep_out_true_min_dev on that shape.
Every figure is KERNEL time: obtg_kernel_stats' device time of --inner calls divided by --inner, a sample of its own.
Reported: median, min and max per call, pair / pair_static, moving / moving_static, and the nodes per item.  Expectation: the
pair prologue is one subtraction per control point where the moving one has about ten cross-lane levels per coordinate, so the
first ratio should not exceed the second."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

EPS = 1e-12
B_PAIR = 293
HALF = 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_keep_out.json"))
    a = ap.parse_args()
    import torch
    import keep_out_moving_probe as mv
    from optimalbeziertrajectorygeneration_amd import _capi
    N, d, n, Yb, tables, motion, tf = mv.batch()
    Bm, Pm = Yb.shape[0], tables[2].shape[0]
    Yp = np.ascontiguousarray(Yb[:B_PAIR])
    P = N * (N - 1) // 2
    H = np.array([[1.0, 0.0, HALF], [0.0, 1.0, HALF], [-1.0, 0.0, HALF], [0.0, -1.0, HALF]])
    dev = torch.device("cuda", 0)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
    p = lambda t: t.data_ptr()      # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    pair_ctx, stat_ctx, mov_ctx = _capi.Context(N, d, n, 0, device=0), _capi.Context(P, d, n, 0, device=0), _capi.Context(N, d, n, 0, device=0)
    ctxs = (pair_ctx, stat_ctx, mov_ctx)
    pair_ctx.set_pair_keep_out(H)
    stat_ctx.set_keep_out(H, np.array([0, 4], np.int32), np.stack((np.arange(P), np.zeros(P, int)), axis=1).astype(np.int32))
    mov_ctx.set_keep_out(*tables)
    mov_ctx.set_keep_out_motion(*motion)
    for c in ctxs:
        c.set_stream(stream)
    dYp, dYm, dtf = torch.from_numpy(Yp).to(dev), torch.from_numpy(Yb).to(dev), torch.from_numpy(tf).to(dev)
    rel = f64(B_PAIR, P, d, n + 1)
    outs = {k: ([f64(*s) for _ in range(4)], i32(*s, 2), i32(*s), i32(*s))
            for k, s in (("pair", (B_PAIR, P)), ("pair_static", (B_PAIR, P)), ("moving", (Bm, Pm)), ("moving_static", (Bm, Pm)))}

    def args(k):
        o, face, nodes, st = outs[k]
        return p(o[0]), p(o[1]), p(face), p(o[2]), p(o[3]), p(nodes), p(st)
    # rel once, with the pair call's other outputs: what the static context searches
    pair_ctx.pair_keep_out_true_min_dev(p(dYp), B_PAIR, *args("pair"), p(rel), eps_rel=EPS)
    torch.cuda.synchronize()
    fns = {
        "pair": (pair_ctx, lambda: pair_ctx.pair_keep_out_true_min_dev(p(dYp), B_PAIR, *args("pair"), eps_rel=EPS)),
        "pair_static": (stat_ctx, lambda: stat_ctx.keep_out_true_min_dev(p(rel), B_PAIR, *args("pair_static"), eps_rel=EPS)),
        "moving": (mov_ctx, lambda: mov_ctx.keep_out_moving_true_min_dev(p(dYm), p(dtf), Bm, *args("moving"), eps_rel=EPS)),
        "moving_static": (mov_ctx, lambda: mov_ctx.keep_out_true_min_dev(p(dYm), Bm, *args("moving_static"), eps_rel=EPS)),
    }
    for c in ctxs:
        c.set_profiling(True)

    def sample(name):
        ctx, fn = fns[name]
        ctx.reset_kernel_stats()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        stats = ctx.kernel_stats()
        assert sum(k for _, k in stats.values()) == stats["speed"][1] == a.inner, stats      # one launch per call, under "speed"
        return stats["speed"][0] / a.inner
    order = list(fns)
    for _ in range(a.warmup):
        for k in order:
            sample(k)
    ms = {k: [] for k in order}
    for _ in range(a.reps):
        for k in order:
            ms[k].append(sample(k))
    for c in ctxs:
        c.set_profiling(False)
    torch.cuda.synchronize()
    res = {k: mv.summary(v) for k, v in ms.items()}
    nodes = {k: outs[k][2].cpu().numpy() for k in order}
    ok = {k: int((outs[k][3].cpu().numpy() == 0).sum()) for k in order}
    same = all(bool(torch.equal(x, y)) for x, y in zip(outs["pair"][0] + list(outs["pair"][1:]), outs["pair_static"][0] + list(outs["pair_static"][1:])))
    assert same, "the pair call and the static call on its rel differ"
    for c in ctxs:
        c.use_own_stream()
        c.close()
    items = {"pair": B_PAIR * P, "pair_static": B_PAIR * P, "moving": Bm * Pm, "moving_static": Bm * Pm}
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _capi.source_hash("keepout_kernels"), "eps_rel": EPS,
              "batch": dict(pair=dict(vehicles=N, pairs=P, degree=n, dim=d, B=B_PAIR, items=items["pair"], region="square, half-width %g" % HALF,
                                      metric="faces"),
                            moving=dict(vehicles=N, degree=n, B=int(Bm), obstacles=8, faces_per_obstacle=4, items=items["moving"],
                                        motion_degree=1, motion_span=mv.SPAN, tf=10.0), inner=a.inner),
              "kernel_time": res,
              "pair_over_static": res["pair"]["median_ms"] / res["pair_static"]["median_ms"],
              "moving_over_static": res["moving"]["median_ms"] / res["moving_static"]["median_ms"],
              "pair_equals_static_on_rel_bit_for_bit": same,
              "nodes": {k: mv.histogram(v) for k, v in nodes.items()}, "status_ok": ok,
              "ns_per_node": {k: 1e6 * res[k]["median_ms"] / float(nodes[k].sum()) for k in order},
              "not_measured": ["3-D", "the Euclidean metric", "hardware counters (no rocprofv3 pass was made)", "call time on the host side",
                               "the _jac call", "degrees other than 10"]}
    result["expectation_met"] = result["pair_over_static"] <= result["moving_over_static"]
    print(json.dumps({k: result[k] for k in ("kernel_time", "pair_over_static", "moving_over_static", "expectation_met")}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
