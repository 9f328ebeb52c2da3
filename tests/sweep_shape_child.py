"""The toy shapes of tests/test_gpu_sweep_shapes.py, their inputs and the calls that test makes on them -- and, run as a
program, a fresh process that makes the same calls under whatever OBTG_* switches its environment holds and leaves every
output array in an .npz (the switches read once per process cannot be flipped inside pytest's):

    python tests/sweep_shape_child.py OUT.npz [--elev R] [SHAPE ...]

Not collected by pytest (no test_ prefix)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# The smallest shapes at which a 256-lane workgroup must refill (one workgroup per row: more than 256 hull pairs).
# name -> N, degree, polygons, point obstacles, B, seed of the control points, seed of the polygons.  The seeds were picked on
# the CPU so that the oracle's results hold what tests/test_gpu_sweep_shapes.py::check_inputs asks for, and so that no polygon
# has more vertices than a hull has points (the planar kernels' condition).
SHAPES = {
    "refill_deg5": dict(N=24, n=5, M=2, n_obs=0, B=3, seed=21, pseed=3),
    "c3_like": dict(N=36, n=10, M=3, n_obs=0, B=9, seed=21, pseed=8),
    "deg3": dict(N=30, n=3, M=0, n_obs=0, B=8, seed=21, pseed=8),
    "deg7": dict(N=30, n=7, M=2, n_obs=0, B=1, seed=21, pseed=8),
    "deg8": dict(N=30, n=8, M=2, n_obs=0, B=1, seed=21, pseed=8),
    "deg15": dict(N=36, n=15, M=2, n_obs=0, B=2, seed=21, pseed=8),
    "deg20": dict(N=26, n=20, M=0, n_obs=0, B=2, seed=21, pseed=8),
    "point_obs": dict(N=23, n=10, M=3, n_obs=5, B=8, seed=21, pseed=8),
}
# rows beyond 48 KB of LDS: the tiled forms.  tiled_dups lists 4000 pairs twice: a tile overflows into a second chunk, so the
# tiles cannot carry the separation rows (two launches, the first of them the tiled plain sweep).
TILED = {
    "tiled_deg15": dict(N=256, n=15, M=5, n_obs=0, B=3, seed=21, pseed=8),
    "tiled_dups": dict(N=603, n=5, M=2, n_obs=0, B=2, seed=21, pseed=3, dups=4000),
}
PLAIN_ONLY = ("deg20",)                # no one-launch pair sweep at 21 points: the plain sweep alone
MAX_SEP, SPEED_BOUND, MAX_RATE, FD_H = 0.9, 5.0, 1.0, 0.01
GJK_KEYS = ("flag", "c1", "c2", "dist", "n_support", "status")


def inputs(name):
    """Yb: B rows of a finite-difference batch (h = 0.01), the middle one moved by N(0, 2) noise; Y: its row 0, the row an FD
    view is opened on; tf per row; polygons, hull pair list, point obstacles."""
    from optimalbeziertrajectorygeneration_amd import synth
    s = SHAPES.get(name) or TILED[name]
    N, n, M, B = s["N"], s["n"], s["M"], s["B"]
    Y = synth.swarm_control_points(N, 2, n, seed=s["seed"])
    Yb = synth.fd_batch(Y, B=B, h=FD_H)
    Yb[B // 2] += np.random.default_rng(4).normal(0, 2.0, size=Y.shape)
    polys = synth.polygon_obstacles(M, seed=s["pseed"]) if M else []
    pa, pb = synth.swarm_pairs(N, M)
    if s.get("dups"):
        pa, pb = np.concatenate([pa, pa[:s["dups"]]]), np.concatenate([pb, pb[:s["dups"]]])
    obs = np.random.default_rng(6).uniform(10, 90, size=(s["n_obs"], 2)) if s["n_obs"] else None
    return dict(name=name, N=N, n=n, M=M, B=B, Y=Y, Yb=Yb, Yfd=synth.fd_batch(Y, B=B, h=FD_H), polys=polys, pa=pa, pb=pb, obs=obs,
                tf=np.linspace(3.0, 9.0, B))


def make_context(capi, torch, inp, deg_elev=0):
    from optimalbeziertrajectorygeneration_amd import synth
    ctx = capi.Context(inp["N"], 2, inp["n"], deg_elev, point_obs=inp["obs"])
    if inp["M"]:
        ctx.set_polygons(*synth.pack_polys(inp["polys"]))
    ctx.set_hull_pairs(inp["pa"], inp["pb"])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


class Buffers:
    """Device outputs of one call, filled with values no kernel writes."""
    def __init__(self, torch, ctx, B, n_hull, L):
        dev = "cuda"
        self.torch = torch
        self.sep = torch.full((B, ctx.num_pairs * L), np.nan, dtype=torch.float64, device=dev)
        self.speed = torch.full((B, ctx.len_speed), np.nan, dtype=torch.float64, device=dev)
        self.ang = torch.full((B, ctx.len_ang_rate), np.nan, dtype=torch.float64, device=dev)
        self.flag = torch.full((B, n_hull), -7, dtype=torch.int32, device=dev)
        self.c1 = torch.full((B, n_hull, 3), -1.0, dtype=torch.float64, device=dev)
        self.c2 = torch.full((B, n_hull, 3), -1.0, dtype=torch.float64, device=dev)
        self.dist = torch.full((B, n_hull), -1.0, dtype=torch.float64, device=dev)
        self.n_support = torch.full((B, n_hull), -7, dtype=torch.int32, device=dev)
        self.status = torch.full((B, n_hull), -7, dtype=torch.int32, device=dev)

    def gjk_ptrs(self):
        return [t.data_ptr() for t in (self.flag, self.c1, self.c2, self.dist, self.n_support, self.status)]

    def host(self, keys):
        self.torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in keys}


def run_calls(capi, torch, inp, deg_elev=0, max_iter=128, md_cap=256, calls=None, ctx=None):
    """Every call of the test on one shape, each made TWICE on fresh buffers (the second launch orders its pairs by the
    trip counts the first left behind).  -> ({"call/array": ndarray} with the second launch's under "call#2/array",
    {"call": launches per kernel name}, {"plain" / "pair" / "all": ctx.sweep_shape})."""
    own = ctx is None
    if own:
        ctx = make_context(capi, torch, inp, deg_elev)
    B, n_hull, L = inp["B"], len(inp["pa"]), 2 * inp["n"] + deg_elev + 1
    dYb, dYfd, dY0 = (torch.from_numpy(np.ascontiguousarray(inp[k])).cuda() for k in ("Yb", "Yfd", "Y"))
    dtf = torch.from_numpy(inp["tf"]).cuda()
    plain_only = inp["name"] in PLAIN_ONLY
    names = ["gjk_swarm", "gjk_swarm_dedup"] if plain_only else ["gjk_swarm", "pair_sweep", "constraint_sweep", "pair_sweep_fd_batch",
                                                                  "pair_sweep_fd_view", "gjk_swarm_dedup"]
    out, launches = {}, {}
    shapes = {"plain": ctx.sweep_shape(B, which=0)}
    if not plain_only:
        shapes["pair"] = ctx.sweep_shape(B, which=1)
        shapes["all"] = ctx.sweep_shape(B, which=1, want_dyn=True)
    for name in (calls or names):
        for rnd in ("", "#2"):
            b = Buffers(torch, ctx, B, n_hull, L)
            ctx.reset_kernel_stats()
            ctx.set_profiling(True)
            keys = GJK_KEYS
            if name == "gjk_swarm":
                ctx.gjk_swarm_dev(dYb.data_ptr(), B, *b.gjk_ptrs(), max_iter, md_cap)
            elif name == "gjk_swarm_dedup":
                ctx.set_fd_dedup(True)
                if not rnd:
                    shapes["dedup"] = ctx.sweep_shape(B, which=0)
                ctx.gjk_swarm_dev(dYb.data_ptr(), B, *b.gjk_ptrs(), max_iter, md_cap)
                ctx.set_fd_dedup(False)
            elif name == "pair_sweep":
                keys = ("sep",) + GJK_KEYS
                ctx.pair_sweep_dev(dYb.data_ptr(), B, MAX_SEP, b.sep.data_ptr(), *b.gjk_ptrs(), max_iter, md_cap)
            elif name == "constraint_sweep":
                keys = ("sep", "speed", "ang") + GJK_KEYS
                ctx.constraint_sweep_dev(dYb.data_ptr(), dtf.data_ptr(), B, MAX_SEP, b.sep.data_ptr(), SPEED_BOUND, True, MAX_RATE,
                                         b.speed.data_ptr(), b.ang.data_ptr(), *b.gjk_ptrs(), max_iter, md_cap)
            elif name == "pair_sweep_fd_batch":      # the materialised batch the view below stands for
                keys = ("sep",) + GJK_KEYS
                ctx.pair_sweep_dev(dYfd.data_ptr(), B, MAX_SEP, b.sep.data_ptr(), *b.gjk_ptrs(), max_iter, md_cap)
            elif name == "pair_sweep_fd_view":
                keys = ("sep",) + GJK_KEYS
                ctx.pair_sweep_fd_dev(dY0.data_ptr(), 1, FD_H, B, MAX_SEP, b.sep.data_ptr(), *b.gjk_ptrs(), max_iter, md_cap)
            else:
                raise ValueError(name)
            for k, v in b.host(keys).items():
                out["%s%s/%s" % (name, rnd, k)] = v
            launches[name + rnd] = {k: v[1] for k, v in ctx.kernel_stats().items() if v[1]}
            ctx.set_profiling(False)
    if own:
        ctx.use_own_stream()
        ctx.close()
    return out, launches, shapes


def main(argv):
    import json
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi as capi
    path, args = argv[0], argv[1:]
    deg_elev = 0
    if args and args[0] == "--elev":
        deg_elev, args = int(args[1]), args[2:]
    arrays, meta = {}, {}
    for name in (args or list(SHAPES)):
        out, launches, shapes = run_calls(capi, torch, inputs(name), deg_elev)
        for k, v in out.items():
            arrays[name + "/" + k] = v
        meta[name] = dict(launches=launches, shapes=shapes)
    meta["env"] = {k: v for k, v in os.environ.items() if k.startswith("OBTG_")}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez(path, **arrays)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
