#!/usr/bin/env python3
"""    python tools/mixed_degree_time.py [out.json]      (default: profiles/mixed_degree_min_dist.json; needs the MI355X)

64 degree-5 vehicles + 32 degree-10 curve obstacles: one evaluation (4560 pairs) and the one-call Jacobian list through
obtg_min_dist_mixed, beside the same scene with the vehicles elevated to degree 10 through obtg_min_dist (other hulls, other
answers: a yardstick for the time only).  Kernel times from the library's timer (OBTG_K_MIN_DIST)."""
import json, os, platform, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optimalbeziertrajectorygeneration_amd import _capi, synth
from optimalbeziertrajectorygeneration_amd.optimization import _spatial_jac_plan

N, M, nv, no = 64, 32, 5, 10
ctx = _capi.scratch_context()
Y = synth.swarm_control_points(N, 2, nv, seed=1234)
obs = np.zeros((M, 3, no + 1)); obs[:, :2] = synth.curve_obstacles(M, 2, no, seed=1234).reshape(M, 2, no + 1)
Yup = ctx.bern_elev(Y, no - nv)
kw = dict(eps=1e-9, max_depth=128, max_nodes=2000)

def scene(Yv):
    K = Yv.shape[1]
    veh = np.zeros((N, 3, K)); veh[:, :2] = Yv.reshape(N, 2, K)
    pa, pb = synth.all_pairs(N + M)
    plan = _spatial_jac_plan(synth.fd_batch(Yv), N, 2, list(obs))
    return (list(veh) + list(obs) if K != no + 1 else np.concatenate((veh, obs))), pa, pb, plan[0], plan[1], plan[2]

def timed(f, reps):
    ctx.set_profiling(True, only="min_dist")
    r = f(); r = f()
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    wall = 1e3 * (time.perf_counter() - t0) / reps
    kms, cnt = ctx.kernel_stats()["min_dist"]
    ctx.set_profiling(False)
    nodes = int(r["nodes"].sum())
    return dict(pairs=int(len(r["status"])), kernel_ms=round(kms / cnt, 4), wall_ms=round(wall, 3), nodes=nodes,
                ns_per_node=round(1e6 * kms / cnt / nodes, 3), status_counts=np.bincount(r["status"], minlength=4).tolist())

out = {"scene": "64 degree-5 vehicles (synth.swarm_control_points seed 1234) + 32 degree-10 curve obstacles (synth.curve_obstacles), 2-D; eps 1e-9, max_depth 128, max_nodes 2000",
       "timer": "OBTG_K_MIN_DIST (hipEvent pair around the launch), mean over the timed calls after two warm calls (the second with the pair order from the first call's node counts)"}
c, pa, pb, jc, jpa, jpb = scene(Y)
assert isinstance(c, list) and isinstance(jc, list)
out["mixed_degree_5_vs_10"] = {"one_evaluation": timed(lambda: ctx.min_dist_mixed(c, pa, pb, **kw), 10),
                               "jacobian_list": timed(lambda: ctx.min_dist_mixed(jc, jpa, jpb, **kw), 3)}
c, pa, pb, jc, jpa, jpb = scene(Yup)
assert isinstance(c, np.ndarray) and isinstance(jc, np.ndarray)
out["vehicles_elevated_to_degree_10_obtg_min_dist"] = {"one_evaluation": timed(lambda: ctx.min_dist(c, pa, pb, **kw), 10),
                                                       "jacobian_list": timed(lambda: ctx.min_dist(jc, jpa, jpb, **kw), 3)}
# the same elevated call on the equal-degree WAVE form (OBTG_MD_FORM is read per call): the form k_min_dist_mixed generalises
os.environ["OBTG_MD_FORM"] = "wave"
out["vehicles_elevated_to_degree_10_wave_form"] = {"one_evaluation": timed(lambda: ctx.min_dist(c, pa, pb, **kw), 10),
                                                   "jacobian_list": timed(lambda: ctx.min_dist(jc, jpa, jpb, **kw), 3)}
del os.environ["OBTG_MD_FORM"]
try:
    import torch
    pr = torch.cuda.get_device_properties(0)
    dev = {"name": pr.name, "arch": getattr(pr, "gcnArchName", "?"), "compute_units": pr.multi_processor_count,
           "memory_GiB": round(pr.total_memory / 2.0 ** 30, 1), "hip": torch.version.hip}
except Exception as e:
    dev = "unknown (%s)" % e
out["box"] = {"device": dev, "host": platform.machine(), "python": platform.python_version(),
              "library_source_hash": _capi.source_hash()}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mixed_degree_min_dist.json")
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
