#!/usr/bin/env python3
"""Generate the golden fixtures in tests/golden/*.npz by RUNNING THE REFERENCE.

This script is the only place that imports /root/reference (read-only).  It
exists in this container only; on the GPU box the reference is absent and the
script exits cleanly.  Nothing of the reference is copied: the fixtures hold
inputs (ours, seeded) and the outputs the reference's functions returned.

How the reference is made importable:
  * `numba` is not installed -> tests/golden/_numba_shim provides identity
    decorators (all reference uses are cache=True only);
  * MPLBACKEND=Agg;
  * two harness-side injections for the GJK-backed methods, because at HEAD
    bezier.py never imports gjkNew (bezier.py:21-22 commented out) and
    `_minDist` builds `Bezier([x, y, z])` from a list (bezier.py:1304) which the
    constructor rejects (bezier.py:58): `bez.gjkNew = gjk.gjkNew` and a Bezier
    subclass that coerces list input with the same np.array(..., ndmin=2,
    dtype=float) the reference's own cpts setter uses (bezier.py:92).
  * every gjkNew/_minDist call runs under a setitimer alarm and a
    RecursionError guard; non-terminating inputs are recorded as such.

Usage:  python tests/golden/gen_golden.py            (writes tests/golden/*.npz)
"""
import os
import signal
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

if not os.path.isdir(REF):
    print("reference absent (%s): nothing to do" % REF)
    sys.exit(0)

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_numba_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "Examples"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

import bezier as bez  # noqa: E402  (reference)
import optimization as opt  # noqa: E402  (reference)
from gjk import gjk as G  # noqa: E402  (reference)

from optimalbeziertrajectorygeneration_amd import synth  # noqa: E402  (ours)

# ---------------------------------------------------------------- injections
bez.gjkNew = G.gjkNew
_OrigBezier = bez.Bezier


class _PB(_OrigBezier):
    def __init__(self, cpts=None, t0=0.0, tf=1.0, tau=None):
        if cpts is not None and not isinstance(cpts, np.ndarray):
            cpts = np.array(cpts, ndmin=2, dtype=float)
        super().__init__(cpts=cpts, t0=t0, tf=tf, tau=tau)


bez.Bezier = _PB


class _Timeout(Exception):
    pass


def _alarm(signum, frame):
    raise _Timeout()


signal.signal(signal.SIGALRM, _alarm)


def guarded(fn, budget, *a, **k):
    """-> (status, value); status 0 ok, 1 timeout, 2 RecursionError."""
    signal.setitimer(signal.ITIMER_REAL, budget)
    try:
        v = fn(*a, **k)
        return 0, v
    except _Timeout:
        return 1, None
    except RecursionError:
        return 2, None
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


# -------------------------------------------------------- support-index trace
_trace = []
_orig_supportPts = G.supportPts
_cur_polys = [None, None]


def _first_row(poly, pt):
    idx = np.where((poly == pt).all(axis=1))[0]
    return int(idx[0])


def _traced_supportPts(poly1, poly2, direction):
    newPt, (p1, p2) = _orig_supportPts(poly1, poly2, direction)
    _trace.append((_first_row(poly1, p1), _first_row(poly2, p2)))
    return newPt, (p1, p2)


G.supportPts = _traced_supportPts
_gjk_calls = [0]
_orig_gjkNew = G.gjkNew


def _counted_gjkNew(*a, **k):
    _gjk_calls[0] += 1
    return _orig_gjkNew(*a, **k)


bez.gjkNew = _counted_gjkNew


def run_gjk(p1, p2, budget=0.5):
    """-> dict(status, flag, c1, c2, dist, trace)."""
    del _trace[:]
    import io
    import contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        st, v = guarded(_orig_gjkNew, budget, p1, p2)
    tr = np.array(_trace, dtype=np.int16).reshape(-1, 2)
    out = dict(status=st, flag=-9, c1=np.full(3, np.nan), c2=np.full(3, np.nan),
               dist=np.nan, trace=tr)
    if st == 0:
        flag, info = v
        out["flag"] = int(flag)
        if flag == 1:
            out["c1"] = np.asarray(info[0], dtype=float)
            out["c2"] = np.asarray(info[1], dtype=float)
            out["dist"] = float(info[2])
    return out


def gjk_group(polys, pair_a, pair_b, budget=0.5):
    pts, off = synth.pack_polys(polys)
    n = len(pair_a)
    flag = np.zeros(n, np.int32)
    status = np.zeros(n, np.int32)
    c1 = np.zeros((n, 3))
    c2 = np.zeros((n, 3))
    dist = np.zeros(n)
    tr_off = np.zeros(n + 1, np.int32)
    traces = []
    for k in range(n):
        r = run_gjk(polys[pair_a[k]], polys[pair_b[k]], budget)
        flag[k], status[k] = r["flag"], r["status"]
        c1[k], c2[k], dist[k] = r["c1"], r["c2"], r["dist"]
        traces.append(r["trace"])
        tr_off[k + 1] = tr_off[k] + len(r["trace"])
    trace = np.concatenate(traces) if traces else np.zeros((0, 2), np.int16)
    return dict(pts=pts, off=off, pair_a=np.asarray(pair_a, np.int32),
                pair_b=np.asarray(pair_b, np.int32), flag=flag, status=status,
                c1=c1, c2=c2, dist=dist, trace=trace.astype(np.int16), trace_off=tr_off)


def save(name, **arrs):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrs)
    print("wrote %-28s %8.1f KB" % (name, os.path.getsize(path) / 1024.0))


# ==================================================================== tables
def gen_tables():
    d = {}
    for (n, R) in [(10, 0), (10, 10), (20, 0), (20, 30), (20, 100), (10, 1), (30, 0),
                   (40, 100), (5, 1), (15, 1), (2, 3)]:
        d["elev_%d_%d" % (n, R)] = bez.elevMatrix(n, R)
    for n in [3, 5, 10, 15, 20]:
        d["prod_%d" % n] = bez.bezProductCoefficients(n, n)
        d["prodT_%d" % n] = bez.prodMatrix(n)
    for n in [5, 10, 15]:
        for T in [1.0, 2.4276, 10.0]:
            d["diff_%d_%s" % (n, repr(T))] = bez.diffMatrix(n, T)
    save("tables.npz", **d)


# =============================================================== Bezier ops
def gen_ops():
    rng = np.random.default_rng(42)
    d = {}
    case = 0
    for dim in (1, 2, 3):
        for n in (5, 10, 15):
            a = rng.normal(0, 3, size=(dim, n + 1))
            b = rng.normal(0, 3, size=(dim, n + 1))
            tf = float(rng.uniform(0.5, 12.0))
            A = bez.Bezier(a.copy(), tf=tf)
            Bc = bez.Bezier(b.copy(), tf=tf)
            pre = "c%d_" % case
            d[pre + "a"], d[pre + "b"], d[pre + "tf"] = a, b, np.array(tf)
            d[pre + "elev1"] = A.elev(1).cpts
            d[pre + "elev7"] = A.elev(7).cpts
            d[pre + "elev0"] = A.elev(0).cpts
            Ad = A.diff()
            d[pre + "diff"] = np.asarray(Ad.cpts)
            d[pre + "diff_tf"] = np.array(Ad.tf)
            d[pre + "diff2"] = np.asarray(Ad.diff().cpts)
            d[pre + "normsq"] = np.asarray(A.normSquare().cpts)
            d[pre + "mul"] = np.asarray((A * Bc).cpts)
            d[pre + "sub"] = np.asarray((A - Bc).cpts)
            d[pre + "add"] = np.asarray((A + Bc).cpts)
            for q, frac in enumerate((0.3, 0.5, 0.875)):       # Bezier.split (bezier.py:533-572)
                c1, c2 = A.split(frac * tf)
                d[pre + "split%d_t" % q] = np.array(frac * tf)
                d[pre + "split%d_l" % q], d[pre + "split%d_r" % q] = np.asarray(c1.cpts), np.asarray(c2.cpts)
                d[pre + "split%d_span" % q] = np.array([c1.t0, c1.tf, c2.t0, c2.tf])
            # Bezier.__call__ and Bezier.curve (bezier.py:184-199, 233-258; deCasteljauCurve): a few samples incl. the ends
            ts = np.array([0.0, 0.125 * tf, 0.5 * tf, 0.77 * tf, tf])
            d[pre + "call_t"], d[pre + "call_v"] = ts, A(ts)
            d[pre + "curve_head"], d[pre + "curve_tail"] = A.curve[:, :3].copy(), A.curve[:, -3:].copy()
            case += 1
    d["n_cases"] = np.array(case)
    save("bezier_ops.npz", **d)


# ============================================================ problem layer
def example1_bezopt():
    numVeh = 2
    return opt.BezOptimization(numVeh=numVeh, dimension=2, degree=10, minimizeGoal='TimeOpt',
                               maxSep=1, maxSpeed=5, maxAngRate=1,
                               initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)],
                               initSpeeds=[1] * numVeh, finalSpeeds=[1] * numVeh,
                               initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2],
                               pointObstacles=[[3, 2], [6, 7]])


def gen_problem():
    d = {}
    rng = np.random.default_rng(7)
    # --- Example1 (time-optimal, speeds+angles, 2 point obstacles)
    bo = example1_bezopt()
    xg = bo.generateGuess(std=0)
    d["ex1_xguess"] = xg
    d["ex1_yguess"] = bo.reshapeVector(xg)
    xr = xg + rng.normal(0, 0.3, size=xg.shape)
    xr[-1] = 3.7
    d["ex1_x"] = xr
    d["ex1_y"] = bo.reshapeVector(xr)
    xg2 = bo.generateGuess(std=0.5, seed=3)
    d["ex1_xguess_std"] = xg2
    for R in (0, 30, 100):
        opt.DEG_ELEV = R
        for tag, x in (("g", xg), ("r", xr)):
            d["ex1_%s_tsep_class_R%d" % (tag, R)] = bo.temporalSeparationConstraints(x)
            d["ex1_%s_tsep_example_R%d" % (tag, R)] = opt._temporalSeparationConstraints(
                bo.reshapeVector(x), 2, 2, 1)
            d["ex1_%s_maxspeed_R%d" % (tag, R)] = bo.maxSpeedConstraints(x)
            d["ex1_%s_minspeed_R%d" % (tag, R)] = bo.minSpeedConstraints(x)
            if R <= 30:
                d["ex1_%s_angrate_R%d" % (tag, R)] = bo.maxAngularRateConstraints(x)
    opt.DEG_ELEV = 0
    d["ex1_obj"] = np.array(bo.objectiveFunction(xr))

    # --- Swarm example as written (36 vehicles, 3-D, degree 5, Euclidean)
    import SwarmOfAerialVehicles as SW
    numVeh, initPts, finalPts = SW.generatePointsFromImage(SW.CAS_IMG)
    bs = opt.BezOptimization(numVeh=numVeh, dimension=3, degree=5, minimizeGoal='Euclidean',
                             maxSep=0.9, initPoints=initPts, finalPoints=finalPts)
    xs = SW.generate3DGuess(initPts, finalPts, 5)
    d["sw_init"], d["sw_final"] = initPts, finalPts
    d["sw_xguess"] = xs
    d["sw_yguess"] = bs.reshapeVector(xs)
    xsr = xs + rng.normal(0, 0.2, size=xs.shape)
    d["sw_x"] = xsr
    d["sw_y"] = bs.reshapeVector(xsr)
    d["sw_g_tsep"] = bs.temporalSeparationConstraints(xs)
    d["sw_r_tsep"] = bs.temporalSeparationConstraints(xsr)
    d["sw_r_obj"] = np.array(bs.objectiveFunction(xsr))
    d["sw_genguess"] = bs.generateGuess(std=0)

    # --- fixed-tf model with speeds (not time-optimal), 3 vehicles
    bf = opt.BezOptimization(numVeh=3, dimension=2, degree=7, minimizeGoal='Euclidean',
                             maxSep=0.5, maxSpeed=4, minSpeed=0.2, maxAngRate=2,
                             initPoints=[(0, 0), (1, 5), (9, 2)], finalPoints=[(10, 1), (8, 8), (0, 7)],
                             initSpeeds=[1, 2, 0.5], finalSpeeds=[1, 1, 2],
                             initAngs=[0.1, -0.4, 2.0], finalAngs=[0.3, 0.0, 2.5], tf=7.0)
    xf = bf.generateGuess(std=0.4, seed=11)
    d["fx_x"] = xf
    d["fx_y"] = bf.reshapeVector(xf)
    d["fx_tsep"] = bf.temporalSeparationConstraints(xf)
    d["fx_maxspeed"] = bf.maxSpeedConstraints(xf)
    d["fx_minspeed"] = bf.minSpeedConstraints(xf)
    d["fx_angrate"] = bf.maxAngularRateConstraints(xf)
    d["fx_obj"] = np.array(bf.objectiveFunction(xf))
    bfa = opt.BezOptimization(numVeh=3, dimension=2, degree=7, minimizeGoal='Accel',
                              initPoints=[(0, 0), (1, 5), (9, 2)], finalPoints=[(10, 1), (8, 8), (0, 7)],
                              initSpeeds=[1, 2, 0.5], finalSpeeds=[1, 1, 2],
                              initAngs=[0.1, -0.4, 2.0], finalAngs=[0.3, 0.0, 2.5], tf=7.0)
    d["fx_obj_accel"] = np.array(bfa.objectiveFunction(xf))
    bfa.model['minGoal'] = 'Jerk'
    d["fx_obj_jerk"] = np.array(bfa.objectiveFunction(xf))
    # literal layout check of optimization.py:614-654 (2 vehicles, speeds, deg 5)
    bm = opt.BezOptimization(numVeh=2, dimension=2, degree=5,
                             initPoints=np.array([[1, 2], [3, 4]]), finalPoints=np.array([[5, 6], [7, 8]]),
                             initSpeeds=np.array([3, 3]), finalSpeeds=np.array([10, 10]),
                             initAngs=np.array([np.pi / 2, np.pi / 2]), finalAngs=np.array([0, 0]),
                             pointObstacles=[[1, 2], [3, 4]])
    xm = np.arange(8.0) + 0.5
    d["main_x"] = xm
    d["main_y"] = bm.reshapeVector(xm)
    d["main_guess"] = bm.generateGuess()
    save("problem.npz", **d)


def ref_constraints(Y, N, dim, tf, maxSep, vmax, vmin, wmax, R, ang=True):
    opt.DEG_ELEV = R
    out = dict(tsep=opt._temporalSeparationConstraints(Y, N, dim, maxSep),
               maxspeed=opt._maxSpeedConstraints(Y, N, dim, tf, vmax),
               minspeed=opt._minSpeedConstraints(Y, N, dim, tf, vmin))
    if ang and dim == 2:
        with np.errstate(all="ignore"):
            out["angrate"] = opt._maxAngularRateConstraints(Y, N, dim, tf, wmax)
    opt.DEG_ELEV = 0
    return out


def gen_constraints():
    d = {}
    cases = [
        # name, N, d, n, R, tf, seed
        ("c2", 8, 3, 10, 0, 10.0, 1234),
        ("c2file_syn", 36, 3, 5, 0, 1.0, 1234),
        ("c3", 64, 2, 10, 0, 10.0, 1234),
        ("c3s_R10", 8, 2, 10, 10, 10.0, 1234),
        ("c3s_R100", 8, 2, 10, 100, 10.0, 1234),
        ("c4s", 12, 2, 15, 0, 10.0, 1234),
        ("c4s_R3", 6, 2, 15, 3, 2.5, 99),
        ("d1", 5, 1, 6, 2, 3.0, 5),
        ("n20", 4, 2, 20, 5, 4.0, 6),
        ("n3", 7, 3, 3, 0, 4.0, 8),
        # degree 8 (9 control points: Examples/DubinsCarTimeOptimal.py:72, DubinsCarExample2.py:83), specialised since round 5
        ("d8", 10, 2, 8, 0, 6.0, 31),
        ("d8_R7", 6, 2, 8, 7, 3.5, 32),
        ("d8_3d", 5, 3, 8, 0, 2.0, 33),
    ]
    names = []
    for (name, N, dim, n, R, tf, seed) in cases:
        Y = synth.swarm_control_points(N, dim, n, seed=seed)
        r = ref_constraints(Y, N, dim, tf, 0.9, 5.0, 0.3, 1.0, R)
        d[name + "_Y"] = Y
        d[name + "_par"] = np.array([N, dim, n, R, tf, 0.9, 5.0, 0.3, 1.0])
        for k, v in r.items():
            d[name + "_" + k] = v
        names.append(name)
    # inf/nan case: one stationary vehicle (all control points equal) and one
    # straight constant-speed line -> exact zeros in numerator/denominator
    Y = synth.swarm_control_points(4, 2, 6, seed=21)
    Y[0, :] = 3.0
    Y[1, :] = -2.0
    Y[2] = np.linspace(0, 6, 7)
    Y[3] = np.linspace(1, 4, 7)
    r = ref_constraints(Y, 4, 2, 2.0, 0.9, 5.0, 0.3, 1.0, 0)
    d["nan_Y"] = Y
    d["nan_par"] = np.array([4, 2, 6, 0, 2.0, 0.9, 5.0, 0.3, 1.0])
    for k, v in r.items():
        d["nan_" + k] = v
    names.append("nan")
    d["names"] = np.array(names)
    save("constraints.npz", **d)


# ======================================================================= GJK
def literal_polys():
    """Literal test inputs used by the reference's own demos (inputs only):
    gjk/gjk.py:690-745 (poly1..8), gjk/gjkTests.py:23-46, bezier.py:1794-1804."""
    P = []
    P.append([(4, 11, 0), (4, 5, 0), (9, 9, 0)])
    P.append([(5, 6, 0), (10, 2, 0), (13, 1, 0), (12, 3, 0), (15, 6, 0)])
    P.append([(4, 11, -1), (4, 5, -1), (9, 9, -1), (7, 8, 3)])
    P.append([(4, 11, 3), (4, 5, 3), (9, 9, 3), (7, 8, -1)])
    P.append([(4, 11, -3), (4, 5, -3), (9, 9, -3), (7, 8, -1)])
    P.append([(4, 11, 0), (4, 5, 1), (9, 9, 2), (7, 8, 3)])
    P.append([(-1, -1, 0), (1, 1, 0), (1, -1, 0), (-1, 1, 0)])
    P.append([(-1, -1, -3), (1, 1, -3), (1, -1, -3), (-1, 1, -3), (0, 0, -1)])
    # dyn4j article pair (gjk/gjkTests.py:23-34)
    P.append([(4, 11, 0), (4, 5, 0), (9, 9, 0)])
    P.append([(8, 6, 0), (10, 2, 0), (13, 1, 0), (15, 6, 0)])
    # 3-D triangle pair (gjk/gjkTests.py:36-46)
    P.append([(1, 0, -2), (0, 4, -3), (0, 0, 0)])
    P.append([(3, 8, 1), (5, -4, 1), (0.2, 0, 5)])
    return [np.array(p, dtype=float) for p in P]


def gen_gjk():
    d = {}
    polys = literal_polys()
    n = len(polys)
    pa, pb = [], []
    for i in range(n):
        for j in range(n):
            if i != j:
                pa.append(i)
                pb.append(j)
    g = gjk_group(polys, pa, pb)
    for k, v in g.items():
        d["lit_" + k] = v
    print("  literal: %d pairs, flags %s, timeouts %d" % (
        len(pa), np.bincount(g["flag"][g["status"] == 0] + 1, minlength=3), (g["status"] != 0).sum()))

    # C3 2-D swarm: 64 vehicles (degree-10 hulls) + 8 polygons
    Y = synth.swarm_control_points(64, 2, 10, seed=1234)
    polys = synth.hulls_from_Y(Y, 2) + synth.polygon_obstacles(8, seed=1234)
    pa, pb = synth.swarm_pairs(64, 8)
    g = gjk_group(polys, pa, pb)
    for k, v in g.items():
        d["c3_" + k] = v
    ok = g["status"] == 0
    print("  c3 2-D: %d pairs, flags(-1,0,1) %s, timeouts %d, mean supports %.2f" % (
        len(pa), np.bincount(g["flag"][ok] + 1, minlength=3), (~ok).sum(),
        np.diff(g["trace_off"])[ok].mean()))

    # a denser 2-D swarm in a smaller box so that more pairs collide / touch
    rng = np.random.default_rng(77)
    Yd = synth.swarm_control_points(24, 2, 6, seed=77)
    Yd *= 0.25
    polys = synth.hulls_from_Y(Yd, 2)
    pa, pb = synth.swarm_pairs(24, 0)
    g = gjk_group(polys, pa, pb)
    for k, v in g.items():
        d["dense_" + k] = v
    ok = g["status"] == 0
    print("  dense 2-D: %d pairs, flags %s, timeouts %d" % (
        len(pa), np.bincount(g["flag"][ok] + 1, minlength=3), (~ok).sum()))

    # 3-D swarm: 64 vehicles degree 10 (terminating subset + non-terminating ids)
    Y3 = synth.swarm_control_points(64, 3, 10, seed=1234)
    polys = synth.hulls_from_Y(Y3, 3)
    pa, pb = synth.swarm_pairs(64, 0)
    g = gjk_group(polys, pa, pb, budget=0.4)
    for k, v in g.items():
        d["s3d_" + k] = v
    ok = g["status"] == 0
    print("  3-D: %d pairs, flags %s, timeouts %d, mean supports %.2f" % (
        len(pa), np.bincount(g["flag"][ok] + 1, minlength=3), (~ok).sum(),
        np.diff(g["trace_off"])[ok].mean()))
    save("gjk.npz", **d)


# ==================================================================== minDist
def run_mindist(c1, c2, budget=5.0):
    _gjk_calls[0] = 0
    import io
    import contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        st, v = guarded(bez._minDist, budget, c1, c2)
    calls = _gjk_calls[0]
    if st == 0:
        return st, np.array([float(v[0]), float(v[1]), float(v[2])]), calls
    return st, np.full(3, np.nan), calls


def run_mindist2poly(c1, poly, budget=5.0):
    _gjk_calls[0] = 0
    import io
    import contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        st, v = guarded(bez._minDist2Poly, budget, c1, poly)
    calls = _gjk_calls[0]
    if st == 0:
        pt = np.asarray(v[2], dtype=float)
        if pt.ndim == 0:
            pt = np.full(3, float(pt))
        return st, np.array([float(v[0]), float(v[1])]), pt, calls
    return st, np.full(2, np.nan), np.full(3, np.nan), calls


def gen_mindist():
    d = {}
    sys.setrecursionlimit(1000)
    # literal curves of bezier.py:1774-1804 (inputs only)
    cpts1 = np.array([(0, 1, 2, 3, 4, 5), (1, 2, 0, 0, 2, 1), (0, 1, 2, 3, 4, 5)], dtype=float)
    cpts2 = np.array([(0, 1, 2, 3, 4, 5), (3, 2, 0, 0, 2, 3), (5, 4, 3, 2, 1, 0)], dtype=float)
    cpts3 = np.array([(0, 1, 2, 3, 4, 5), (0, 1, 2, 3, 4, 5), (0, 0, 0, 0, 0, 0)], dtype=float)
    cpts4 = np.array([(5, 4, 3, 2, 1, 0), (0, 1, 2, 3, 4, 5), (0, 0, 0, 0, 0, 0)], dtype=float)
    cpts4[1, :] -= 1
    cpts5 = cpts1 + 3
    poly1 = np.array([(1, 1, 3), (1, 1, 2), (1, 2, 1), (3, 1, 3), (1, 3, 1)], dtype=float)
    poly2 = np.array([(1, 1, 3), (1, 1, 2), (1, 2, 1), (3, -1, 3), (1, 3, 1)], dtype=float)
    curves = [cpts1, cpts2, cpts3, cpts4, cpts5]
    d["lit_curves"] = np.stack(curves)
    res, stat, calls, pairs = [], [], [], []
    for i in range(5):
        for j in range(5):
            if i == j:
                continue
            st, v, nc = run_mindist(bez.Bezier(curves[i].copy()), bez.Bezier(curves[j].copy()))
            res.append(v); stat.append(st); calls.append(nc); pairs.append((i, j))
    d["lit_pairs"] = np.array(pairs, np.int32)
    d["lit_res"] = np.array(res)
    d["lit_status"] = np.array(stat, np.int32)
    d["lit_calls"] = np.array(calls, np.int32)
    print("  literal curve pairs: status", np.bincount(stat, minlength=3), "calls max", max(calls))
    # curve vs polygon
    d["lit_polys"] = np.stack([poly1, poly2])
    r2, p2, s2, c2, pr2 = [], [], [], [], []
    for i in range(5):
        for k, poly in enumerate((poly1, poly2)):
            st, v, pt, nc = run_mindist2poly(bez.Bezier(curves[i].copy()), poly.copy())
            r2.append(v); p2.append(pt); s2.append(st); c2.append(nc); pr2.append((i, k))
    d["litp_pairs"] = np.array(pr2, np.int32)
    d["litp_res"] = np.array(r2)
    d["litp_pt"] = np.array(p2)
    d["litp_status"] = np.array(s2, np.int32)
    d["litp_calls"] = np.array(c2, np.int32)
    print("  literal curve/poly: status", np.bincount(s2, minlength=3), "calls max", max(c2))

    # seeded C3 pairs: first 60 pairs of a stride through the 2016 list
    Y = synth.swarm_control_points(64, 2, 10, seed=1234)
    pa, pb = synth.swarm_pairs(64, 0)
    sel = np.arange(0, len(pa), len(pa) // 60)[:60]
    res, stat, calls = [], [], []
    for k in sel:
        i, j = int(pa[k]), int(pb[k])
        st, v, nc = run_mindist(bez.Bezier(Y[2 * i:2 * i + 2].copy()), bez.Bezier(Y[2 * j:2 * j + 2].copy()),
                                budget=4.0)
        res.append(v); stat.append(st); calls.append(nc)
    d["c3_Y"] = Y
    d["c3_sel"] = sel.astype(np.int32)
    d["c3_pa"], d["c3_pb"] = pa[sel], pb[sel]
    d["c3_res"] = np.array(res)
    d["c3_status"] = np.array(stat, np.int32)
    d["c3_calls"] = np.array(calls, np.int32)
    print("  c3 curve pairs: status", np.bincount(stat, minlength=3), "calls median",
          int(np.median(np.array(calls)[np.array(stat) == 0])), "max", max(calls))
    # vehicles vs polygons
    polys = synth.polygon_obstacles(8, seed=1234)
    r2, p2, s2, c2, pr2 = [], [], [], [], []
    for i in range(0, 64, 4):
        for k in range(8):
            st, v, pt, nc = run_mindist2poly(bez.Bezier(Y[2 * i:2 * i + 2].copy()), polys[k].copy(), budget=3.0)
            r2.append(v); p2.append(pt); s2.append(st); c2.append(nc); pr2.append((i, k))
    pts, off = synth.pack_polys(polys)
    d["c3p_pts"], d["c3p_off"] = pts, off
    d["c3p_pairs"] = np.array(pr2, np.int32)
    d["c3p_res"] = np.array(r2)
    d["c3p_pt"] = np.array(p2)
    d["c3p_status"] = np.array(s2, np.int32)
    d["c3p_calls"] = np.array(c2, np.int32)
    print("  c3 curve/poly: status", np.bincount(s2, minlength=3), "calls max", max(c2))
    save("mindist.npz", **d)


def gen_mindist_script():
    """The inputs of Examples/MinDistBez2Bez.py:42-84 (its five 3-D curves; cpts5 = cpts1 - 3 there, + 3 in bezier.py's
    own block above) through the reference's `_minDist` on every ordered pair, and `_minDist2Poly` on its three polygons."""
    d = {}
    sys.setrecursionlimit(1000)
    cpts1 = np.array([(0, 1, 2, 3, 4, 5), (1, 2, 0, 0, 2, 1), (0, 1, 2, 3, 4, 5)], dtype=float)
    cpts2 = np.array([(0, 1, 2, 3, 4, 5), (3, 2, 0, 0, 2, 3), (5, 4, 3, 2, 1, 0)], dtype=float)
    cpts3 = np.array([(0, 1, 2, 3, 4, 5), (0, 1, 2, 3, 4, 5), (0, 0, 0, 0, 0, 0)], dtype=float)
    cpts4 = np.array([(5, 4, 3, 2, 1, 0), (0, 1, 2, 3, 4, 5), (0, 0, 0, 0, 0, 0)], dtype=float)
    cpts4[1, :] -= 1
    cpts5 = cpts1 - 3
    polys = [np.array([(1, 3, 3), (1, 3, 2), (1, 4, 1), (3, 3, 3), (1, 5, 1)], dtype=float),
             np.array([(1, 1, 3), (1, 1, 2), (1, 2, 1), (4, 0, 2), (1, 3, 1)], dtype=float),
             np.array([(1, 1, 0), (1, 3, 0), (2, 5, 0), (4, 4, 0)], dtype=float)]
    curves = [cpts1, cpts2, cpts3, cpts4, cpts5]
    d["curves"] = np.stack(curves)
    res, stat, pairs = [], [], []
    for i in range(5):
        for j in range(5):
            if i == j:
                continue
            st, v, _ = run_mindist(bez.Bezier(curves[i].copy()), bez.Bezier(curves[j].copy()))
            res.append(v); stat.append(st); pairs.append((i, j))
    d["pairs"], d["res"], d["status"] = np.array(pairs, np.int32), np.array(res), np.array(stat, np.int32)
    print("  script curve pairs: status", np.bincount(stat, minlength=3))
    pts, off = synth.pack_polys(polys)
    d["poly_pts"], d["poly_off"] = pts, off
    r2, p2, s2, pr2 = [], [], [], []
    for i in range(5):
        for k, poly in enumerate(polys):
            st, v, pt, _ = run_mindist2poly(bez.Bezier(curves[i].copy()), poly.copy())
            r2.append(v); p2.append(pt); s2.append(st); pr2.append((i, k))
    d["p_pairs"], d["p_res"], d["p_pt"], d["p_status"] = np.array(pr2, np.int32), np.array(r2), np.array(p2), np.array(s2, np.int32)
    print("  script curve/poly: status", np.bincount(s2, minlength=3))
    save("mindist_script.npz", **d)


def _wide_poly(kv, planar, rng):
    """kv vertices on a small ellipse somewhere in the swarm's square, jittered; planar (z = 0) or a point set in space."""
    ang = np.sort(rng.uniform(0, 2 * np.pi, kv))
    c = rng.uniform(10, 90, 2)
    P = np.zeros((kv, 3))
    P[:, 0] = c[0] + 6 * np.cos(ang) + rng.normal(0, 0.3, kv)
    P[:, 1] = c[1] + 4 * np.sin(ang) + rng.normal(0, 0.3, kv)
    if not planar:
        P[:, 2] = rng.uniform(0, 30, kv)
    return P


def gen_mindist_wide():
    """`_minDist` and `_minDist2Poly` at the shapes the device runs in its wave and one-lane forms: curves of 17..32 control points
    (kMdMaxK = 32) and polygons of 20..64 vertices.  Per group `<g>_`: curves[n][3][K] (2-D ones with a zero z row), the pair
    list, and the reference's status, result, gjkNew-call count (and closest point).  Mostly separated swarm curves -- the
    reference takes seconds on crossing K = 32 pairs -- plus a few crossing pairs drawn in a small box, whose status (a timeout
    among them) is recorded as it is."""
    d = {}
    sys.setrecursionlimit(1000)
    md_groups, p_groups = [], []
    for K in (17, 21, 25, 32):
        for dim in (2, 3):
            g = "md_K%d_d%d" % (K, dim)
            nsw = 6
            Y = synth.swarm_control_points(nsw, dim, K - 1, seed=100 * K + dim)
            rng = np.random.default_rng(200 * K + dim)
            box = rng.uniform(0, 10, size=(2 * dim, K))          # two curves in a small box: they cross
            curves = np.zeros((nsw + 2, 3, K))
            curves[:nsw, :dim, :] = Y.reshape(nsw, dim, K)
            curves[nsw:, :dim, :] = box.reshape(2, dim, K)
            pa, pb = synth.all_pairs(nsw)
            sel = np.arange(0, len(pa), 2)                       # 8 of the 15 swarm pairs
            pairs = [(int(pa[k]), int(pb[k])) for k in sel] + [(nsw, nsw + 1), (0, nsw)]
            res, stat, calls = [], [], []
            for (i, j) in pairs:
                st, v, nc = run_mindist(bez.Bezier(curves[i, :dim].copy()), bez.Bezier(curves[j, :dim].copy()), budget=5.0)
                res.append(v); stat.append(st); calls.append(nc)
            d[g + "_curves"], d[g + "_pairs"] = curves, np.array(pairs, np.int32)
            d[g + "_res"], d[g + "_status"], d[g + "_calls"] = np.array(res), np.array(stat, np.int32), np.array(calls, np.int32)
            md_groups.append(g)
            print("  %s: status %s, calls max %d" % (g, np.bincount(stat, minlength=3), max(calls)))
    for K in (11, 21, 32):
        for dim in (2, 3):
            g = "p_K%d_d%d" % (K, dim)
            nc_ = 3
            Y = synth.swarm_control_points(nc_, dim, K - 1, seed=300 * K + dim)
            curves = np.zeros((nc_, 3, K))
            curves[:, :dim, :] = Y.reshape(nc_, dim, K)
            rng = np.random.default_rng(400 * K + dim)
            polys = [_wide_poly(kv, dim == 2, rng) for kv in (20, 32, 40, 64)]
            pts, off = synth.pack_polys(polys)
            pairs = [(i, q) for i in range(nc_) for q in range(len(polys))]
            res, pt, stat, calls = [], [], [], []
            for (i, q) in pairs:
                st, v, p, nc = run_mindist2poly(bez.Bezier(curves[i, :dim].copy()), polys[q].copy(), budget=5.0)
                res.append(v); pt.append(p); stat.append(st); calls.append(nc)
            d[g + "_curves"], d[g + "_pts"], d[g + "_off"], d[g + "_pairs"] = curves, pts, off, np.array(pairs, np.int32)
            d[g + "_res"], d[g + "_pt"] = np.array(res), np.array(pt)
            d[g + "_status"], d[g + "_calls"] = np.array(stat, np.int32), np.array(calls, np.int32)
            p_groups.append(g)
            print("  %s: status %s, calls max %d" % (g, np.bincount(stat, minlength=3), max(calls)))
    d["md_groups"], d["p_groups"] = np.array(md_groups), np.array(p_groups)
    save("mindist_wide.npz", **d)


# ========================================================================= C5
def gen_c5():
    """BASELINE config 5 (ComplexObstacles.py-style): 64 vehicles + 32 curve obstacles, degree 10.
    gjkNew over all C(96,2) = 4560 hull pairs of the seeded set, and `_minDist` on a strided subset
    of the same pair list (status, result, gjkNew-call count)."""
    d = {}
    N, M, n = 64, 32, 10
    Y = synth.swarm_control_points(N, 2, n, seed=1234)
    Yo = synth.curve_obstacles(M, 2, n, seed=1234)
    polys = synth.hulls_from_Y(Y, 2) + synth.hulls_from_Y(Yo, 2)
    pa, pb = synth.all_pairs(N + M)
    g = gjk_group(polys, pa, pb)
    for k, v in g.items():
        d["gjk_" + k] = v
    ok = g["status"] == 0
    print("  c5 hulls: %d pairs, flags(-1,0,1) %s, timeouts %d, mean supports %.2f" % (
        len(pa), np.bincount(g["flag"][ok] + 1, minlength=3), (~ok).sum(), np.diff(g["trace_off"])[ok].mean()))
    d["Y"], d["Yobs"] = Y, Yo
    sys.setrecursionlimit(1000)
    Yall = np.vstack((Y, Yo))
    sel = np.arange(0, len(pa), len(pa) // 60)[:60]
    res, stat, calls = [], [], []
    for k in sel:
        i, j = int(pa[k]), int(pb[k])
        st, v, nc = run_mindist(bez.Bezier(Yall[2 * i:2 * i + 2].copy()), bez.Bezier(Yall[2 * j:2 * j + 2].copy()),
                                budget=4.0)
        res.append(v); stat.append(st); calls.append(nc)
    d["md_sel"] = sel.astype(np.int32)
    d["md_pa"], d["md_pb"] = pa[sel], pb[sel]
    d["md_res"] = np.array(res)
    d["md_status"] = np.array(stat, np.int32)
    d["md_calls"] = np.array(calls, np.int32)
    print("  c5 curve pairs: status", np.bincount(stat, minlength=3), "calls median",
          int(np.median(np.array(calls)[np.array(stat) == 0])), "max", max(calls))
    save("c5.npz", **d)


# ==================================================== spatialSeparationConstraints
def spatial_problem(dim, deg, seed, nveh=2):
    """Inputs (ours, seeded) of one small spatial-separation problem: nveh vehicles + 1 curve obstacle."""
    rng = np.random.default_rng(seed)
    ip = rng.uniform(0, 10, size=(nveh, dim))
    fp = rng.uniform(0, 10, size=(nveh, dim))
    obs = rng.uniform(0, 10, size=(dim, deg + 1))
    return ip, fp, obs


def gen_spatial():
    """BezOptimization.spatialSeparationConstraints (optimization.py:109-133) on small problems the
    reference finishes: the assembled (P,3) array (maxSep subtracted from dist, t1 AND t2), pair order,
    and the total number of gjkNew calls."""
    import io
    import contextlib
    sys.setrecursionlimit(1000)
    d = {}
    names = []
    for (dim, deg, seed) in [(2, 5, 10), (2, 5, 11), (3, 5, 0), (3, 5, 2), (3, 5, 6), (3, 5, 9)]:
        ip, fp, obs = spatial_problem(dim, deg, seed)
        bo = opt.BezOptimization(numVeh=2, dimension=dim, degree=deg, minimizeGoal='Euclidean', maxSep=0.5,
                                 initPoints=ip, finalPoints=fp, shapeObstacles=[bez.Bezier(obs.copy())])
        x = bo.generateGuess(std=0.7, seed=seed)
        _gjk_calls[0] = 0
        with contextlib.redirect_stdout(io.StringIO()):
            st, v = guarded(bo.spatialSeparationConstraints, 60.0, x)
        if st != 0:
            print("  spatial (%d,%d,%d): reference did not finish (status %d), skipped" % (dim, deg, seed, st))
            continue
        name = "s%dd_%d" % (dim, seed)
        names.append(name)
        d[name + "_par"] = np.array([2, dim, deg, 0.5])
        d[name + "_init"], d[name + "_final"], d[name + "_obs"] = ip, fp, obs
        d[name + "_x"] = x
        d[name + "_y"] = bo.reshapeVector(x)
        d[name + "_out"] = np.asarray(v, dtype=float)
        d[name + "_calls"] = np.array(_gjk_calls[0])
        print("  spatial %s: out %s, %d gjkNew calls" % (name, np.asarray(v).shape, _gjk_calls[0]))
    d["names"] = np.array(names)
    save("spatial.npz", **d)


def gen_nearstop():
    """Angular rate with DEG_ELEV > 0 on vehicles that nearly stop (round 3).  A random-shape stress run of round 2
    (tools/stress_sweeps.py families, trial 28: 48 vehicles, degree 15, DEG_ELEV 100,
    synth.swarm_control_points(48, 2, 15, seed=528)) found one element 1.45e-8 (scale-aware) from the oracle in the
    default order of operations.  Its worst-conditioned vehicles -- the four whose elevated |v|^2 control points come
    closest to zero (some cross it) -- go through the REFERENCE here, at two final times, so that the suite can state
    what each order of operations achieves against the reference itself."""
    N, n, R = 48, 15, 100
    Yall = synth.swarm_control_points(N, 2, n, seed=528)
    veh = [9, 41, 42, 32]
    Y = np.concatenate([Yall[2 * v:2 * v + 2] for v in veh])
    d = {"Y": Y, "veh": np.array(veh), "par": np.array([len(veh), 2, n, R, 1.0])}
    for tf in (10.0, 14.3):
        opt.DEG_ELEV = R
        with np.errstate(all="ignore"):
            a = opt._maxAngularRateConstraints(Y, len(veh), 2, tf, 1.0)
        sp = opt._maxSpeedConstraints(Y, len(veh), 2, tf, 5.0)
        opt.DEG_ELEV = 0
        d["angrate_tf%g" % tf] = np.asarray(a, dtype=float)
        d["maxspeed_tf%g" % tf] = np.asarray(sp, dtype=float)
        print("  nearstop tf=%g: angrate %s, |max| %.3e" % (tf, np.asarray(a).shape, np.nanmax(np.abs(a))))
    d["tfs"] = np.array([10.0, 14.3])
    save("nearstop.npz", **d)


def gen_sequential():
    """The sequential planner's constraint (Examples/SequentialSwarm.py:43-70) through the REFERENCE's own function:
    vehicle 0 against every other vehicle, min of the elevated (by 10, hard-coded there) squared-distance control
    points minus maxSep^2 -- all K = nveh - 1 pairs of each shape.  `hawks`: the example's own shape (3-D, degree 3)
    with its final points from Examples/HawksLogo_1000pts.csv (stored as input data) and straight-line-plus-noise
    interiors; the module imports cleanly (its work is under `if __name__ == '__main__'`)."""
    import pandas as pd
    import SequentialSwarm as SS
    d = {}
    names = []
    for name, nveh, dim, deg, seed in (("v37_3d_deg5", 37, 3, 5, 71), ("v1000_2d_deg5", 1000, 2, 5, 72)):
        y = synth.swarm_control_points(nveh, dim, deg, seed=seed)
        out = SS.temporalSeparationConstraints(y, nveh, dim, 1.0)
        d[name + "_y"], d[name + "_out"] = y, np.asarray(out, dtype=float)
        d[name + "_par"] = np.array([nveh, dim, deg, 10, 1.0])
        names.append(name)
        print("  sequential %s: %s, min %.4f" % (name, out.shape, out.min()))
    df = pd.read_csv(os.path.join(REF, "Examples", "HawksLogo_1000pts.csv"))
    fin2 = np.ascontiguousarray(df.values, dtype=float)
    nveh, dim, deg, volume = fin2.shape[0], 3, 3, 100.0
    rng = np.random.default_rng(73)
    ini = volume * np.concatenate([rng.random((nveh, dim - 1)), np.zeros((nveh, 1))], axis=1)
    fin = np.concatenate((fin2, volume * np.ones((nveh, 1))), axis=1)
    s = np.linspace(0.0, 1.0, deg + 1)
    y = (ini[:, :, None] + (fin - ini)[:, :, None] * s[None, None, :]).reshape(nveh * dim, deg + 1)
    y[:, 1:-1] += rng.normal(0.0, 2.0, size=(nveh * dim, deg - 1))
    out = SS.temporalSeparationConstraints(y, nveh, dim, 1.0)
    d["hawks_y"], d["hawks_out"], d["hawks_finalpts"] = y, np.asarray(out, dtype=float), fin
    d["hawks_par"] = np.array([nveh, dim, deg, 10, 1.0])
    names.append("hawks")
    print("  sequential hawks: %s, min %.4f" % (out.shape, out.min()))
    # nveh == 1: the function's own answer
    d["single_out"] = np.asarray(SS.temporalSeparationConstraints(y[:dim], 1, dim, 1.0), dtype=float)
    # reshape / initguess of the example (layout of x and of the trajectory matrix)
    P = type("P", (), {})()
    P.ndim, P.deg, P.inipts, P.finalpts = dim, deg, ini, fin
    x0 = SS.initguess(5, P)
    d["hawks_x0_v5"] = x0
    d["hawks_reshape_v5"] = SS.reshape(x0, y[:2 * dim], dim, ini[5], fin[5])
    d["hawks_inipts"] = ini
    d["names"] = np.array(names)
    save("sequential.npz", **d)


def gen_spatial_fd():
    """Finite-difference rows of spatialSeparationConstraints through the REFERENCE (round 3): for two of spatial.npz's
    problems (one 2-D, one 3-D) the closure at x + h e_k for every variable k -- what SciPy's approx_derivative calls when
    the constraint is handed to SLSQP as Examples/ComplexObstacles.py:49-63 does.  Rows the reference does not finish
    within its time budget are marked (mask 0) and skipped by the test."""
    import contextlib
    import io
    sp = np.load(os.path.join(HERE, "spatial.npz"))
    h = 1.4901161193847656e-08
    d = {}
    names = []
    for name in ("s2d_11", "s3d_9"):
        nveh, dim, deg, max_sep = sp[name + "_par"]
        dim, deg = int(dim), int(deg)
        bo = opt.BezOptimization(numVeh=2, dimension=dim, degree=deg, minimizeGoal='Euclidean', maxSep=float(max_sep),
                                 initPoints=sp[name + "_init"], finalPoints=sp[name + "_final"],
                                 shapeObstacles=[bez.Bezier(sp[name + "_obs"].copy())])
        x = sp[name + "_x"]
        rows = np.full((x.size, 3, 3), np.nan)
        mask = np.zeros(x.size, dtype=np.int32)
        for k in range(x.size):
            xk = x.copy()
            xk[k] += h
            with contextlib.redirect_stdout(io.StringIO()):
                st, v = guarded(bo.spatialSeparationConstraints, 60.0, xk)
            if st == 0:
                rows[k] = np.asarray(v, dtype=float)
                mask[k] = 1
        d[name + "_rows"], d[name + "_mask"] = rows, mask
        names.append(name)
        print("  spatial_fd %s: %d of %d rows finished" % (name, int(mask.sum()), x.size))
    d["names"] = np.array(names)
    d["h"] = np.array(h)
    save("spatial_fd.npz", **d)


def gen_c1_text():
    """BASELINE.json configs[0] as its TEXT has it: 1 vehicle, degree 10, 4 point obstacles ->
    through the class path the obstacles join the pair loop as constant curves (optimization.py:86-98): P = C(5, 2) = 10
    pairs, 210 separation values, 21 speed values, 41 angular-rate values per evaluation."""
    d = {}
    obs = [[3.0, 2.0], [6.0, 7.0], [2.0, 8.0], [8.0, 3.0]]
    bo = opt.BezOptimization(numVeh=1, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, maxAngRate=1,
                             initPoints=[(0, 0)], finalPoints=[(10, 10)], initSpeeds=[1], finalSpeeds=[1],
                             initAngs=[0], finalAngs=[np.pi / 2], pointObstacles=obs)
    rng = np.random.default_rng(11)
    xg = bo.generateGuess(std=0)
    xr = xg + rng.normal(0, 0.4, size=xg.shape)
    xr[-1] = 4.2
    d["obs"] = np.array(obs)
    for tag, x in (("g", xg), ("r", xr)):
        d["x_" + tag] = x
        d["y_" + tag] = bo.reshapeVector(x)
        opt.DEG_ELEV = 0
        d["tsep_" + tag] = bo.temporalSeparationConstraints(x)
        d["maxspeed_" + tag] = bo.maxSpeedConstraints(x)
        d["angrate_" + tag] = bo.maxAngularRateConstraints(x)
    assert d["tsep_r"].shape == (210,) and d["maxspeed_r"].shape == (21,) and d["angrate_r"].shape == (41,)
    save("c1_text.npz", **d)


def gen_fullsize():
    """BASELINE configs 4 and 5 at their FULL shapes through the reference's own closures
    (optimization.py:311-459): until round 5 the reference had seen these degrees / elevations only on
    8- and 12-vehicle swarms (`c3s_R100`, `c4s` in constraints.npz) and the full shapes were held to the
    oracle alone.  C5 (64 vehicles, degree 10, DEG_ELEV 100): every output in full (2.2 MB).  C4 (256
    vehicles, degree 15): speed and angular-rate rows in full; of the 1 011 840 separation values the
    per-pair minimum, the per-pair sum (both over a pair's 31 control points, so every value is
    pinned through one of them) and every 7th value."""
    import time
    d = {}
    for name, N, n, R in (("c5", 64, 10, 100), ("c4", 256, 15, 0)):
        Y = synth.swarm_control_points(N, 2, n, seed=1234)
        t0 = time.perf_counter()
        r = ref_constraints(Y, N, 2, 10.0, 0.9, 5.0, 0.3, 1.0, R)
        print("  %s: reference closures %.2f s, tsep %d, speed %d, angrate %d values" % (
            name, time.perf_counter() - t0, r["tsep"].size, r["maxspeed"].size, r["angrate"].size))
        d[name + "_Y"] = Y
        d[name + "_par"] = np.array([N, 2, n, R, 10.0, 0.9, 5.0, 0.3, 1.0])
        d[name + "_maxspeed"], d[name + "_minspeed"], d[name + "_angrate"] = r["maxspeed"], r["minspeed"], r["angrate"]
        if name == "c5":
            d[name + "_tsep"] = r["tsep"]
        else:
            L = 2 * n + R + 1
            blk = r["tsep"].reshape(-1, L)
            d[name + "_tsep_min"] = blk.min(axis=1)
            d[name + "_tsep_sum"] = blk.sum(axis=1)
            d[name + "_tsep_every7"] = r["tsep"][::7].copy()
            d[name + "_tsep_absmax"] = np.array(np.abs(r["tsep"]).max())
    save("fullsize.npz", **d)


def gen_c4_hulls():
    """BASELINE config 4's hull sweep through the reference: gjkNew on all C(256, 2) = 32 640 pairs of the seeded
    256-vehicle degree-15 swarm (16-point control polygons), with the support-index trace of every pair.  Closest
    points are left out (1.5 MB); flag, distance, status and traces are what the bit-exactness bar is about."""
    import time
    N, n = 256, 15
    Y = synth.swarm_control_points(N, 2, n, seed=1234)
    polys = synth.hulls_from_Y(Y, 2)
    pa, pb = synth.swarm_pairs(N, 0)
    t0 = time.perf_counter()
    g = gjk_group(polys, pa, pb)
    ok = g["status"] == 0
    print("  c4 hulls: %d pairs in %.1f s, flags(-1,0,1) %s, timeouts %d, mean supports %.2f" % (
        len(pa), time.perf_counter() - t0, np.bincount(g["flag"][ok] + 1, minlength=3), (~ok).sum(), np.diff(g["trace_off"])[ok].mean()))
    d = {"c4_" + k: v for k, v in g.items() if k not in ("c1", "c2")}
    d["Y"] = Y
    save("c4_hulls.npz", **d)


def _slsqp_attempts(bo, cons, bounds=None, max_retries=8):
    """The drivers' `results = minimize(...); while not results.success: xGuess = generateGuess(std=std); ...` loop
    (Examples/DubinsCarTimeOptimal.py:109-137) with SEEDED retries (seed 100 + std; the examples draw unseeded).  One
    record per attempt: start, outcome (1 success, 0 SLSQP gave up, -1 the reference raised TypeError -- SLSQP stepped to
    tf <= 0, where Bezier.sub returns None, bezier.py:365-368, and optimization.py:604 multiplies None by None), fun, nit, x."""
    import scipy.optimize as sop
    kw = dict(method='SLSQP', constraints=cons, options={'maxiter': 250, 'disp': False})
    if bounds is not None:
        kw['bounds'] = bounds
    x0s, outcome, funs, nits, xs = [], [], [], [], []
    x0 = bo.generateGuess(std=0)
    std = 0
    while True:
        x0s.append(x0)
        try:
            with np.errstate(all='ignore'):
                r = sop.minimize(bo.objectiveFunction, x0=x0, **kw)
            outcome.append(1 if r.success else 0); funs.append(r.fun); nits.append(r.nit); xs.append(r.x)
        except TypeError:
            outcome.append(-1); funs.append(np.nan); nits.append(-1); xs.append(np.full_like(x0, np.nan))
        if outcome[-1] == 1 or std >= max_retries:
            break
        std += 1
        x0 = bo.generateGuess(std=std, seed=100 + std)
    return dict(x0=np.array(x0s), outcome=np.array(outcome, np.int32), fun=np.array(funs), nit=np.array(nits, np.int32),
                x=np.array(xs))


def gen_drivers():
    """The three example drivers the package had no fixtures for (round 5): Examples/DubinsCarTimeOptimal.py:60-137 and
    Examples/DubinsCarExample2.py:83-140 (degree 8: 9 control points, speeds and angles prescribed, point obstacles,
    time-optimal, retry-with-noisier-guess loop; the second one with bounds and DEG_ELEV) and
    Examples/DrivingOnATrack.py:18-50 (scalar constructor arguments, list-built Bezier tracks as shapeObstacles).
    Constraint vectors at the drivers' own guess and at a noisy one, DEG_ELEV 0 and 10, and the outcome of every
    attempt of the SLSQP loops."""
    d = {}

    def dubins_time_optimal():
        return opt.BezOptimization(numVeh=1, dimension=2, degree=8, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5,
                                   maxAngRate=1, initPoints=[(3, 0)], finalPoints=[(7, 10)], initSpeeds=[1], finalSpeeds=[1],
                                   initAngs=[np.pi / 2], finalAngs=[np.pi / 2], pointObstacles=[[3, 2], [6, 7]])

    def dubins_example2():
        return opt.BezOptimization(numVeh=1, dimension=2, degree=8, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=3,
                                   maxAngRate=np.pi / 2, initPoints=[(0, 0)], finalPoints=[(12, 8)], initSpeeds=[1],
                                   finalSpeeds=[1], tf=8, initAngs=[np.pi / 2], finalAngs=[0],
                                   pointObstacles=[(3, 2), (7, 6), (9, 9), (4, 5), (5, 8), (3, 7), (7, 3)])

    import scipy.optimize as sop
    for pre, make, bounds in (("tt", dubins_time_optimal, None),
                              ("e2", dubins_example2, sop.Bounds([-100] * 10 + [0.0001], [100] * 10 + [50], [False] * 10 + [True]))):
        for R in (0, 10):
            opt.DEG_ELEV = R
            bo = make()
            cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints}, {'type': 'ineq', 'fun': bo.maxSpeedConstraints},
                    {'type': 'ineq', 'fun': bo.maxAngularRateConstraints}, {'type': 'ineq', 'fun': lambda x: x[-1]}]
            xs = np.array([bo.generateGuess(std=0), bo.generateGuess(std=0.3, seed=7)])
            d["%s_x" % pre] = xs
            d["%s_y" % pre] = np.array([bo.reshapeVector(x) for x in xs])
            with np.errstate(all="ignore"):
                d["%s_R%d_tsep" % (pre, R)] = np.array([bo.temporalSeparationConstraints(x) for x in xs])
                d["%s_R%d_maxspeed" % (pre, R)] = np.array([bo.maxSpeedConstraints(x) for x in xs])
                d["%s_R%d_angrate" % (pre, R)] = np.array([bo.maxAngularRateConstraints(x) for x in xs])
            a = _slsqp_attempts(bo, cons, bounds)
            for k, v in a.items():
                d["%s_R%d_flow_%s" % (pre, R, k)] = v
            print("  %s DEG_ELEV %d: attempts %s, fun %s, nit %s" % (pre, R, a["outcome"], np.round(a["fun"], 6), a["nit"]))
    opt.DEG_ELEV = 0
    # DrivingOnATrack.py: the constructor takes scalars / one tuple, the tracks are Beziers built from lists
    tracks = [[[0, 0, 0, 3, 4, 5, 6, 7, 10, 10, 10], [0, 3, 4, 5, 6, 6, 6, 6, 7, 8, 10]],
              [[4, 4, 4, 7, 8, 9, 10, 11, 14, 14, 14], [0, 3, 4, 4, 4, 5, 5, 5, 7, 8, 10]]]
    bo = opt.BezOptimization(numVeh=1, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=0.5, maxSpeed=5,
                             maxAngRate=0.5, initPoints=(2, 1), finalPoints=(12, 9), initSpeeds=1, finalSpeeds=1,
                             initAngs=np.pi / 2, finalAngs=np.pi / 2, shapeObstacles=[bez.Bezier(t) for t in tracks])
    xg = bo.generateGuess()
    xg[-1] = 10
    d["tr_tracks"] = np.array(tracks, dtype=float)
    d["tr_x"] = xg
    d["tr_y"] = bo.reshapeVector(xg)
    d["tr_maxspeed"] = bo.maxSpeedConstraints(xg)
    d["tr_angrate"] = bo.maxAngularRateConstraints(xg)
    sys.setrecursionlimit(1000)
    curves = [bez.Bezier(d["tr_y"][0:2, :])] + list(bo.shapeObstacles)
    st = []
    for i in range(3):
        for j in range(i + 1, 3):
            s_, v = guarded(curves[i].minDist, 30.0, curves[j])
            st.append(s_)
    d["tr_mindist_status"] = np.array(st, np.int32)          # 2 = RecursionError in the reference (all three pairs)
    s_, v = guarded(bo.spatialSeparationConstraints, 60.0, xg)
    d["tr_spatial_status"] = np.array(s_, np.int32)
    print("  track: minDist status per pair %s, spatialSeparationConstraints status %d" % (st, s_))
    save("drivers.npz", **d)


def gen_trajectories():
    """Teacher-forced trajectory fixtures (round 6): the reference's OWN drivers run with an SLSQP `callback` that records
    every iterate x_k, and every constraint closure's value there.  SLSQP amplifies the last bits of its callbacks, so two
    float64 implementations do not stay on one trajectory (drivers.npz pins only outcomes); the iterates the REFERENCE
    visited are data, and a replacement can be held to the reference's values at each of them with no SLSQP in the loop.
      ex1_R{0,30}   Examples/Example1_DubinsCarTimeOptimal.py:94-148 (2 vehicles, degree 10, its own separation function
                    with degElev, speed / angular rate at DEG_ELEV 0)
      tt_R{0,10}    Examples/DubinsCarTimeOptimal.py:60-137, the attempt of its retry loop that converges (seeded guesses
                    as in drivers.npz)
      e2_R{0,10}    Examples/DubinsCarExample2.py:83-140, likewise (bounds)
      sw            Examples/SwarmOfAerialVehicles.py:137-170 with the first 8 vehicles of its image (3-D, degree 5; the
                    example's own initial guess; at most 40 iterations are kept)"""
    import scipy.optimize as sop
    import Example1_DubinsCarTimeOptimal as ex1
    import SwarmOfAerialVehicles as swm
    d = {}
    names = []

    def record(tag, bo, cons_named, x0, bounds=None, maxiter=250, keep=400):
        xs = [np.array(x0, dtype=float)]
        kw = dict(method='SLSQP', constraints=[{'type': 'ineq', 'fun': f} for _, f in cons_named] + [{'type': 'ineq', 'fun': lambda x: x[-1]}]
                  if bo.model['minGoal'].lower() == 'timeopt' else [{'type': 'ineq', 'fun': f} for _, f in cons_named],
                  options={'maxiter': maxiter, 'disp': False}, callback=lambda xk: xs.append(np.array(xk, dtype=float)))
        if bounds is not None:
            kw['bounds'] = bounds
        try:
            with np.errstate(all='ignore'):
                r = sop.minimize(bo.objectiveFunction, x0=x0, **kw)
            outcome = (1 if r.success else 0, r.nit, float(r.fun))
        except TypeError:
            outcome = (-1, -1, float('nan'))
        xs = np.array(xs[:keep])
        d[tag + "_x"] = xs
        d[tag + "_y"] = np.array([bo.reshapeVector(x) for x in xs])
        with np.errstate(all='ignore'):
            for cname, f in cons_named:
                d["%s_%s" % (tag, cname)] = np.array([f(x) for x in xs])
            d[tag + "_obj"] = np.array([bo.objectiveFunction(x) for x in xs])
        d[tag + "_outcome"] = np.array(outcome, dtype=float)
        names.append(tag)
        print("  %s: %d iterates kept, outcome %s" % (tag, len(xs), outcome))

    # Example1: two Dubins cars
    for elev in (0, 30):
        opt.DEG_ELEV = 0
        bo = opt.BezOptimization(numVeh=2, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, maxAngRate=1,
                                 initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)], initSpeeds=[1] * 2, finalSpeeds=[1] * 2,
                                 initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], pointObstacles=[[3, 2], [6, 7]])
        sep = (lambda e: (lambda x: ex1._temporalSeparationConstraints(bo.reshapeVector(x), 2, 2, 1, e)))(elev)
        record("ex1_R%d" % elev, bo, [("tsep", sep), ("maxspeed", bo.maxSpeedConstraints), ("angrate", bo.maxAngularRateConstraints)],
               bo.generateGuess(std=0))

    # the two degree-8 Dubins drivers: the attempt that converges in the reference
    def dubins_time_optimal():
        return opt.BezOptimization(numVeh=1, dimension=2, degree=8, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5,
                                   maxAngRate=1, initPoints=[(3, 0)], finalPoints=[(7, 10)], initSpeeds=[1], finalSpeeds=[1],
                                   initAngs=[np.pi / 2], finalAngs=[np.pi / 2], pointObstacles=[[3, 2], [6, 7]])

    def dubins_example2():
        return opt.BezOptimization(numVeh=1, dimension=2, degree=8, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=3,
                                   maxAngRate=np.pi / 2, initPoints=[(0, 0)], finalPoints=[(12, 8)], initSpeeds=[1],
                                   finalSpeeds=[1], tf=8, initAngs=[np.pi / 2], finalAngs=[0],
                                   pointObstacles=[(3, 2), (7, 6), (9, 9), (4, 5), (5, 8), (3, 7), (7, 3)])

    drv = np.load(os.path.join(HERE, "drivers.npz"))
    for pre, make, bounds in (("tt", dubins_time_optimal, None),
                              ("e2", dubins_example2, sop.Bounds([-100] * 10 + [0.0001], [100] * 10 + [50], [False] * 10 + [True]))):
        for R in (0, 10):
            opt.DEG_ELEV = R
            bo = make()
            outc = drv["%s_R%d_flow_outcome" % (pre, R)]
            win = int(np.nonzero(outc == 1)[0][0])
            x0 = drv["%s_R%d_flow_x0" % (pre, R)][win]
            record("%s_R%d" % (pre, R), bo, [("tsep", bo.temporalSeparationConstraints), ("maxspeed", bo.maxSpeedConstraints),
                                             ("angrate", bo.maxAngularRateConstraints)], x0, bounds)
            d["%s_R%d_attempt" % (pre, R)] = np.array(win)
    # the 3-D swarm, 8 vehicles
    opt.DEG_ELEV = 0
    nveh_all, initPts, finalPts = swm.generatePointsFromImage(swm.CAS_IMG)
    sel = np.arange(8)
    bo = opt.BezOptimization(numVeh=8, dimension=3, degree=5, minimizeGoal='Euclidean', maxSep=0.9,
                             initPoints=initPts[sel], finalPoints=finalPts[sel])
    d["sw_init"], d["sw_final"] = initPts[sel], finalPts[sel]
    record("sw", bo, [("tsep", bo.temporalSeparationConstraints)], swm.generate3DGuess(initPts[sel], finalPts[sel], 5), maxiter=40, keep=41)
    opt.DEG_ELEV = 0
    d["names"] = np.array(names)
    save("trajectories.npz", **d)


if __name__ == "__main__":
    which = sys.argv[1:] or ["trajectories", "tables", "ops", "problem", "constraints", "gjk", "mindist", "c5", "spatial", "nearstop", "sequential", "spatial_fd", "mindist_script", "c1_text", "fullsize", "drivers", "c4_hulls"]
    for w in which:
        if w == "none":          # import-only (exploration)
            continue
        print("== " + w)
        globals()["gen_" + w]()
