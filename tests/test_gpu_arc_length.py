"""True arc length on the device (obtg_bern_arc_length, obtg_arc_length_obj, Bezier.arcLength, BezOptimization(minGoal=
'arcLength')) against the 60-digit yardstick of tests/arc_length_ref.py.

Bounds, with S the length of the control polygon, u = 2^-53 and the operation counts K of arc_length_ref.py:
    |len - ref| <= eps_rel S + k_len u S,   err <= eps_rel S,   chord (1 - k_len u) <= len <= S (1 + k_len u)    (status OK)
    |sum_ci grad[c][i] (P_ci - P_c0) - len| <= k_identity u S     (the speed is homogeneous of degree 1; P_c0 is taken off
                                                                   first, which translation invariance allows, so that every
                                                                   factor is bounded by S)
    |sum_i grad[c][i]| <= 2 (n + 1) k_grad u                      (translation invariance; the gradient has no unit, so this
                                                                   bound has no S: every case here has S >= 1, so it is never
                                                                   wider than k u S)
    |grad - ref grad| <= GRAD_TOL[eps_rel]                        (regular cases: 4 x the rule's own error measured on the CPU)
Both identities are evaluated in exact rational arithmetic, so the test adds no rounding of its own.
Every case is at most 257 curves."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arc_length_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = R.UNIT
CASES = [(n, d) for n in R.DEGREES for d in R.DIMS]


@pytest.fixture(scope="module")
def ctx():
    from optimalbeziertrajectorygeneration_amd import _capi
    return _capi.scratch_context()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _curve(n, d):
    return R.random_curve(n, d, R.SEEDS[(n, d)])


def _hold_identities(P, length, grad, nodes, what):
    """the two rounding-level identities of the gradient, in exact arithmetic"""
    P = np.atleast_2d(P)
    d, n = P.shape[0], P.shape[1] - 1
    S = float(R.polygon_and_chord(P)[0])
    dot = sum(Fraction(float(grad[c][i])) * (Fraction(float(P[c][i])) - Fraction(float(P[c][0]))) for c in range(d) for i in range(n + 1))
    gap = abs(float(dot - Fraction(float(length))))
    rows = [abs(float(sum(Fraction(float(g)) for g in grad[c]))) for c in range(d)]
    print("%s: |grad.P - len| = %.3e (bound %.3e)   max |sum_i grad| = %.3e (bound %.3e)"
          % (what, gap, R.k_identity(n, d, nodes) * U * S, max(rows), 2 * (n + 1) * R.k_grad(n, d, nodes) * U))
    assert gap <= R.k_identity(n, d, nodes) * U * S, what
    assert max(rows) <= 2 * (n + 1) * R.k_grad(n, d, nodes) * U, what


def _hold_value(P, r, i, eps, breaks, what):
    P = np.atleast_2d(P)
    d, n = P.shape[0], P.shape[1] - 1
    ref = R.reference_of(P, breaks=breaks)
    S, chord, L = float(ref["S"]), float(ref["chord"]), float(ref["len"])
    length, err, nodes = float(r["len"][i]), float(r["err"][i]), int(r["nodes"][i])
    k = R.k_len(n, d, nodes)
    print("%s: len - ref = %.3e (bound %.3e)  err %.3e  nodes %d" % (what, length - L, eps * S + k * U * S, err, nodes))
    assert r["status"][i] == R.MD_OK, what
    assert abs(float(Fraction(length) - Fraction(ref["len"]))) <= eps * S + k * U * S, what
    assert err <= eps * S, what
    assert chord * (1 - k * U) <= length <= S * (1 + k * U), what
    return ref


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("n,d", CASES)
def test_random_curves(ctx, n, d, eps):
    """One seeded curve per degree and dimension, every bound of the module docstring.  (In one dimension chord = L = S: the
    bracket leaves room for rounding alone, and the 8-point rule is not exact above degree 16.)"""
    P = _curve(n, d)
    ref0 = R.reference_of(P)
    assert R.min_speed_over_grid(P) > R.MIN_SPEED * float(ref0["S"]) and float(ref0["S"]) >= 1.0
    r = ctx.bern_arc_length(P, eps_rel=eps, grad=True)
    what = "deg %d dim %d eps %.0e" % (n, d, eps)
    ref = _hold_value(P, r, 0, eps, (), what)
    _hold_identities(P, r["len"][0], r["grad"][0], r["nodes"][0], what)
    g = np.array([[float(v) for v in row] for row in ref["grad"]])
    worst = float(np.abs(r["grad"][0] - g).max())
    print("%s: max |grad - ref| = %.3e (bound %.3e)" % (what, worst, R.GRAD_TOL[eps]))
    assert np.abs(r["grad"][0]).max() <= 2.0 + 1e-9
    assert worst <= R.GRAD_TOL[eps], what
    # without the gradient: the same bits
    r0 = ctx.bern_arc_length(P, eps_rel=eps)
    for key in ("len", "err"):
        assert np.array_equal(_bits(r0[key]), _bits(r[key])), key
    assert np.array_equal(r0["nodes"], r["nodes"]) and np.array_equal(r0["status"], r["status"])


@pytest.mark.parametrize("eps", [1e-3, 1e-6, 1e-10, 1e-13, 0.0])
def test_elevated_line(ctx, eps):
    for d, p0, p1, deg in ((2, [0.25, -1.0], [3.25, 3.0], 7), (3, [1.0, -2.0, 0.5], [4.0, 2.0, 0.5], 8), (1, [-1.5], [2.0], 31)):
        P = R.elevated_line(p0, p1, deg)
        r = ctx.bern_arc_length(P, eps_rel=eps, grad=True)
        ref = R.reference_of(P)
        S = float(ref["S"])
        assert r["nodes"][0] == 3 and r["status"][0] == R.MD_OK, (d, deg)
        assert abs(float(Fraction(float(r["len"][0])) - Fraction(ref["len"]))) <= R.k_len(deg, d, 3) * U * S, (d, deg)
        _hold_identities(P, r["len"][0], r["grad"][0], 3, "line dim %d" % d)


def test_constant_curve(ctx):
    for d, K in ((2, 6), (3, 11), (1, 2)):
        P = np.repeat(np.array([[0.75], [-2.5], [1e3]])[:d], K, axis=1)
        r = ctx.bern_arc_length(P, eps_rel=1e-10, grad=True)
        assert r["status"][0] == R.MD_OK and r["len"][0] == 0.0 and r["err"][0] == 0.0
        assert np.array_equal(r["grad"][0], np.zeros((d, K))) and not np.isnan(r["grad"]).any()


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("t0", [0.5, 0.3])
def test_cusp_cubics(ctx, t0, eps):
    P = R.CUSP_HALF if t0 == 0.5 else R.cusp_at(t0)
    r = ctx.bern_arc_length(P, eps_rel=eps, grad=True)
    what = "cusp at %.1f eps %.0e" % (t0, eps)
    _hold_value(P, r, 0, eps, (t0,), what)
    _hold_identities(P, r["len"][0], r["grad"][0], r["nodes"][0], what)
    if t0 == 0.5:
        assert abs(r["len"][0] - (2.0 * 2.0 ** 0.5 - 1.0)) <= eps * 4.0 + R.k_len(3, 2, r["nodes"][0]) * U * 4.0


def test_non_finite_control_point(ctx):
    for bad in (np.nan, np.inf):
        P = np.stack([_curve(10, 2), _curve(10, 2), _curve(10, 2)])
        P[1, 1, 4] = bad
        r = ctx.bern_arc_length(P, eps_rel=1e-10, grad=True)
        assert np.isnan(r["len"][1]) and np.isnan(r["err"][1]) and np.isnan(r["grad"][1]).all()
        assert r["nodes"][1] == 0 and r["status"][1] == R.MD_OK
        alone = ctx.bern_arc_length(P[0], eps_rel=1e-10, grad=True)
        for i in (0, 2):
            assert np.array_equal(_bits(r["len"][i]), _bits(alone["len"][0])) and np.array_equal(_bits(r["grad"][i]), _bits(alone["grad"][0]))


def test_node_cap(ctx):
    P = _curve(10, 2)
    r = ctx.bern_arc_length(P, eps_rel=1e-10, max_nodes=3, grad=True)
    k = R.kernel_rule(P, 1e-10, max_nodes=3)
    assert k["status"] == R.MD_NODE_CAP
    assert r["status"][0] == R.MD_NODE_CAP and r["nodes"][0] == 3 and np.isfinite(r["len"][0]) and np.isfinite(r["grad"]).all()
    assert abs(r["len"][0] - k["len"]) <= 2 * R.k_len(10, 2, 3) * U * k["S"]
    _hold_identities(P, r["len"][0], r["grad"][0], 3, "node cap")          # the gradient is that of the returned len
    full = ctx.bern_arc_length(P, eps_rel=1e-10)
    assert full["status"][0] == R.MD_OK and full["nodes"][0] > 3


def test_degree_limits(ctx):
    from optimalbeziertrajectorygeneration_amd import _capi
    with pytest.raises(_capi.ObtgError) as e:
        ctx.bern_arc_length(R.elevated_line([0.0, 0.0], [1.0, 1.0], 32))
    assert e.value.code == _capi.ERR_UNSUPPORTED
    with pytest.raises(_capi.ObtgError) as e:
        ctx.bern_arc_length(np.zeros((4, 6)))
    assert e.value.code == -1
    r = ctx.bern_arc_length(R.elevated_line([0.0, 0.0], [3.0, 4.0], 31), eps_rel=1e-10)
    assert r["status"][0] == R.MD_OK and abs(r["len"][0] - 5.0) <= R.k_len(31, 2, 3) * U * 5.0


def _elevate_to(P, deg):
    """exact degree elevation (rational arithmetic), rounded once"""
    rows = [[Fraction(float(v)) for v in row] for row in P]
    n = len(rows[0]) - 1
    while n < deg:
        rows = [[(Fraction(i, n + 1) * row[i - 1] if i > 0 else 0) + (Fraction(n + 1 - i, n + 1) * row[i] if i <= n else 0)
                 for i in range(n + 2)] for row in rows]
        n += 1
    return np.array([[float(v) for v in row] for row in rows])


def _batch257():
    rng = np.random.default_rng(257)
    B = np.cumsum(rng.standard_normal((257, 2, 11)), axis=2)
    B[5], B[131], B[255] = _elevate_to(R.CUSP_HALF, 10), _elevate_to(R.cusp_at(0.3), 10), _elevate_to(R.CUSP_HALF, 10)
    for i in (0, 130, 256):
        B[i] = _curve(10, 2)
    return B


@pytest.mark.parametrize("eps", R.EPS)
def test_independent_of_batch_and_entry(ctx, eps):
    import torch
    alone = ctx.bern_arc_length(_curve(10, 2), eps_rel=eps, grad=True)
    B = _batch257()
    r = ctx.bern_arc_length(B, eps_rel=eps, grad=True)
    for i in (0, 130, 256):
        for key in ("len", "err", "grad"):
            assert np.array_equal(_bits(r[key][i]), _bits(alone[key][0])), (i, key)
        assert r["nodes"][i] == alone["nodes"][0] and r["status"][i] == alone["status"][0]
    assert np.array_equal(_bits(r["len"][5]), _bits(r["len"][255])) and np.array_equal(_bits(r["grad"][5]), _bits(r["grad"][255]))
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        dc = torch.from_numpy(np.ascontiguousarray(B)).to(dev)
        dl, de = (torch.empty(257, dtype=torch.float64, device=dev) for _ in range(2))
        dn, ds = (torch.empty(257, dtype=torch.int32, device=dev) for _ in range(2))
        dg = torch.empty((257, 2, 11), dtype=torch.float64, device=dev)
        ctx.bern_arc_length_dev(dc.data_ptr(), 257, 2, 11, dl.data_ptr(), de.data_ptr(), dn.data_ptr(), ds.data_ptr(), dg.data_ptr(), eps_rel=eps)
        torch.cuda.synchronize()
        for key, t in (("len", dl), ("err", de), ("grad", dg)):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(r[key])), key
        assert np.array_equal(dn.cpu().numpy(), r["nodes"]) and np.array_equal(ds.cpu().numpy(), r["status"])
        # the value alone, every optional output left out
        dl2 = torch.empty(257, dtype=torch.float64, device=dev)
        ctx.bern_arc_length_dev(dc.data_ptr(), 257, 2, 11, dl2.data_ptr(), eps_rel=eps)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(dl2.cpu().numpy()), _bits(r["len"]))
    finally:
        ctx.use_own_stream()


def test_objective_is_the_vehicle_order_sum(ctx):
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    N, d, n, B = 3, 3, 5, 7
    rng = np.random.default_rng(11)
    Y = np.cumsum(rng.standard_normal((B, N * d, n + 1)), axis=2)
    Y[2, 3:6] = 1.25                                   # a vehicle at rest
    c = _capi.Context(N, d, n)
    o = c.arc_length_obj(Y, eps_rel=1e-10, grad=True)
    r = ctx.bern_arc_length(Y.reshape(B * N, d, n + 1), eps_rel=1e-10, grad=True)
    want = np.empty(B)
    for b in range(B):
        s = 0.0
        for v in range(N):
            s += r["len"][b * N + v]
        want[b] = s
    assert np.array_equal(_bits(o["val"]), _bits(want))
    assert np.array_equal(_bits(o["grad"]), _bits(r["grad"].reshape(B, N * d, n + 1)))
    assert np.array_equal(o["status"], r["status"].reshape(B, N).max(axis=1))
    assert np.array_equal(_bits(c.arc_length_obj(Y, eps_rel=1e-10)["val"]), _bits(want))
    capped = c.arc_length_obj(Y, eps_rel=1e-10, max_nodes=3)
    assert capped["status"][2] == R.MD_NODE_CAP and np.isfinite(capped["val"]).all()
    dev = torch.device("cuda", 0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(Y).to(dev)
    do, dg = torch.empty(B, dtype=torch.float64, device=dev), torch.empty((B, N * d, n + 1), dtype=torch.float64, device=dev)
    ds = torch.empty(B, dtype=torch.int32, device=dev)
    c.arc_length_obj_dev(dY.data_ptr(), B, do.data_ptr(), ds.data_ptr(), dg.data_ptr(), eps_rel=1e-10)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(do.cpu().numpy()), _bits(want)) and np.array_equal(_bits(dg.cpu().numpy()), _bits(o["grad"]))
    assert np.array_equal(ds.cpu().numpy(), o["status"])
    c.close()


def test_kernel_stats_id(ctx):
    ctx.reset_kernel_stats()
    ctx.set_profiling(True, only="arc_length")
    ctx.bern_arc_length(_curve(10, 2), eps_rel=1e-10, grad=True)
    st = ctx.kernel_stats()
    ctx.set_profiling(False)
    assert st["arc_length"][1] == 1 and st["arc_length"][0] > 0.0 and st["bern"][1] == 0


# ---------------------------------------------------------------------------------------------------------------------
#  the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_bezier_arc_length(ctx):
    from optimalbeziertrajectorygeneration_amd.bezier import Bezier
    P = _curve(8, 3)
    assert Bezier(P, t0=1.0, tf=4.0).arcLength() == ctx.bern_arc_length(P, eps_rel=1e-12)["len"][0]
    assert Bezier(P).arcLength(eps=1e-6) == ctx.bern_arc_length(P, eps_rel=1e-6)["len"][0]
    with pytest.raises(RuntimeError):
        Bezier(_curve(10, 2)).arcLength(max_nodes=3)
    cp = np.random.default_rng(6).uniform(-3.0, 3.0, (3, 7))
    got = Bezier(cp, t0=1.0, tf=3.0).integrate()
    assert [float(v).hex() for v in got] == [float(3.0 * sum(list(row)) / 7).hex() for row in cp]


def _problem(goal):
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal=goal, maxSep=1, maxSpeed=5, minSpeed=0.2, maxAngRate=1, tf=10.0,
                           initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)], initSpeeds=[1, 1], finalSpeeds=[1, 1],
                           initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2])


def test_optimization_goal():
    bo = _problem('arcLength')
    c = bo._ctx(False)
    x = bo.generateGuess(std=0.3, seed=3)
    Y = bo.reshapeVector(x)
    eps = bo.ARC_LENGTH_EPS_REL
    assert eps == 1e-12
    o = c.arc_length_obj(Y, eps_rel=eps, grad=True)
    assert bo.objectiveFunction(x) == o["val"][0]
    X, dx = bo._fd_rows(x)
    F = c.arc_length_obj(bo.reshapeVectors(X), eps_rel=eps)["val"]
    assert np.array_equal(_bits(bo.objectiveGradient(x, method='fd')), _bits((F[1:] - F[0]) / dx))
    first = bo._rv_parts()[1]
    assert np.array_equal(_bits(bo.objectiveGradient(x, method='exact')), _bits(o["grad"][0][:, first:first + bo._numCols].ravel()))
    L = bo.trueArcLengths(x)
    assert L.shape == (2,) and float(L[0]) + float(L[1]) == o["val"][0]
    # the exact gradient is the derivative the differences approximate: central differences at a step that keeps the rule's
    # tolerance (1e-12 S, over 2 h: 1e-7) and the third derivative (h^2 / 6) small
    h, g = 1e-4, bo.objectiveGradient(x, method='exact')
    for k in range(x.size):
        e = np.zeros(x.size)
        e[k] = h
        assert abs((bo.objectiveFunction(x + e) - bo.objectiveFunction(x - e)) / (2 * h) - g[k]) <= 1e-6
    # SciPy's differences of the closure are served from one batch, with the one-row call's values
    f0 = bo.objectiveFunction(x)
    xk = x.copy()
    xk[1] += 1.4901161193847656e-08
    assert bo.objectiveFunction(xk) == c.arc_length_obj(bo.reshapeVector(xk), eps_rel=eps)["val"][0] and f0 == o["val"][0]
    assert _problem('Euclidean').trueArcLengths(x).sum() == L.sum()        # whatever the goal is
    bad = _problem('arcLength')
    bad.model['minGoal'] = 'shortest'
    with pytest.raises(ValueError):
        bad.objectiveFunction
    with pytest.raises(ValueError):
        bad.objectiveGradient(x, method='exact')


def test_slsqp_with_the_exact_gradient():
    """One SLSQP run per goal from the same guess, at most 50 iterations.  The arc-length run has to end with status 0.  That
    its true length is no longer than the Euclidean solution's does not follow from reasoning alone (SLSQP is a local method
    under the non-convex separation constraint), so both lengths are printed and not compared."""
    import scipy.optimize as sop
    out = {}
    for goal in ('Euclidean', 'arcLength'):
        bo = _problem(goal)
        x0 = bo.generateGuess(std=0)
        cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints, 'jac': bo.temporalSeparationJacobian},
                {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': bo.maxSpeedJacobian}]
        res = sop.minimize(bo.objectiveFunction, x0=x0, method='SLSQP', constraints=cons,
                           jac=lambda x, bo=bo: bo.objectiveGradient(x, method='exact'), options={'maxiter': 50, 'disp': False})
        out[goal] = (res.status, res.nit, float(bo.trueArcLengths(res.x).sum()), float(res.fun))
        print("%s: status %d nit %d true length %.9f objective %.9f" % ((goal,) + out[goal]))
    assert out['arcLength'][0] == 0
    assert abs(out['arcLength'][2] - out['arcLength'][3]) == 0.0
