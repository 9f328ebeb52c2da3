"""True Bernstein extrema on the device (obtg_bern_extrema, obtg_temporal_sep_true_min, Bezier.min / max,
BezOptimization(separationRows='true_min')) against the exact yardstick of tests/extrema_ref.py.

Rounding allowance throughout: r = 1e-12 * s, s the row's largest coefficient magnitude (a de Casteljau level costs two
roundings, K <= 41, depth <= 50: 2 * 41 * 50 * 1.1e-16 = 4.5e-13)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extrema_ref as R  # noqa: E402
from util import RTOL  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 6, 11, 21, 31, 41)
C6 = [(0, 1, 2, 3, 4, 5), (5, 0, 2, 5, 7, 5)]
C6_MIN, C6_MAX = 2.2606668630782703, 5.699106677492463        # 200 001 samples; the yardstick brackets them (test_extrema_ref)


@pytest.fixture(scope="module")
def ctx():
    from optimalbeziertrajectorygeneration_amd import _capi
    return _capi.scratch_context()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_yard = {}


def _bracket(row, want_max=False):
    key = (np.ascontiguousarray(row, dtype=np.float64).tobytes(), want_max)
    if key not in _yard:
        _yard[key] = (R.certified_max if want_max else R.certified_min)(row)
    return _yard[key]


def _hold(row, val, t, bound, eps_rel, want_max=False, what="", bound_gap=True):
    """one row of the device against the yardstick, as the issue states it (the maximum through the negated row)"""
    sgn = -1.0 if want_max else 1.0
    y = _bracket(row, want_max)
    s = float(y["s"])
    r, tol = 1e-12 * s, eps_rel * s
    L, H = (-float(y["H"]), -float(y["L"])) if want_max else (float(y["L"]), float(y["H"]))
    v, b = sgn * val, (sgn * bound if bound is not None else None)
    print("%s: val - H = %.3e  (tol %.1e, r %.1e)" % (what, v - H, tol, r))
    assert L - r <= v <= H + tol + r, what
    if b is not None:
        assert b <= H + r, what
        if bound_gap:
            assert v - b <= tol, what
    assert 0.0 <= t <= 1.0, what
    assert abs(float(O.curve_eval(row, [t], 0.0, 1.0)[0, 0]) - val) <= r, what


def _random_rows(K, per=8, seed=0):
    rng = np.random.default_rng(1000 * K + seed)
    rows = [rng.uniform(-1.0, 1.0, K) * 10.0 ** e for e in (-6, 0, 6) for _ in range(per)]
    return np.array(rows)


@pytest.mark.parametrize("eps_rel", [RTOL, 1e-6])
@pytest.mark.parametrize("K", KS)
def test_random_rows(ctx, K, eps_rel):
    from optimalbeziertrajectorygeneration_amd import _capi
    c = _random_rows(K)
    for want_max in (False, True):
        g = ctx.bern_extrema(c, want_max=want_max, eps_rel=eps_rel)
        assert (g["status"] == _capi.MD_OK).all(), (K, want_max, g["status"])
        for i in range(c.shape[0]):
            _hold(c[i], g["val"][i], g["t_star"][i], g["bound"][i], eps_rel, want_max, "K=%d row %d max=%d" % (K, i, want_max))


def test_special_rows(ctx):
    from optimalbeziertrajectorygeneration_amd import _capi
    K = 7
    rng = np.random.default_rng(3)
    first = rng.uniform(1.0, 2.0, (5, K)); first[:, 0] = 0.5
    last = rng.uniform(1.0, 2.0, (5, K)); last[:, -1] = -0.25
    for c, t, col in ((first, 0.0, 0), (last, 1.0, -1)):
        g = ctx.bern_extrema(c)
        assert np.array_equal(_bits(g["val"]), _bits(c[:, col])) and (g["t_star"] == t).all() and (g["nodes"] == 1).all()
        assert (g["status"] == _capi.MD_OK).all() and np.array_equal(_bits(g["bound"]), _bits(c[:, col]))
    # constants and ties (the smallest coefficient at an end AND inside: the end is the answer)
    const = np.full((3, K), 4.75)
    g = ctx.bern_extrema(const)
    assert (g["val"] == 4.75).all() and (g["nodes"] == 1).all() and (g["t_star"] == 0.0).all()
    tie = rng.uniform(1.0, 2.0, (4, K)); tie[:, 3] = 0.5; tie[:, -1] = 0.5
    g = ctx.bern_extrema(tie)
    assert (g["val"] == 0.5).all() and (g["t_star"] == 1.0).all() and (g["nodes"] == 1).all()
    # tangent double minima: ((t - 1/4)(t - 3/4))^2 - 1/2 at degree 4 and elevated (coefficients as Fractions, then rounded)
    from fractions import Fraction as F
    from math import comb
    q = [F(3, 16), F(-1), F(1)]
    sq = [sum(q[i] * q[k - i] for i in range(3) if 0 <= k - i < 3) for k in range(5)]
    sq[0] -= F(1, 2)
    bern = [sum(F(comb(k, i), comb(4, i)) * sq[i] for i in range(k + 1)) for k in range(5)]
    for elev in (0, 3, 16):
        c = list(bern)
        for _ in range(elev):
            n = len(c)
            c = [c[0]] + [F(i, n) * c[i - 1] + F(n - i, n) * c[i] for i in range(1, n)] + [c[-1]]
        row = np.array([float(x) for x in c])
        g = ctx.bern_extrema(row[None])
        assert g["status"][0] == _capi.MD_OK
        _hold(row, g["val"][0], g["t_star"][0], g["bound"][0], RTOL, False, "double minimum, elevated %d" % elev)
        assert abs(g["val"][0] + 0.5) <= 2e-9
    # non-finite rows
    bad = rng.uniform(-1.0, 1.0, (3, K)); bad[0, 2] = np.nan; bad[1, 0] = np.inf; bad[2, -1] = -np.inf
    for want_max in (False, True):
        g = ctx.bern_extrema(bad, want_max=want_max)
        assert np.isnan(g["val"]).all() and np.isnan(g["t_star"]).all() and np.isnan(g["bound"]).all()
        assert (g["nodes"] == 0).all() and (g["status"] == _capi.MD_OK).all()
    # max == -min(-c), bit for bit
    for K2 in (4, 11, 41):
        c = _random_rows(K2, per=6, seed=7)
        a, b = ctx.bern_extrema(c, want_max=True), ctx.bern_extrema(-c)
        assert np.array_equal(_bits(a["val"]), _bits(-b["val"])) and np.array_equal(_bits(a["bound"]), _bits(-b["bound"]))
        assert np.array_equal(_bits(a["t_star"]), _bits(b["t_star"])) and np.array_equal(a["nodes"], b["nodes"])


def test_node_budget(ctx):
    from optimalbeziertrajectorygeneration_amd import _capi
    for K in (6, 21, 41):
        c = _random_rows(K, per=6, seed=11)
        inner = np.array([0 < int(np.argmin(row)) < K - 1 and min(row[0], row[-1]) - row.min() > RTOL * np.abs(row).max() for row in c])
        assert inner.sum() >= 6
        g = ctx.bern_extrema(c[inner], max_nodes=1)
        assert (g["status"] == _capi.MD_NODE_CAP).all() and (g["nodes"] == 1).all()
        for row, v, t, b in zip(c[inner], g["val"], g["t_star"], g["bound"]):
            y = _bracket(row)
            r = 1e-12 * float(y["s"])
            assert b <= float(y["L"]) + r and v >= float(y["H"]) - r and b <= v, "a valid bracket around [L, H]"
            assert abs(float(O.curve_eval(row, [t], 0.0, 1.0)[0, 0]) - v) <= r
        g = ctx.bern_extrema(c[inner], max_nodes=7)
        capped = g["status"] == _capi.MD_NODE_CAP
        assert (g["nodes"][capped] <= 7).all()
        for row, v, b in zip(c[inner], g["val"], g["bound"]):
            y = _bracket(row)
            r = 1e-12 * float(y["s"])
            assert b <= float(y["L"]) + r and v >= float(y["L"]) - r


def test_rows_are_independent(ctx):
    import torch
    rng = np.random.default_rng(21)
    K = 21
    c = rng.uniform(-10.0, 10.0, (5000, K))
    c[::7, 0] = -11.0                                     # some rows that end at node 1 among the searched ones
    g = ctx.bern_extrema(c)
    keys = ("val", "t_star", "bound")
    rev = ctx.bern_extrema(c[::-1].copy())
    for k in keys:
        assert np.array_equal(_bits(g[k]), _bits(rev[k][::-1])), k
    assert np.array_equal(g["nodes"], rev["nodes"][::-1]) and np.array_equal(g["status"], rev["status"][::-1])
    for i in list(range(0, 5000, 97)) + [4999]:
        one = ctx.bern_extrema(c[i:i + 1])
        for k in keys:
            assert np.array_equal(_bits(one[k]), _bits(g[k][i:i + 1])), (k, i)
        assert one["nodes"][0] == g["nodes"][i] and one["status"][0] == g["status"][i]
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        dc = torch.from_numpy(c).to(dev)
        dv, dt, db = (torch.empty(5000, dtype=torch.float64, device=dev) for _ in range(3))
        dn, ds = (torch.empty(5000, dtype=torch.int32, device=dev) for _ in range(2))
        ctx.bern_extrema_dev(dc.data_ptr(), 5000, K, dv.data_ptr(), dt.data_ptr(), db.data_ptr(), dn.data_ptr(), ds.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    for k, d in zip(keys, (dv, dt, db)):
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(g[k])), k
    assert np.array_equal(dn.cpu().numpy(), g["nodes"]) and np.array_equal(ds.cpu().numpy(), g["status"])


def _swarm(N, dim, deg, M, seed):
    """N vehicles inside one box.  Vehicle 1 flies vehicle 0's path backwards, a little to the side: the two are far apart at
    both ends and pass each other in between, so pair (0, 1) has its minimum separation -- and its smallest coefficient --
    inside; vehicle 2 starts far off and flies away, so its pairs are closest at an end (both asserted by the test)."""
    from optimalbeziertrajectorygeneration_amd import synth
    rng = np.random.default_rng(seed)
    Y = (synth.swarm_control_points(N, dim, deg, seed=seed, noise=25.0) - 50.0) * 0.2
    line = np.linspace(-9.0, 9.0, deg + 1)
    Y[0:dim] = rng.normal(0.0, 0.3, (dim, deg + 1)); Y[0] += line
    Y[dim:2 * dim] = rng.normal(0.0, 0.3, (dim, deg + 1)); Y[dim] -= line; Y[dim + 1] += 0.7
    Y[2 * dim:3 * dim] = rng.normal(0.0, 0.3, (dim, deg + 1)); Y[2 * dim] += np.linspace(40.0, 90.0, deg + 1)   # vehicle 2 leaves: closest at t = 0
    obs = rng.uniform(-8.0, 8.0, (M, dim)) if M else None
    return Y, obs


@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("deg", [3, 5, 8, 10, 15, 20, 7])
def test_temporal_sep_true_min(deg, dim, M):
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    N, max_sep = 3, 0.9
    Y, obs = _swarm(N, dim, deg, M, seed=10 * deg + dim + M)
    P, L = (N + M) * (N + M - 1) // 2, 2 * deg + 1
    c0 = _capi.Context(N, dim, deg, 0, point_obs=obs, device=0)
    try:
        for B in (1, 40):
            Yb = synth.fd_batch(Y, B=B) if B > 1 else Y[None].copy()
            g = c0.temporal_sep_true_min(Yb, max_sep, eps_rel=RTOL)
            assert g["val"].shape == (B, P) and (g["status"] == _capi.MD_OK).all()
            rows = c0.temporal_sep(Yb, max_sep).reshape(B * P, L)
            # fused = unfused, bit for bit
            u = c0.bern_extrema(rows, eps_rel=RTOL)
            assert np.array_equal(_bits(g["val"]).ravel(), _bits(u["val"])), "fused value != bern_extrema of the R = 0 rows"
            assert np.array_equal(_bits(g["t_star"]).ravel(), _bits(u["t_star"])) and np.array_equal(g["status"].ravel(), u["status"])
            # end-minimum pairs: the bits of the R = 0 control-point minimum
            mn0 = c0.temporal_sep_min(Yb, max_sep).ravel()
            am = rows.argmin(axis=1)
            ends = (rows[:, 0] == rows.min(axis=1)) | (rows[:, -1] == rows.min(axis=1))
            assert np.array_equal(_bits(g["val"]).ravel()[ends], _bits(mn0)[ends]), (am[ends])
            assert (~ends).any(), "no pair of this case reaches the search"
            assert ends.any(), "no pair of this case ends at an end coefficient"
            assert (u["nodes"][~ends] >= 1).all() and (u["nodes"] > 1).any(), "no pair of this case is subdivided"
            # the yardstick on the oracle's polynomials (separation_coeffs), bounds as for the random rows: r = 1e-12 s, tol = eps_rel s
            worst = 0.0
            for b in range(B):
                yfull = Yb[b] if obs is None else np.vstack([Yb[b], np.repeat(obs.reshape(-1, 1), deg + 1, axis=1)])
                co = R.separation_coeffs(yfull, N + M, dim, max_sep)
                worst = max(worst, float((np.abs(co - rows[b * P:(b + 1) * P]).max(axis=1) / np.abs(co).max(axis=1)).max()))
                for p in range(P):
                    _hold(co[p], g["val"][b, p], g["t_star"][b, p], None, RTOL, False,
                          "deg %d dim %d M %d row %d pair %d" % (deg, dim, M, b, p))
            print("deg %d dim %d M %d B %d: largest |device row - oracle row| / s = %.3e" % (deg, dim, M, B, worst))
            # never below the control-point bound, whatever the elevation
            for Rr in (0, 10, 100):
                c0.set_deg_elev(Rr)
                lo = c0.temporal_sep_min(Yb, max_sep)
                again = c0.temporal_sep_true_min(Yb, max_sep, eps_rel=RTOL)
                assert np.array_equal(_bits(again["val"]), _bits(g["val"])), "DEG_ELEV must not enter (R = %d)" % Rr
                sc = np.abs(rows).max(axis=1).reshape(B, P)
                assert (g["val"] >= lo - 1e-12 * sc).all(), Rr
            c0.set_deg_elev(0)
            # _dev = host
            dev = torch.device("cuda", 0)
            c0.set_stream(torch.cuda.current_stream().cuda_stream)
            try:
                dY = torch.from_numpy(np.ascontiguousarray(Yb)).to(dev)
                dv, dt = torch.empty((B, P), dtype=torch.float64, device=dev), torch.empty((B, P), dtype=torch.float64, device=dev)
                ds = torch.empty((B, P), dtype=torch.int32, device=dev)
                c0.temporal_sep_true_min_dev(dY.data_ptr(), B, max_sep, dv.data_ptr(), dt.data_ptr(), ds.data_ptr(), eps_rel=RTOL)
                torch.cuda.synchronize()
            finally:
                c0.use_own_stream()
            assert np.array_equal(_bits(dv.cpu().numpy()), _bits(g["val"])) and np.array_equal(_bits(dt.cpu().numpy()), _bits(g["t_star"]))
            assert np.array_equal(ds.cpu().numpy(), g["status"])
    finally:
        c0.close()


def test_bezier_min_max():
    from optimalbeziertrajectorygeneration_amd.bezier import Bezier
    c6 = Bezier(np.array(C6, dtype=float))
    lo, hi = c6.min(dim=1), c6.max(dim=1)
    assert type(lo) is float and type(hi) is float
    ymin, ymax = R.certified_min(C6[1]), R.certified_max(C6[1])
    assert abs(lo - float(ymin["H"])) <= 1e-6 and abs(lo - C6_MIN) <= 1e-6
    assert abs(hi - float(ymax["L"])) <= 1e-6 and abs(hi - C6_MAX) <= 1e-6
    assert c6.min() == 0.0 and c6.max() == 5.0                       # default dim 0: a line, the ends
    assert c6.min(1, -np.inf, 1e-6) == lo and c6.max(1, np.inf, 1e-6) == hi      # the reference's positional signature
    one = Bezier(np.array([[1.0, -2.0, 3.0, 0.5]]))
    y = R.certified_min([1.0, -2.0, 3.0, 0.5])
    assert float(y["L"]) - 1e-12 <= one.min() <= float(y["H"]) + 1e-6
    with pytest.raises(IndexError):
        c6.min(dim=2)
    with pytest.raises(IndexError):
        one.max(dim=1)


def _crossing(rows):
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=1.0,
                           initPoints=[(0.0, 0.0), (0.0, 4.0)], finalPoints=[(6.0, 4.0), (6.0, 0.0)], tf=1.0, separationRows=rows)


def test_true_min_rows_in_bezoptimization():
    import scipy.optimize as sop
    from scipy.optimize._numdiff import approx_derivative
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    assert int(opt.DEG_ELEV) == 0
    with pytest.raises(ValueError):
        _crossing('nearly')
    bo = BezOptimization(numVeh=3, dimension=2, degree=5, maxSep=0.8, initPoints=[(0, 0), (1, 5), (9, 2)],
                         finalPoints=[(10, 1), (8, 8), (0, 7)], tf=1.0, separationRows='true_min')
    x = bo.generateGuess(std=0.6, seed=4)
    f = bo.temporalSeparationConstraints
    v = f(x)
    direct = bo._ctx(False).temporal_sep_true_min(bo.reshapeVector(x)[None], 0.8, eps_rel=bo.TRUE_MIN_EPS_REL)["val"][0]
    assert np.array_equal(_bits(bo.trueMinSeparation(x)[0]), _bits(direct))
    assert v.shape == (3,) and np.array_equal(_bits(v), _bits(direct))
    # SciPy's own forward differences: served from one batch, identical to one-row calls
    bo.fdBatchingStats.update(batches=0, served=0, direct=0)
    J = approx_derivative(f, x, method='2-point', abs_step=opt.FD_STEP)
    assert bo.fdBatchingStats['batches'] >= 1 and bo.fdBatchingStats['served'] >= x.size - 1
    plain = BezOptimization(numVeh=3, dimension=2, degree=5, maxSep=0.8, initPoints=[(0, 0), (1, 5), (9, 2)],
                            finalPoints=[(10, 1), (8, 8), (0, 7)], tf=1.0, separationRows='true_min', fdBatching=False)
    g = plain.temporalSeparationConstraints
    Jp = approx_derivative(g, x, method='2-point', abs_step=opt.FD_STEP)
    assert np.array_equal(_bits(J), _bits(Jp))
    for k in (0, 3, x.size - 1):
        xk = x.copy(); xk[k] += opt.FD_STEP
        assert np.array_equal(_bits(g(xk)), _bits(bo._fd_values(x, 'tsep')[0][k + 1]))
    Jf = bo.temporalSeparationJacobian(x, method='fd')
    F = bo._fd_values(x, 'tsep')
    assert Jf.shape == (3, x.size) and np.array_equal(_bits(Jf), _bits(((F[0][1:] - F[0][0:1]) / F[1][:, None]).T))
    with pytest.raises(ValueError, match="true_min"):
        bo.temporalSeparationJacobian(x, method='exact')
    # one solve of a two-vehicle crossing at DEG_ELEV = 0: feasibility by the yardstick, not by SLSQP's flag
    cr = _crossing('true_min')
    cons = [{'type': 'ineq', 'fun': cr.temporalSeparationConstraints, 'jac': cr.temporalSeparationJacobian}]
    res = sop.minimize(cr.objectiveFunction, x0=cr.generateGuess(std=0.3, seed=2), method='SLSQP', constraints=cons,
                       options={'maxiter': 300, 'ftol': 1e-12, 'disp': False})
    co = R.separation_coeffs(cr.reshapeVector(res.x), 2, 2, 1.0)
    for p in range(co.shape[0]):
        y = R.certified_min(co[p])
        print("crossing: pair %d true minimum in [%.6e, %.6e], SLSQP status %d" % (p, float(y["L"]), float(y["H"]), res.status))
        assert float(y["L"]) >= -1e-9 * float(y["s"])
