"""The envelope Jacobian of the true-minimum separation rows on the device (obtg_temporal_sep_true_min_jac,
BezOptimization.temporalSeparationJacobian(method='envelope')) against the exact-rational yardstick of tests/envelope_ref.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envelope_ref as E  # noqa: E402
import extrema_ref as R  # noqa: E402
import test_envelope_ref as T  # noqa: E402
from util import RTOL, assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

FAST = (3, 5, 7, 10, 20)     # degrees with a fused kernel (control-point counts 4, 6, 8, 11, 21 of the fast-kernel list)
SLOW = (6, 13)               # degrees off that list (counts 7, 14): the value path, then the launch that forms the blocks


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _swarm(N, dim, deg, M, seed):
    """Vehicles 0 and 1 pass each other (minimum inside), vehicle 2 flies away (its pairs are closest at t = 0), M point obstacles"""
    from optimalbeziertrajectorygeneration_amd import synth
    rng = np.random.default_rng(seed)
    Y = (synth.swarm_control_points(N, dim, deg, seed=seed, noise=25.0) - 50.0) * 0.2
    line = np.linspace(-9.0, 9.0, deg + 1)
    Y[0:dim] = rng.normal(0.0, 0.3, (dim, deg + 1)); Y[0] += line
    Y[dim:2 * dim] = rng.normal(0.0, 0.3, (dim, deg + 1)); Y[dim] -= line; Y[dim + 1] += 0.7
    Y[2 * dim:3 * dim] = rng.normal(0.0, 0.3, (dim, deg + 1)); Y[2 * dim] += np.linspace(40.0, 90.0, deg + 1)
    obs = rng.uniform(-8.0, 8.0, (M, dim)) if M else None
    return Y, obs


def _yard(Yb, obs, dim, n_veh, t_star):
    """[B][P][dim][n + 1]: the yardstick's blocks at the given t_star[B][P]"""
    n_obj = n_veh + (0 if obs is None else len(obs))
    return np.stack([E.envelope_blocks(E.full_row(Yb[b], obs), dim, n_veh, n_obj, t_star[b]) for b in range(Yb.shape[0])])


def _hold_blocks(jac, ref, what):
    """every pair's block within 1e-9 of its own largest yardstick entry (all-zero blocks: exactly zero)"""
    worst = 0.0
    for b in range(ref.shape[0]):
        for p in range(ref.shape[1]):
            if not ref[b, p].any():
                assert not jac[b, p].any(), "%s row %d pair %d: a zero block" % (what, b, p)
            else:
                worst = max(worst, assert_close(jac[b, p], ref[b, p], what="%s row %d pair %d" % (what, b, p)))
    return worst


@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("deg", FAST + SLOW)
def test_blocks_search_and_bits(deg, dim, M):
    """(1) blocks against the yardstick at the device's own t_star, end minima and the obstacle-obstacle block included;
    (2) val, t_star, status are the bits of temporal_sep_true_min; (3) host = _dev, a row alone = the row in a batch."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    N, max_sep = 3, 0.9
    Y, obs = _swarm(N, dim, deg, M, seed=10 * deg + dim + M)
    P = (N + M) * (N + M - 1) // 2
    prs = E.pairs(N + M)
    c0 = _capi.Context(N, dim, deg, 0, point_obs=obs, device=0)
    try:
        assert bool(_capi.fast_kernels(dim, deg) & 1) == (deg in FAST)
        Yb = synth.fd_batch(Y, B=5)
        g = c0.temporal_sep_true_min_jac(Yb, max_sep, eps_rel=RTOL)
        v = c0.temporal_sep_true_min(Yb, max_sep, eps_rel=RTOL)
        assert g["jac"].shape == (5, P, dim, deg + 1) and (g["status"] == _capi.MD_OK).all()
        for k in ("val", "t_star"):
            assert np.array_equal(_bits(g[k]), _bits(v[k])), k
        assert np.array_equal(g["status"], v["status"])
        worst = _hold_blocks(g["jac"], _yard(Yb, obs, dim, N, g["t_star"]), "deg %d dim %d M %d" % (deg, dim, M))
        print("deg %d dim %d M %d: largest scaled |device - yardstick| = %.3e" % (deg, dim, M, worst))
        inside = (g["t_star"] > 0.0) & (g["t_star"] < 1.0)
        assert inside.any() and (~inside).any(), "the case must hold interior and end minima"
        for b in range(5):
            for p, (a, _) in enumerate(prs):
                blk, t = g["jac"][b, p], g["t_star"][b, p]
                if a >= N:
                    assert (blk == 0.0).all(), "obstacle against obstacle"
                elif t in (0.0, 1.0):
                    keep = 0 if t == 0.0 else deg
                    assert (np.delete(blk, keep, axis=1) == 0.0).all() and (blk[:, keep] != 0.0).any(), (b, p, t)
        if M:
            assert any(a >= N for a, _ in prs)
        # a row alone: the bits it has inside the batch
        for b in (0, 3):
            one = c0.temporal_sep_true_min_jac(Yb[b:b + 1], max_sep, eps_rel=RTOL)
            for k in ("val", "t_star", "jac"):
                assert np.array_equal(_bits(one[k][0]), _bits(g[k][b])), (k, b)
        # _dev = host
        dev = torch.device("cuda", 0)
        c0.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dY = torch.from_numpy(np.ascontiguousarray(Yb)).to(dev)
            dv, dt = torch.empty((5, P), dtype=torch.float64, device=dev), torch.empty((5, P), dtype=torch.float64, device=dev)
            ds = torch.empty((5, P), dtype=torch.int32, device=dev)
            dj = torch.empty((5, P, dim, deg + 1), dtype=torch.float64, device=dev)
            c0.temporal_sep_true_min_jac_dev(dY.data_ptr(), 5, max_sep, dv.data_ptr(), dj.data_ptr(), dt.data_ptr(), ds.data_ptr(),
                                             eps_rel=RTOL)
            torch.cuda.synchronize()
            dj2 = torch.empty_like(dj)           # t_star and status are nullable
            c0.temporal_sep_true_min_jac_dev(dY.data_ptr(), 5, max_sep, dv.data_ptr(), dj2.data_ptr(), eps_rel=RTOL)
            torch.cuda.synchronize()
        finally:
            c0.use_own_stream()
        assert np.array_equal(_bits(dj.cpu().numpy()), _bits(g["jac"])) and np.array_equal(_bits(dj2.cpu().numpy()), _bits(g["jac"]))
        assert np.array_equal(_bits(dv.cpu().numpy()), _bits(g["val"])) and np.array_equal(_bits(dt.cpu().numpy()), _bits(g["t_star"]))
        assert np.array_equal(ds.cpu().numpy(), g["status"])
    finally:
        c0.close()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("deg", [5, 10, 20])
def test_fused_and_two_launch_forms_give_the_same_bits(deg, dim, monkeypatch):
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    Y, obs = _swarm(3, dim, deg, 2, seed=3 * deg + dim)
    Yb = synth.fd_batch(Y, B=7)
    got, launches = [], []
    for fused in (True, False):
        if not fused:
            monkeypatch.setenv("OBTG_TRUE_MIN_JAC_FUSED", "0")
        c = _capi.Context(3, dim, deg, 0, point_obs=obs, device=0)
        try:
            c.set_profiling(True)
            c.reset_kernel_stats()
            got.append(c.temporal_sep_true_min_jac(Yb, 0.9, eps_rel=1e-12))
            launches.append(c.kernel_stats()["temporal_sep"][1])
        finally:
            c.close()
    monkeypatch.delenv("OBTG_TRUE_MIN_JAC_FUSED")
    assert launches == [1, 2], launches
    for k in ("val", "t_star", "jac"):
        assert np.array_equal(_bits(got[0][k]), _bits(got[1][k])), k
    assert np.array_equal(got[0]["status"], got[1]["status"])


@pytest.mark.parametrize("deg", [5, 6])
def test_edge_rows(deg):
    """A non-finite coefficient: NaN block, status OK.  A node budget too small: status NODE_CAP and the finite block that
    is the yardstick's at the returned t_star."""
    from optimalbeziertrajectorygeneration_amd import _capi
    dim, N = 2, 3
    Y, _ = _swarm(N, dim, deg, 0, seed=77 + deg)
    c = _capi.Context(N, dim, deg, 0, device=0)
    try:
        Yn = Y.copy()
        Yn[2 * dim, 2] = np.nan                       # vehicle 2: pairs (0, 2) and (1, 2)
        Yi = Y.copy()
        Yi[0, 1] = np.inf                             # vehicle 0: pairs (0, 1) and (0, 2)
        for Yq, bad in ((Yn, (1, 2)), (Yi, (0, 1))):
            g = c.temporal_sep_true_min_jac(Yq[None], 0.9, eps_rel=RTOL)
            v = c.temporal_sep_true_min(Yq[None], 0.9, eps_rel=RTOL)
            assert (g["status"] == _capi.MD_OK).all()
            assert np.array_equal(_bits(g["val"]), _bits(v["val"])) and np.array_equal(_bits(g["t_star"]), _bits(v["t_star"]))
            for p in range(3):
                assert np.isnan(g["val"][0, p]) == (p in bad)
                assert np.isnan(g["jac"][0, p]).all() if p in bad else np.isfinite(g["jac"][0, p]).all(), p
        g = c.temporal_sep_true_min_jac(Y[None], 0.9, eps_rel=1e-14, max_nodes=3)
        v = c.temporal_sep_true_min(Y[None], 0.9, eps_rel=1e-14, max_nodes=3)
        assert (g["status"] == _capi.MD_NODE_CAP).any() and np.array_equal(g["status"], v["status"])
        assert np.array_equal(_bits(g["val"]), _bits(v["val"])) and np.array_equal(_bits(g["t_star"]), _bits(v["t_star"]))
        assert np.isfinite(g["jac"]).all()
        _hold_blocks(g["jac"], _yard(Y[None], None, dim, N, g["t_star"]), "node cap")
    finally:
        c.close()


@pytest.mark.parametrize("deg,dim", [(5, 2), (10, 3), (6, 2)])
def test_contraction_identity(deg, dim):
    """jac = sum_k B_k^2n(t_star) J_k over obtg_temporal_sep_jac's blocks of an R = 0 context"""
    from fractions import Fraction
    from optimalbeziertrajectorygeneration_amd import _capi
    Y, obs = _swarm(3, dim, deg, 1, seed=5 * deg + dim)
    c = _capi.Context(3, dim, deg, 0, point_obs=obs, device=0)
    try:
        g = c.temporal_sep_true_min_jac(Y[None], 0.9, eps_rel=RTOL)
        J = c.temporal_sep_jac(Y[None])[0]                         # [P][2n + 1][dim][n + 1]
        for p in range(J.shape[0]):
            w = np.array([float(v) for v in E.basis(2 * deg, Fraction(float(g["t_star"][0, p])))])
            want = np.einsum('k,kci->ci', w, J[p])
            if want.any():
                assert_close(g["jac"][0, p], want, what="pair %d" % p)
            else:
                assert not g["jac"][0, p].any()
    finally:
        c.close()


def _dubins(**kw):
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=2, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, maxAngRate=1,
                           initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)], initSpeeds=[1, 1], finalSpeeds=[1, 1],
                           initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], **kw)


def _planar(rows, obs=None):
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=3, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=3, minSpeed=0.1,
                           maxAngRate=2, tf=6.0, initPoints=[(0, 0), (3, 0), (6, 0.5)], finalPoints=[(6, 6), (0, 6.5), (3, 6)],
                           pointObstacles=obs, separationRows=rows)


def test_provider():
    bo = _planar('true_min', obs=[[3.0, 3.0]])
    x = bo.generateGuess(std=0.3, seed=4)
    J = bo.temporalSeparationJacobian(x, method='envelope')
    assert J.shape == (6, x.size) and np.isfinite(J).all()
    assert np.array_equal(_bits(J), _bits(bo.trueMinSeparationJacobian(x)))
    ctx = bo._ctx(True)
    r = ctx.temporal_sep_true_min_jac(bo.reshapeVector(x)[None], 0.9, eps_rel=bo.TRUE_MIN_EPS_REL)
    assert np.array_equal(_bits(J), _bits(E.scatter(r["jac"][0], 3, 4, 2, 1, 4)))
    # one launch per call on a fast-list shape
    ctx.set_profiling(True)
    ctx.reset_kernel_stats()
    bo.temporalSeparationJacobian(x, method='envelope')
    stats = ctx.kernel_stats()
    ctx.set_profiling(False)
    assert stats["temporal_sep"][1] == 1 and sum(n for _, n in stats.values()) == 1, stats
    # every other row kind, and the per-vehicle providers
    for rows in ('all', 'min', 'active'):
        other = _planar(rows)
        with pytest.raises(ValueError, match=rows):
            other.temporalSeparationJacobian(x, method='envelope')
    for name in ('maxSpeedJacobian', 'minSpeedJacobian', 'maxAngularRateJacobian'):
        with pytest.raises(ValueError):
            getattr(bo, name)(x, method='envelope')
    with pytest.raises(ValueError, match="true_min"):
        bo.temporalSeparationJacobian(x, method='exact')
    # time-optimal with prescribed speeds: the tf column is the blocks along dY/dtf
    du = _dubins(separationRows='true_min')
    xd = du.generateGuess(std=0.3, seed=4)
    Jd = du.temporalSeparationJacobian(xd, method='envelope')
    assert Jd.shape == (1, xd.size)
    rd = du._ctx(False).temporal_sep_true_min_jac(du.reshapeVectors(xd[None]), 1, eps_rel=du.TRUE_MIN_EPS_REL)
    D = du._dY_dtf().reshape(2, 2, -1)
    assert D.any()
    want = float((rd["jac"][0, 0] * (D[0] - D[1])).sum())
    assert abs(Jd[0, -1] - want) <= 1e-12 * max(1.0, abs(want)), (Jd[0, -1], want)
    first, cols = du._rv_parts()[1], du._numCols
    assert np.array_equal(_bits(Jd[:, :-1]), _bits(E.scatter(rd["jac"][0], 2, 2, 2, first, cols)))


FD_GAP = 3.22e-9            # test_envelope_ref.test_fd_comparison_point_is_smooth_and_its_gap measures it on this x


def test_against_the_finite_difference_provider():
    """Three vehicles of test_true_min_rows_in_bezoptimization at generateGuess(std=0.6, seed=4).  Entries whose yardstick
    minimiser moves by more than 1e-3 between x and x + h e_k are left out (ties; none of the 72 on this x, at most 5 %
    allowed).  Bound per pair: 4 x 3.22e-9 -- the largest gap between the yardstick's envelope entries and central
    differences of its certified minima on this x, measured on the CPU -- plus the finite-difference provider's documented
    search slack eps_rel * s / h = 1e-12 s / 1.49e-8 = 6.7e-5 s (s = 52.4, 135.4, 72.4: 3.5e-3, 9.1e-3, 4.9e-3).
    Measured on the MI355X: 1.08e-6, 4.7e-7, 2.1e-7."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    bo, x = T._fd_problem()
    out = T.ties(bo, x, opt.FD_STEP)
    assert out.mean() <= T.MAX_LEFT_OUT
    Je = bo.temporalSeparationJacobian(x, method='envelope')
    Jf = bo.temporalSeparationJacobian(x, method='fd')
    assert Je.shape == Jf.shape == (3, x.size)
    s = np.array([float(r["s"]) for r in T.certified(bo, x)])
    bound = 4.0 * FD_GAP + bo.TRUE_MIN_EPS_REL * s / opt.FD_STEP
    gap = np.where(out, 0.0, np.abs(Je - Jf))
    print("largest |envelope - fd| per pair", gap.max(axis=1), "bound", bound, "left out", int(out.sum()))
    assert (gap <= bound[:, None]).all()


def _example10():
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=3, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=1.0, tf=10.0,
                           initPoints=[(0.0, 0.0), (0.0, 4.0), (3.0, -1.0)], finalPoints=[(6.0, 4.0), (6.0, 0.0), (3.0, 5.0)],
                           separationRows='true_min')


def _crossing():
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=1.0,
                           initPoints=[(0.0, 0.0), (0.0, 4.0)], finalPoints=[(6.0, 4.0), (6.0, 0.0)], tf=1.0, separationRows='true_min')


SOLVE_REL_GAP = 1e-6        # ten times the gap measured on the MI355X, not below 1e-6 (the docstring below has the figures)


@pytest.mark.parametrize("make,ftol", [(_crossing, 1e-12), (_example10, 1e-10)])
def test_solve_with_the_envelope_jacobian(make, ftol):
    """SLSQP with jac from method='envelope': every pair feasible by the yardstick, objective within SOLVE_REL_GAP of the
    method='fd' solve from the same start.  Measured relative gaps on the MI355X: 9.6e-15 (crossing: 14.422205101856 both ways)
    and 1.1e-13 (example10's swarm: 20.422205101881 / 20.422205101878); ten times that is below the floor of 1e-6, which holds."""
    import scipy.optimize as sop
    res = {}
    for method in ('envelope', 'fd'):
        bo = make()
        cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
                 'jac': lambda x, bo=bo, method=method: bo.temporalSeparationJacobian(x, method=method)}]
        res[method] = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0.3, seed=2), method='SLSQP', constraints=cons,
                                   options={'maxiter': 300, 'ftol': ftol, 'disp': False})
    n_obj = bo.model['numVeh']
    co = R.separation_coeffs(bo.reshapeVector(res['envelope'].x), n_obj, 2, 1.0)
    for p in range(co.shape[0]):
        y = R.certified_min(co[p])
        print("pair %d true minimum in [%.6e, %.6e]" % (p, float(y["L"]), float(y["H"])))
        assert float(y["L"]) >= -1e-9 * float(y["s"])
    fe, ff = res['envelope'].fun, res['fd'].fun
    gap = abs(fe - ff) / abs(ff)
    print("%s: objective %.12f (envelope, %d iterations) %.12f (fd, %d iterations): relative gap %.3e"
          % (make.__name__, fe, res['envelope'].nit, ff, res['fd'].nit, gap))
    assert gap <= SOLVE_REL_GAP
