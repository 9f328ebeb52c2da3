"""The true jerk rows and their envelope Jacobian on the device (obtg_jerk_true_min[_jac], BezOptimization(maxJerk=..,
jerkRows='true_min'), maxJerkJacobian(method='envelope'), trueJerkMax) against the exact-rational yardstick of
tests/jerk_envelope_ref.py.  Every device case is N = 4 vehicles, B = 5 rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import jerk_envelope_ref as S  # noqa: E402
import test_jerk_envelope_ref as T  # noqa: E402
from util import RTOL, assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

N, B = 4, 5
TF = np.array([1.0, 2.5, 1.0, 2.5, 1.0])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _batch(deg, dim):
    from optimalbeziertrajectorygeneration_amd import synth
    return synth.fd_batch(T._vehicles(deg, dim, T.seed_of(deg, dim)), B=B)


def _hold_blocks(g, Yb, dim, tf, what):
    """every vehicle's block within RTOL of its own largest yardstick entry, d/dtf within RTOL of itself, at the device's t_star"""
    worst = 0.0
    for b in range(Yb.shape[0]):
        blk, dtf = S.envelope_blocks(Yb[b], dim, tf[b], g["t_star"][b])
        for v in range(blk.shape[0]):
            w = "%s row %d vehicle %d" % (what, b, v)
            if not blk[v].any():
                assert not g["jac"][b, v].any(), w + ": a zero block"
            else:
                worst = max(worst, assert_close(g["jac"][b, v], blk[v], what=w))
            worst = max(worst, assert_close(g["jac_tf"][b, v:v + 1], dtf[v:v + 1], what=w + " d/dtf"))
    return worst


@pytest.mark.parametrize("dim", T.DIMS)
@pytest.mark.parametrize("deg", T.FAST + T.SLOW)
def test_bits_and_blocks(deg, dim):
    """(1) val, t_star, status of the _jac call are the bits of the value call, and both the bits of obtg_bern_extrema on
    obtg_jerk's rows of a DEG_ELEV = 0 context (the context under test has DEG_ELEV = 2: it does not enter); (2) val
    against the yardstick's bracket [L, H] of the oracle's row: L - r <= val <= H + RTOL s + r, s the row's largest
    coefficient, r = 1e-12 s for the rounding of the coefficients (device and oracle form them in different orders; the
    allowance of test_gpu_extrema._hold); (3) blocks and d/dtf against the yardstick at the device's own t_star, end
    minima with exactly four non-zero columns; (4) a row alone = the row in the batch, _dev = host, nullable outputs;
    (5) one launch where obtg_fast_kernels & 1, three otherwise.
    Degree 4: a quartic's row is concave (test_jerk_envelope_ref.test_shared_inputs_hold_interior_and_end_minima), every
    minimum is at an end; every other degree must hold both kinds."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    bound = T.BOUND
    Yb = _batch(deg, dim)
    fused = deg in T.FAST
    assert bool(_capi.fast_kernels(dim, deg) & 1) == fused
    ctx, ctx0 = _capi.Context(N, dim, deg, 2, device=0), _capi.Context(N, dim, deg, 0, device=0)
    try:
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        g = ctx.jerk_true_min_jac(Yb, TF, bound, eps_rel=RTOL)
        stats = ctx.kernel_stats()
        ctx.set_profiling(False)
        assert stats["speed"][1] == (1 if fused else 3) and sum(n for _, n in stats.values()) == stats["speed"][1], stats
        v = ctx.jerk_true_min(Yb, TF, bound, eps_rel=RTOL)
        assert g["jac"].shape == (B, N, dim, deg + 1) and g["jac_tf"].shape == (B, N) and ctx.deg_elev == 2
        rows = ctx0.jerk(Yb, TF, bound).reshape(B * N, 2 * deg + 1)
        e = ctx.bern_extrema(rows, eps_rel=RTOL, eps_abs=0.0)
        for k in ("val", "t_star"):
            assert np.array_equal(_bits(g[k]), _bits(v[k])), k
            assert np.array_equal(_bits(v[k]).ravel(), _bits(e[k])), k + " against obtg_bern_extrema of obtg_jerk's rows"
        assert np.array_equal(g["status"], v["status"]) and np.array_equal(v["status"].ravel(), e["status"])
        assert (g["status"] == _capi.MD_OK).all()
        for b in range(B):
            for vv, y in enumerate(S.true_rows(Yb[b], dim, TF[b], bound)):
                s = float(y["s"])
                r = 1e-12 * s
                assert float(y["L"]) - r <= g["val"][b, vv] <= float(y["H"]) + RTOL * s + r, (b, vv)
        worst = _hold_blocks(g, Yb, dim, TF, "deg %d dim %d" % (deg, dim))
        print("deg %d dim %d: largest scaled |device - yardstick| = %.3e" % (deg, dim, worst))
        inside = (g["t_star"] > 0.0) & (g["t_star"] < 1.0)
        if deg == 4:
            assert not inside.any(), "a quartic's jerk row is concave: every minimum is at an end"
        else:
            assert inside.any() and (~inside).any(), "the case must hold interior and end minima"
        for b in range(B):
            for vv in range(N):
                blk, t = g["jac"][b, vv], g["t_star"][b, vv]
                if t in (0.0, 1.0):
                    keep = [0, 1, 2, 3] if t == 0.0 else [deg - 3, deg - 2, deg - 1, deg]
                    assert (np.delete(blk, keep, axis=1) == 0.0).all() and (blk[:, keep] != 0.0).any(axis=0).all(), (b, vv, t)
        # a row alone: the bits it has inside the batch
        for b in (0, 3):
            one = ctx.jerk_true_min_jac(Yb[b:b + 1], TF[b:b + 1], bound, eps_rel=RTOL)
            for k in ("val", "t_star", "jac", "jac_tf"):
                assert np.array_equal(_bits(one[k][0]), _bits(g[k][b])), (k, b)
        # _dev = host
        dev = torch.device("cuda", 0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dY, dtf = torch.from_numpy(np.ascontiguousarray(Yb)).to(dev), torch.from_numpy(TF).to(dev)
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
            dv, dt, dg, dj = f64(B, N), f64(B, N), f64(B, N), f64(B, N, dim, deg + 1)
            ds = torch.empty((B, N), dtype=torch.int32, device=dev)
            ctx.jerk_true_min_jac_dev(dY.data_ptr(), dtf.data_ptr(), B, bound, dv.data_ptr(), dj.data_ptr(), dg.data_ptr(),
                                       dt.data_ptr(), ds.data_ptr(), eps_rel=RTOL)
            dv2, dj2 = f64(B, N), f64(B, N, dim, deg + 1)           # t_star, status and jac_tf are nullable
            ctx.jerk_true_min_jac_dev(dY.data_ptr(), dtf.data_ptr(), B, bound, dv2.data_ptr(), dj2.data_ptr(), eps_rel=RTOL)
            dv3, dt3 = f64(B, N), f64(B, N)
            ds3 = torch.empty((B, N), dtype=torch.int32, device=dev)
            ctx.jerk_true_min_dev(dY.data_ptr(), dtf.data_ptr(), B, bound, dv3.data_ptr(), dt3.data_ptr(), ds3.data_ptr(), eps_rel=RTOL)
            dv4 = f64(B, N)
            ctx.jerk_true_min_dev(dY.data_ptr(), dtf.data_ptr(), B, bound, dv4.data_ptr(), eps_rel=RTOL)
            torch.cuda.synchronize()
        finally:
            ctx.use_own_stream()
        for got, k in ((dv, "val"), (dv2, "val"), (dv3, "val"), (dv4, "val"), (dt, "t_star"), (dt3, "t_star"), (dg, "jac_tf"),
                       (dj, "jac"), (dj2, "jac")):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(g[k])), k
        assert np.array_equal(ds.cpu().numpy(), g["status"]) and np.array_equal(ds3.cpu().numpy(), g["status"])
    finally:
        ctx.close()
        ctx0.close()


@pytest.mark.parametrize("dim", T.DIMS)
@pytest.mark.parametrize("deg", [5, 10, 20])
def test_fused_and_two_launch_forms_give_the_same_bits(deg, dim, monkeypatch):
    from optimalbeziertrajectorygeneration_amd import _capi
    Yb = _batch(deg, dim)
    got, launches = [], []
    for fused in (True, False):
        if not fused:
            monkeypatch.setenv("OBTG_TRUE_MIN_JAC_FUSED", "0")
        c = _capi.Context(N, dim, deg, 0, device=0)
        try:
            c.set_profiling(True)
            c.reset_kernel_stats()
            got.append(c.jerk_true_min_jac(Yb, TF, T.BOUND, eps_rel=1e-12))
            launches.append(c.kernel_stats()["speed"][1])
        finally:
            c.close()
    monkeypatch.delenv("OBTG_TRUE_MIN_JAC_FUSED")
    assert launches == [1, 2], launches
    a, b = got
    for k in ("val", "t_star", "jac", "jac_tf"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["status"], b["status"])


@pytest.mark.parametrize("deg", [5, 6])
def test_edge_rows(deg):
    """A vehicle at rest: zero rows, val = bound**2 bit for bit, a block of zeros.  A cubic (elevated to the context's
    degree): a constant jerk 6 e / T^3, val = bound**2 - (d/2)(6 e / T^3)^2 within RTOL of the row's scale wherever the search
    puts t_star in [0, 1], and the yardstick's block there.  A NaN control point: NaN val, t_star, block and d/dtf, status OK.
    max_nodes = 3 on interior minima: NODE_CAP, val still an upper bound of the minimum (not below the yardstick's lower
    bound), a finite block that is the yardstick's at the returned t_star."""
    from optimalbeziertrajectorygeneration_amd import _capi
    dim = 2
    Y = T._vehicles(deg, dim, T.seed_of(deg, dim))
    tf = np.array([2.5])
    bound = T.BOUND
    c = _capi.Context(N, dim, deg, 0, device=0)
    try:
        Yr = Y.copy()
        i = np.arange(deg + 1)
        # a + b i/n + c i(i-1)/(n(n-1)) + e i(i-1)(i-2)/(n(n-1)(n-2)): the cubic a + b t + c t^2 + e t^3 at degree n
        cub = np.array([[1.0, 3.0, -4.5, 2.5], [-2.0, 0.5, 2.25, -3.75]])
        Yr[1 * dim:2 * dim] = (cub[:, :1] + cub[:, 1:2] * i / deg + cub[:, 2:3] * (i * (i - 1)) / (deg * (deg - 1))
                               + cub[:, 3:4] * (i * (i - 1) * (i - 2)) / (deg * (deg - 1) * (deg - 2)))
        Yr[2 * dim:3 * dim] = np.array([[1.25], [-3.5]])          # vehicle 2 at rest
        Yr[3 * dim, 2] = np.nan                                    # vehicle 3: a NaN control point
        g = c.jerk_true_min_jac(Yr[None], tf, bound, eps_rel=RTOL)
        v = c.jerk_true_min(Yr[None], tf, bound, eps_rel=RTOL)
        assert (g["status"] == _capi.MD_OK).all()
        assert np.array_equal(_bits(g["val"]), _bits(v["val"])) and np.array_equal(_bits(g["t_star"]), _bits(v["t_star"]))
        assert np.array_equal(_bits(g["val"][0, 2]), _bits(np.float64(bound ** 2))) and g["t_star"][0, 2] == 0.0
        assert (g["jac"][0, 2] == 0.0).all() and g["jac_tf"][0, 2] == 0.0
        acc = 6.0 * cub[:, 3] / tf[0] ** 3
        want = bound ** 2 - 0.5 * dim * float((acc * acc).sum())
        assert abs(g["val"][0, 1] - want) <= RTOL * max(bound ** 2, abs(want)) and 0.0 <= g["t_star"][0, 1] <= 1.0
        assert np.isnan(g["val"][0, 3]) and np.isnan(g["t_star"][0, 3]) and np.isnan(g["jac"][0, 3]).all() and np.isnan(g["jac_tf"][0, 3])
        assert np.isfinite(g["val"][0, :2]).all() and np.isfinite(g["jac"][0, :2]).all() and np.isfinite(g["jac_tf"][0, :2]).all()
        keep = {k: a[:, :3] for k, a in g.items()}
        _hold_blocks(keep, Yr[None, :3 * dim], dim, tf, "rest and constant jerk")
        g = c.jerk_true_min_jac(Y[None], tf, bound, eps_rel=1e-14, max_nodes=3)
        v = c.jerk_true_min(Y[None], tf, bound, eps_rel=1e-14, max_nodes=3)
        assert (g["status"] == _capi.MD_NODE_CAP).any() and np.array_equal(g["status"], v["status"])
        assert np.array_equal(_bits(g["val"]), _bits(v["val"])) and np.array_equal(_bits(g["t_star"]), _bits(v["t_star"]))
        for vv, y in enumerate(S.true_rows(Y, dim, tf[0], bound)):
            assert g["val"][0, vv] >= float(y["L"]) - 1e-12 * float(y["s"]), vv
        assert np.isfinite(g["jac"]).all() and np.isfinite(g["jac_tf"]).all()
        _hold_blocks(g, Y[None], dim, tf, "node cap")
        with pytest.raises(_capi.ObtgError) as err:                   # a null `out`
            c._check(c._lib.obtg_jerk_true_min(c._h, _capi._ptr(Y), _capi._ptr(tf), 1, 1.0, 1e-9, 100, None, None, None), "null out")
        assert err.value.code == -1
    finally:
        c.close()
    big = _capi.Context(1, 2, 32, 0, device=0)
    try:
        with pytest.raises(_capi.ObtgError) as err:
            big.jerk_true_min(np.zeros((1, 2, 33)), 1.0, 1.0)
        assert err.value.code == _capi.ERR_UNSUPPORTED
        with pytest.raises(_capi.ObtgError) as err:
            big.jerk_true_min_jac(np.zeros((1, 2, 33)), 1.0, 1.0)
        assert err.value.code == _capi.ERR_UNSUPPORTED
    finally:
        big.close()


@pytest.mark.parametrize("dim", T.DIMS)
def test_degrees_one_two_three(dim):
    """Degree 1: the second pass is exactly zero -- val = bound**2 bit for bit, a zero block, jac_tf 0.  Degree 2: no jerk, but
    three rounded passes need not cancel -- |val - bound^2| <= RTOL bound^2, and the block, which is formed from an empty basis,
    is zero.  Degree 3: a constant jerk -- val = bound^2 - (d/2)|6 (P3 - 3 P2 + 3 P1 - P0) / T^3|^2 within RTOL of the row's
    scale, t_star anywhere in [0, 1], and the block the yardstick's (the same at every t)."""
    from optimalbeziertrajectorygeneration_amd import _capi
    bound, tf = T.BOUND, np.array([2.5])
    for deg in (1, 2, 3):
        Y = T._vehicles(deg, dim, T.seed_of(deg, dim))
        c = _capi.Context(N, dim, deg, 0, device=0)
        try:
            g = c.jerk_true_min_jac(Y[None], tf, bound, eps_rel=RTOL)
        finally:
            c.close()
        assert (g["status"] == _capi.MD_OK).all() and ((g["t_star"] >= 0.0) & (g["t_star"] <= 1.0)).all(), deg
        if deg == 1:
            assert np.array_equal(_bits(g["val"]), _bits(np.full((1, N), bound ** 2)))
        if deg <= 2:
            assert (np.abs(g["val"] - bound ** 2) <= RTOL * bound ** 2).all(), deg
            assert (g["jac"] == 0.0).all() and (g["jac_tf"] == 0.0).all(), deg
        else:
            for v in range(N):
                want = float(S.offset(bound) + S.row_minus_offset(Y[v * dim:(v + 1) * dim], tf[0], 0.5))
                assert abs(g["val"][0, v] - want) <= RTOL * max(bound ** 2, abs(want)), v
            _hold_blocks(g, Y[None], dim, tf, "degree 3 dim %d" % dim)
            assert g["jac"].any()


# ------------------------------------------------------------------ BezOptimization
MAX_JERK = 3.0


def _dubins(**kw):
    """time-optimal, speeds prescribed: tf moves columns 1 and -2 of every vehicle"""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    kw.setdefault('maxJerk', MAX_JERK)
    return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, minSpeed=0.2, maxAngRate=1,
                           initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)], initSpeeds=[1, 1], finalSpeeds=[1, 1],
                           initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], **kw)


def _space(**kw):
    """3-D, fixed tf, degree 6 (off the fast-kernel list)"""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    kw.setdefault('maxJerk', MAX_JERK)
    return BezOptimization(numVeh=3, dimension=3, degree=6, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=3, minSpeed=0.1, tf=6.0,
                           initPoints=[(0, 0, 0), (3, 0, 1), (6, 0.5, 2)], finalPoints=[(6, 6, 2), (0, 6.5, 1), (3, 6, 0)], **kw)


PROBLEMS = {"dubins": (_dubins, 7), "space": (_space, 4)}


def _x0(make, seed, **kw):
    bo = make(**kw)
    x = bo.generateGuess(std=0.3, seed=seed)
    if bo._timeopt():
        x[-1] = 9.0
    return bo, x


def bo_step():
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    return opt.FD_STEP


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_closures_and_providers(name):
    make, seed = PROBLEMS[name]
    bo, x = _x0(make, seed, jerkRows='true_min')
    ba, _ = _x0(make, seed)
    Nv, dim, deg = bo.model['numVeh'], bo.model['dim'], bo.model['deg']
    ctx = bo._ctx(False)
    first, cols = bo._rv_parts()[1], bo._numCols
    D = bo._dY_dtf() if bo._timeopt() else None
    # the closures: the raw calls bit for bit, N (2n+1) control points or N true minima
    raw = ctx.jerk_true_min(bo.reshapeVector(x)[None], bo._tf_of(x), MAX_JERK, eps_rel=bo.TRUE_MIN_EPS_REL)
    rows = bo.maxJerkConstraints(x)
    assert rows.shape == (Nv,) and np.array_equal(_bits(rows), _bits(raw["val"][0]))
    rows_a = ba.maxJerkConstraints(x)
    assert rows_a.shape == (Nv * (2 * deg + 1),)
    assert np.array_equal(_bits(rows_a), _bits(ba._ctx(False).jerk(ba.reshapeVector(x), ba._tf_of(x), MAX_JERK)[0]))
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    assert np.array_equal(_bits(rows_a), _bits(opt._maxJerkConstraints(ba.reshapeVector(x), Nv, dim, ba._tf_of(x), MAX_JERK)))
    assert (rows >= rows_a.reshape(Nv, -1).min(axis=1) - 1e-9 * np.abs(rows_a).max()).all(), "the control points bound the row from below"
    # SciPy's forward differences: served from one batch, identical to direct calls -- both forms of the rows
    for b_, kw in ((bo, dict(jerkRows='true_min')), (ba, {})):
        plain = make(fdBatching=False, **kw)
        before = dict(b_.fdBatchingStats)
        closure, direct = b_.maxJerkConstraints, plain.maxJerkConstraints
        closure(x)
        for k in range(x.size):
            xk = x.copy()
            xk[k] += bo_step()
            assert np.array_equal(_bits(closure(xk)), _bits(direct(xk))), (kw, k)
        assert b_.fdBatchingStats['served'] - before['served'] == x.size and b_.fdBatchingStats['batches'] - before['batches'] == 1
    # the control-point rows: structured and brute-force finite differences, bit for bit
    Js, Jb = ba.maxJerkJacobian(x, structured=True), ba.maxJerkJacobian(x, structured=False)
    assert Js.shape == (Nv * (2 * deg + 1), x.size) and np.array_equal(_bits(Js), _bits(Jb)) and np.abs(Js).max() > 0
    # the envelope provider: dense [N][n_x], free columns of the vehicle's own block, the tf column with the dY/dtf chain
    J = bo.maxJerkJacobian(x, method='envelope')
    assert J.shape == (Nv, x.size) and np.isfinite(J).all()
    r = ctx.jerk_true_min_jac(bo.reshapeVectors(x[None]), float(bo._tf_of(x)), MAX_JERK, eps_rel=bo.TRUE_MIN_EPS_REL)
    assert np.array_equal(_bits(r["val"]), _bits(raw["val"]))
    blk, dtf = S.envelope_blocks(bo.reshapeVector(x), dim, float(bo._tf_of(x)), r["t_star"][0])
    want = S.scatter(blk, dtf, Nv, dim, first, cols, D)
    n_pts = Nv * dim * cols
    for v in range(Nv):
        assert_close(J[v, :n_pts], want[v, :n_pts], what="%s row %d" % (name, v))
    if D is not None:
        assert D.any() and J.shape[1] == n_pts + 1
        assert_close(J[:, -1], want[:, -1], what="%s tf column" % name)
        assert np.abs(want[:, -1] - dtf).max() > 1e-6 * np.abs(dtf).max(), "the dY/dtf chain must matter in this case"
    for b_ in (bo, ba):
        with pytest.raises(ValueError, match="envelope"):
            b_.maxJerkJacobian(x, method='exact')
    with pytest.raises(ValueError, match="true_min"):
        ba.maxJerkJacobian(x, method='envelope')
    unbounded = make(maxJerk=None)
    with pytest.raises(ValueError, match="maxJerk"):
        unbounded.maxJerkConstraints(x)
    with pytest.raises(ValueError, match="maxJerk"):
        unbounded.maxJerkJacobian(x)
    hi, t_hi = bo.trueJerkMax(x)
    hi_a, _ = ba.trueJerkMax(x)
    assert np.array_equal(_bits(hi), _bits(hi_a)), "whatever jerkRows is"
    for v, y in enumerate(S.true_rows(bo.reshapeVector(x), dim, float(bo._tf_of(x)), 0.0)):
        s = float(y["s"])
        assert float(-y["H"]) - 1e-11 * s <= hi[v] <= float(-y["L"]) + 1e-12 * s and 0.0 <= t_hi[v] <= 1.0


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_envelope_against_the_finite_difference_provider(name):
    """method='fd' (forward differences of the search itself, h = FD_STEP) against method='envelope', entry by entry.  The
    bound of a row is not fixed in advance: it is the yardstick's own largest |central difference of certified minima
    (step 2^-17, brackets 1e-20 s) - envelope entry at its own minimiser| on that row, plus the finite-difference provider's
    documented search slack TRUE_MIN_EPS_REL * s / FD_STEP, times 2 for the forward difference's curvature term -- derived as
    test_gpu_speed_true_min.test_envelope_against_the_finite_difference_provider derives its bound."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    make, seed = PROBLEMS[name]
    bo, x = _x0(make, seed, jerkRows='true_min')
    Je, Jf = bo.maxJerkJacobian(x, method='envelope'), bo.maxJerkJacobian(x, method='fd')
    assert Je.shape == Jf.shape == (bo.model['numVeh'], x.size)
    yard_gap, s = T.yardstick_gap(bo, x)
    bound = 2.0 * (yard_gap + bo.TRUE_MIN_EPS_REL * s / opt.FD_STEP)
    gap = np.abs(Je - Jf).max(axis=1)
    print("%s: largest |envelope - fd| per row" % name, gap, "bound", bound, "yardstick's own gap", yard_gap,
          "largest entry", np.abs(Je).max())
    assert (gap <= bound).all()


def test_solve_with_the_jerk_rows():
    """example17's two solves at ftol = 1e-10 -- the control-point rows from the straight-line guess, the true rows from that
    solve's solution, as the example runs them.  Asserted: the control-point solve converges; its final time is above the
    unbounded problem's 2.427643190; at both solutions the true maximum of (d/2)|j|^2 is at most (d/2) maxJerk^2 (1 + 1e-6)
    -- the slack is SLSQP's own constraint tolerance at that ftol, as in test_solve_with_the_true_speed_rows, not an allowance
    for the rows --; the true-row solve does not end above the first by more than 1e-8, and it converges too.
    Measured on the MI355X: tf 2.772558152 (19 iterations, status 0; the CPU rehearsal's figure, which took 22) and
    2.755968758 (236 iterations, status 0).  At the first solution vehicle 1's maximum is the end coefficient at t = 0
    (1.000000 of the bound: that row is tight), vehicle 0's true maximum is 0.9664 of the bound at t = 1; the true rows
    release the slack the control points leave inside the span and LOWER tf by 0.017: at the second solution the maxima are
    0.8620 (t = 0.826) and 1.000000 (t = 0.870, inside) of the bound."""
    import example17_jerk_bounds as ex
    bo_a, res_a = ex.solve('all', ftol=1e-10)
    bo_t, res_t = ex.solve('true_min', ftol=1e-10, x0=res_a.x)
    d = bo_t.model['dim']
    hi_a, hi_t = bo_a.trueJerkMax(res_a.x)[0], bo_t.trueJerkMax(res_t.x)[0]
    cap = 0.5 * d * ex.MAX_JERK ** 2
    print("tf with 'all' rows %.9f (%d iterations, status %d), with 'true_min' rows %.9f (%d iterations, status %d); true maximum "
          "of (d/2)|j|^2 over the bound: %s and %s" % (res_a.fun, res_a.nit, res_a.status, res_t.fun, res_t.nit, res_t.status,
                                                       hi_a / cap, hi_t / cap))
    assert res_a.success and res_t.success
    assert res_a.fun > ex.TF_UNBOUNDED
    assert (hi_a <= cap * (1.0 + 1e-6)).all() and (hi_t <= cap * (1.0 + 1e-6)).all()
    assert res_t.fun <= res_a.fun + 1e-8
    assert bo_t.maxJerkConstraints(res_t.x).shape == (2,) and bo_a.maxJerkConstraints(res_a.x).shape == (2 * 21,)
