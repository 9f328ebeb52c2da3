"""The space-curvature rows on the device (obtg_space_curvature_poly, obtg_space_curvature_true_min[_jac],
obtg_bern_space_curvature, Bezier.spaceCurvatureMax, BezOptimization(maxSpaceCurvature=...)) against the exact-rational
yardstick of tests/space_curvature_ref.py.

Shapes: N = 2 vehicles in space; degrees 3, 5, 7, 8, 10, 15 (every in-register instantiation), 1, 2, 4, 6, 31 (the workspace
form; 31: K = 63, the last lane and 65 280 bytes of frames), 32 (refused); B = 7 rows of 2 vehicles for the values -- 12
seeded curves per degree (3 at degree 31, where the rational search of one curve takes half a second) and the wide-speed
curve where the degree is 4 --, 65 and 129 items for the batches.  Regular inputs: curves of the seeded family on which the
YARDSTICK's search ends with at most 32 waiting and within max_nodes -- decided on the CPU before the device sees them.  Every
device status on them must be MD_OK.  Every bound is a majorant space_curvature_ref.py derives; none is a tuned number."""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curvature_ref as C  # noqa: E402
import space_curvature_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

N = 2
W = 0.5                   # max_curv
EPS = 1e-9
MAX_NODES = 100000
U = mpmath.mpf(2) ** -53
LISTED = (3, 5, 7, 8, 10, 15)            # degrees whose coefficients stay in registers
ERR_ARG, ERR_UNSUPPORTED = -1, -5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_CASES = {}


def cases(deg):
    """[dict(yv, co, ref)]: the degree's curves with the yardstick's coefficients and its certified search (the search that
    admitted the seed); computed once, shared, left unchanged"""
    if deg not in _CASES:
        out = []
        for yv, ref in S.regular_curves(deg, 3 if deg == 31 else 12, EPS, MAX_NODES, W):
            assert ref['waiting'] <= 32
            out.append(dict(yv=yv, co=S.coeffs(yv), ref=ref))
        if deg == 4:
            yv = S.as_floats(S.wide_speed())
            ref = S.certified_max(yv, W, Fraction(EPS), MAX_NODES)
            assert ref['status'] == 'ok' and ref['waiting'] <= 32
            den = S.coeffs(yv)[1]
            assert max(S._bern(den, Fraction(i, 64)) for i in range(65)) > 25 * min(S._bern(den, Fraction(i, 64)) for i in range(65))
            out.append(dict(yv=yv, co=S.coeffs(yv), ref=ref))
        _CASES[deg] = out
    return _CASES[deg]


def batch(deg, B):
    """Y[B][N * 3][deg + 1] and which[B][N]: vehicle v of row b is curve (N b + v) mod (number of curves)"""
    cs = cases(deg)
    which = np.array([[(N * b + v) % len(cs) for v in range(N)] for b in range(B)])
    return np.stack([np.concatenate([cs[i]['yv'] for i in row]) for row in which]), which


def _hold_value(what, yv, co, ref, out, t, eps=EPS, w=W):
    """lo - eps max(W, lo) - R_bound <= m_dev <= hi + R_point, and the value against the rational kappa at the device's own
    t_star; returns |device - yardstick| / majorant"""
    assert 0.0 <= t <= 1.0 and S.depth_of(t) <= 64, what
    m = Fraction(w) - Fraction(out)                      # the device's maximum, exactly as the row holds it
    K, M = S.kappa_majorant(yv, t, co=co)
    assert mpmath.isfinite(M), what
    r_point = (K + 1) * U * (M + w)
    r_bound = S.bound_majorant(yv, S.depth_of(t), co=co, points=17) + U * w
    want = w - S.kappa(yv, t)
    err = abs(mpmath.mpf(out) - want)
    assert err <= r_point, (what, float(err), float(r_point))
    lo, hi = ref['L'], ref['H']
    tol = Fraction(eps) * max(Fraction(w), lo)
    assert S._mp(lo) - S._mp(tol) - r_bound <= S._mp(m) <= S._mp(hi) + r_point, (what, float(m), float(lo), float(hi))
    return float(err / r_point)


def _hold_block(what, yv, t, jac):
    """a block against the exact rational gradient at the device's own t_star, within the derived majorant"""
    Kb, Mb = S.block_majorant(yv, t)
    blk = S.envelope_block(yv, t)
    worst = 0.0
    for cc in range(3):
        for i in range(jac.shape[1]):
            bound = mpmath.mpf("1.05") * Kb * U * Mb[cc][i]
            assert mpmath.isfinite(bound), what
            err = abs(mpmath.mpf(float(jac[cc, i])) - blk[cc][i])
            assert err <= bound, (what, cc, i, float(err), float(bound))
            if bound:
                worst = max(worst, float(err / bound))
    return worst


# 3, 5, 7, 8, 10, 15: every in-register instantiation; 1: w == 0 through the workspace form; 2: K = 5; 4, 6: the workspace form (4 with the wide-speed curve); 31: K = 63
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5, 6, 7, 8, 10, 15, 31])
def test_rows_against_the_yardstick(deg, monkeypatch):
    """values, t_star, the bracket, the coefficients and the blocks against the yardstick; the _jac call's out / t_star /
    status are the plain call's bits; the same curve elsewhere in the batch has the same bits; the two-launch form
    (OBTG_TRUE_MIN_JAC_FUSED=0) gives the fused form's bits; launches under OBTG_K_ANG_RATE: 1 in registers (2 with the
    blocks in their own launch), 2 / 3 through the workspace."""
    from optimalbeziertrajectorygeneration_amd import _capi
    cs = cases(deg)
    B = (len(cs) + N - 1) // N + 1
    Y, which = batch(deg, B)
    assert len(set(which.ravel())) == len(cs)
    ctx = _capi.Context(N, 3, deg, 0, device=0)
    try:
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        g = ctx.space_curvature_true_min_jac(Y, W, eps_rel=EPS, max_nodes=MAX_NODES)
        launches = [ctx.kernel_stats()["ang_rate"][1]]
        ctx.reset_kernel_stats()
        v = ctx.space_curvature_true_min(Y, W, eps_rel=EPS, max_nodes=MAX_NODES)
        stats = ctx.kernel_stats()
        launches.append(stats["ang_rate"][1])
        assert sum(n for _, n in stats.values()) == launches[1], stats
        ctx.set_profiling(False)
        assert launches == ([1, 1] if deg in LISTED else [3, 2]), launches
        assert g["val"].shape == (B, N) and g["jac"].shape == (B, N, 3, deg + 1)
        for k in ("val", "t_star"):
            assert np.array_equal(_bits(g[k]), _bits(v[k])), k
        assert np.array_equal(g["status"], v["status"])
        assert (g["status"] == _capi.MD_OK).all(), np.argwhere(g["status"] != _capi.MD_OK)
        rows = ctx.space_curvature_poly(Y)
        assert rows.shape == (B, N, 4, 2 * deg + 1)
        first, worst = {}, dict(val=0.0, coeff=0.0, block=0.0)
        for b in range(B):
            for vv in range(N):
                i = which[b, vv]
                if i in first:          # the same curve elsewhere in the batch: the same bits, whatever its position
                    b0, v0 = first[i]
                    for k in ("val", "t_star", "jac"):
                        assert np.array_equal(_bits(g[k][b, vv]), _bits(g[k][b0, v0])), (k, b, vv)
                    assert np.array_equal(_bits(rows[b, vv]), _bits(rows[b0, v0]))
                    continue
                first[i] = (b, vv)
                c = cs[i]
                what = "deg %d curve %d" % (deg, i)
                out, t = float(g["val"][b, vv]), float(g["t_star"][b, vv])
                worst["val"] = max(worst["val"], _hold_value(what, c['yv'], c['co'], c['ref'], out, t))
                if deg == 1:                                     # a straight path: the row IS max_curv, the block zero
                    assert out == W and t == 0.0 and not g["jac"][b, vv].any(), what
                else:
                    assert out < W                               # a curve of the family turns somewhere
                    worst["block"] = max(worst["block"], _hold_block(what, c['yv'], t, g["jac"][b, vv]))
                co = c['co']
                for part in range(4):
                    exact, mag = (co[0][part], co[2][part]) if part < 3 else (co[1], co[3])
                    for k in range(2 * deg + 1):
                        bound = S.coeff_count(deg) * S.UNIT * mag[k]
                        err = abs(Fraction(float(rows[b, vv, part, k])) - exact[k])
                        if bound:
                            worst["coeff"] = max(worst["coeff"], float(err / bound))
                        assert err <= bound, (what, part, k)
        print("deg %d: largest |device - yardstick| / majorant: value %.3g, coefficient %.3g, block entry %.3g"
              % (deg, worst["val"], worst["coeff"], worst["block"]))
        one = ctx.space_curvature_true_min_jac(Y[:1], W, eps_rel=EPS, max_nodes=MAX_NODES)
        for k in ("val", "t_star", "jac"):
            assert np.array_equal(_bits(one[k][0]), _bits(g[k][0])), k
    finally:
        ctx.close()
    monkeypatch.setenv("OBTG_TRUE_MIN_JAC_FUSED", "0")
    ctx = _capi.Context(N, 3, deg, 0, device=0)
    try:
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        two = ctx.space_curvature_true_min_jac(Y, W, eps_rel=EPS, max_nodes=MAX_NODES)
        assert ctx.kernel_stats()["ang_rate"][1] == (2 if deg in LISTED else 3)
        for k in ("val", "t_star", "jac"):
            assert np.array_equal(_bits(two[k]), _bits(g[k])), "two-launch form: " + k
        assert np.array_equal(two["status"], g["status"])
    finally:
        ctx.close()


def test_the_wide_speed_curve_at_three_tolerances():
    """space_curvature_ref.wide_speed() (degree 4: the workspace form; its control points padded into a degree-5 context are
    another curve, so the in-register form sees it through the free-curve call's twin below): den varies by more than 25 x,
    the +inf guard is what keeps the nodes around the maximum open.  Every status MD_OK, the bracket holds the value."""
    from optimalbeziertrajectorygeneration_amd import _capi
    yv = S.as_floats(S.wide_speed())
    co = S.coeffs(yv)
    ctx = _capi.Context(1, 3, 4, 0, device=0)
    try:
        for eps in (1e-6, 1e-9, 1e-12):
            ref = S.certified_max(yv, W, Fraction(eps), MAX_NODES, co=co)
            assert ref['status'] == 'ok' and ref['waiting'] <= 32
            g = ctx.space_curvature_true_min_jac(yv[None], W, eps_rel=eps, max_nodes=MAX_NODES)
            assert (g["status"] == _capi.MD_OK).all(), g["status"]
            _hold_value("wide speed, eps %g" % eps, yv, co, ref, float(g["val"][0, 0]), float(g["t_star"][0, 0]), eps)
            assert abs((W - g["val"][0, 0]) - 53.43312516) < 1e-4 and abs(g["t_star"][0, 0] - 0.6649) < 1e-3
        r = ctx.bern_space_curvature(yv, eps_rel=1e-9)
        assert r["status"][0] == _capi.MD_OK and abs(r["k_max"][0] - 53.43312516) < 1e-6
    finally:
        ctx.close()


# 65 items: 5 vehicles x 13 rows; 129 items: 43 vehicles x 3 rows -- lanes, waves and workgroups turn over; degree 5 in
# registers, degree 6 through the workspace
@pytest.mark.parametrize("deg", [5, 6])
@pytest.mark.parametrize("n_veh,B", [(5, 13), (43, 3)])
def test_batches_host_dev_two_launch_and_view(deg, n_veh, B, monkeypatch):
    """One batch -- the finite-difference rows of one row of seeded vehicles, obtg_fd_view_begin's rows (B <= N d (n - 1) + 1;
    only the first B rows of the view are used) -- through the host call, the _dev call, the two-launch form and a call inside
    an FD view with dY == NULL: everything equal bit for bit; every nullable output left out once; in registers against the
    workspace form on the same coefficients (the free-curve call with max_curv = 0)."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    assert B <= n_veh * 3 * (deg - 1) + 1
    Y0 = np.concatenate([S.seeded(deg, s) for s in range(n_veh)])
    Y = synth.fd_batch(Y0, B=B)
    items = B * n_veh
    assert items in (65, 129)
    ctx = _capi.Context(n_veh, 3, deg, 0, device=0)
    try:
        g = ctx.space_curvature_true_min_jac(Y, W, eps_rel=EPS)
        assert (g["status"] == _capi.MD_OK).all()
        rows = ctx.space_curvature_poly(Y)
        dev = torch.device("cuda", 0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dY = torch.from_numpy(Y).to(dev)
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
            i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
            dv, dt, dj, ds = f64(B, n_veh), f64(B, n_veh), f64(B, n_veh, 3, deg + 1), i32(B, n_veh)
            ctx.space_curvature_true_min_jac_dev(dY.data_ptr(), B, W, dv.data_ptr(), dj.data_ptr(), dt.data_ptr(), ds.data_ptr(), eps_rel=EPS)
            dv2, dj2 = f64(B, n_veh), f64(B, n_veh, 3, deg + 1)
            ctx.space_curvature_true_min_jac_dev(dY.data_ptr(), B, W, dv2.data_ptr(), dj2.data_ptr(), eps_rel=EPS)     # t_star, status left out
            dv3, dt3, ds3 = f64(B, n_veh), f64(B, n_veh), i32(B, n_veh)
            ctx.space_curvature_true_min_dev(dY.data_ptr(), B, W, dv3.data_ptr(), dt3.data_ptr(), ds3.data_ptr(), eps_rel=EPS)
            dv4 = f64(B, n_veh)
            ctx.space_curvature_true_min_dev(dY.data_ptr(), B, W, dv4.data_ptr(), eps_rel=EPS)                        # t_star, status left out
            dr = f64(B, n_veh, 4, 2 * deg + 1)
            ctx.space_curvature_poly_dev(dY.data_ptr(), B, dr.data_ptr())
            fv, ft, fj, fs = f64(B, n_veh), f64(B, n_veh), f64(B, n_veh, 3, deg + 1), i32(B, n_veh)
            d0 = torch.from_numpy(np.ascontiguousarray(Y0)).to(dev)
            ctx.fd_view_begin(d0.data_ptr(), 1, synth.FD_STEP, B)
            try:
                ctx.space_curvature_true_min_jac_dev(None, B, W, fv.data_ptr(), fj.data_ptr(), ft.data_ptr(), fs.data_ptr(), eps_rel=EPS)
            finally:
                ctx.fd_view_end()
            torch.cuda.synchronize()
            for got, k in ((dv, "val"), (dv2, "val"), (dv3, "val"), (dv4, "val"), (fv, "val"), (dt, "t_star"), (dt3, "t_star"),
                           (ft, "t_star"), (dj, "jac"), (dj2, "jac"), (fj, "jac")):
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(g[k])), k
            for got in (ds, ds3, fs):
                assert np.array_equal(got.cpu().numpy(), g["status"])
            assert np.array_equal(_bits(dr.cpu().numpy()), _bits(rows))
        finally:
            ctx.use_own_stream()
        # the host call with its nullable outputs left out
        out = np.empty((B, n_veh))
        assert ctx._lib.obtg_space_curvature_true_min(ctx._h, Y.ctypes.data, B, W, EPS, MAX_NODES, out.ctypes.data, None, None) == 0
        assert np.array_equal(_bits(out), _bits(g["val"]))
        # in registers (degree 5) or through the workspace (degree 6) against the workspace form of the free-curve call
        z = ctx.space_curvature_true_min(Y, 0.0, eps_rel=EPS)
        free = ctx.bern_space_curvature(Y.reshape(items, 3, deg + 1), eps_rel=EPS)
        assert np.array_equal(_bits(-z["val"].ravel()), _bits(free["k_max"])) and np.array_equal(_bits(z["t_star"].ravel()), _bits(free["t_max"]))
        assert np.array_equal(z["status"].ravel(), free["status"])
        k2 = np.empty(items)
        t2 = np.empty(items)
        assert ctx._lib.obtg_bern_space_curvature(ctx._h, Y.ctypes.data, items, deg + 1, EPS, MAX_NODES, k2.ctypes.data, t2.ctypes.data, None) == 0
        assert np.array_equal(_bits(k2), _bits(free["k_max"]))
    finally:
        ctx.close()
    monkeypatch.setenv("OBTG_TRUE_MIN_JAC_FUSED", "0")
    ctx = _capi.Context(n_veh, 3, deg, 0, device=0)
    try:
        two = ctx.space_curvature_true_min_jac(Y, W, eps_rel=EPS)
        for k in ("val", "t_star", "jac"):
            assert np.array_equal(_bits(two[k]), _bits(g[k])), "two-launch form: " + k
        assert np.array_equal(two["status"], g["status"])
    finally:
        ctx.close()


@pytest.mark.parametrize("deg", [5, 6])
def test_lifted_planar_curves_against_the_planar_rows(deg):
    """Planar curves of curvature_ref.py's seeded family, snapped so that their lift under the exact rational rotation is exact
    in binary64: obtg_space_curvature_true_min of the lift against obtg_curvature_true_min's max_curv - max(m_+, m_-) of the
    planar curve.  Allowed gap: both searches' tolerances eps max(W, m) plus both points' majorants and the bound majorant."""
    from optimalbeziertrajectorygeneration_amd import _capi
    planar = [S.snap3(C.seeded(deg, s)) for s in range(4)]
    space = [S.as_floats(S.lift(p)) for p in planar]
    c2 = _capi.Context(1, 2, deg, 0, device=0)
    c3 = _capi.Context(1, 3, deg, 0, device=0)
    try:
        for p, q in zip(planar, space):
            a = c2.curvature_true_min(p[None], W, eps_rel=EPS)
            b = c3.space_curvature_true_min(q[None], W, eps_rel=EPS)
            assert (a["status"] == _capi.MD_OK).all() and (b["status"] == _capi.MD_OK).all()
            side = int(np.argmin(a["val"][0, 0]))
            m2, m3 = W - float(a["val"][0, 0, side]), W - float(b["val"][0, 0])
            K2, M2 = C.kappa_majorant(p, float(a["t_star"][0, 0, side]))
            K3, M3 = S.kappa_majorant(q, float(b["t_star"][0, 0]))
            slack = (2 * EPS * max(W, m2, m3) + float((K2 + 1) * U * (M2 + W)) + float((K3 + 1) * U * (M3 + W))
                     + float(S.bound_majorant(q, S.depth_of(float(b["t_star"][0, 0])), points=17)))
            assert abs(m2 - m3) <= slack, (deg, m2, m3, slack)
    finally:
        c2.close()
        c3.close()


def test_degenerate_rows_nan_cusp_and_refusals():
    from optimalbeziertrajectorygeneration_amd import _capi
    # degree 1: w == 0, the row is max_curv, the block zero
    ctx = _capi.Context(N, 3, 1, 0, device=0)
    try:
        Y = np.array([[[0.0, 2.0], [1.0, 5.0], [3.0, -1.0], [0.5, 0.25], [1.0, 1.5], [2.0, -2.0]]])
        g = ctx.space_curvature_true_min_jac(Y, 0.75)
        assert (g["val"] == 0.75).all() and (g["t_star"] == 0.0).all() and (g["status"] == _capi.MD_OK).all() and not g["jac"].any()
    finally:
        ctx.close()
    for deg in (4, 5):         # the workspace form and the in-register form
        ctx = _capi.Context(3, 3, deg, 0, device=0)
        try:
            line = np.stack((np.linspace(0.0, 4.0, deg + 1), np.linspace(1.0, -1.0, deg + 1), np.linspace(0.0, 2.0, deg + 1)))
            rest = np.stack((np.full(deg + 1, 2.5), np.full(deg + 1, -1.0), np.full(deg + 1, 0.25)))
            bad = S.seeded(deg, 0)
            bad[1, 2] = np.nan
            g = ctx.space_curvature_true_min_jac(np.concatenate([line, rest, bad])[None], W)
            assert (g["val"][0, :2] == W).all() and (g["t_star"][0, :2] == 0.0).all() and not g["jac"][0, :2].any()
            assert np.isnan(g["val"][0, 2]) and np.isnan(g["t_star"][0, 2]) and np.isnan(g["jac"][0, 2]).all()
            assert (g["status"] == _capi.MD_OK).all()
            # B == 0 and M == 0 are OBTG_OK and touch nothing
            one, out = np.zeros((1, 9, deg + 1)), np.full((1, 3), 7.0)
            p = lambda a: a.ctypes.data      # noqa: E731
            assert ctx._lib.obtg_space_curvature_true_min(ctx._h, p(one), 0, W, EPS, 100, p(out), None, None) == 0
            assert ctx._lib.obtg_space_curvature_true_min_jac(ctx._h, p(one), 0, W, EPS, 100, p(out), None, None, p(one)) == 0
            assert ctx._lib.obtg_space_curvature_poly(ctx._h, p(one), 0, p(out)) == 0
            assert ctx._lib.obtg_bern_space_curvature(ctx._h, p(one), 0, deg + 1, EPS, 100, p(out), p(out), None) == 0
            assert (out == 7.0).all()
        finally:
            ctx.close()
    # a cusp (den = 0 at t = 1/2 with w != 0 on both sides) ends on a cap status with a finite incumbent, the block finite
    ctx = _capi.Context(1, 3, 3, 0, device=0)
    try:
        g = ctx.space_curvature_true_min_jac(S.CUSP[None], W, eps_rel=EPS, max_nodes=200)
        assert g["status"][0, 0] in (_capi.MD_NODE_CAP, _capi.MD_DEPTH_CAP), g["status"]
        assert np.isfinite(g["val"]).all() and np.isfinite(g["t_star"]).all() and np.isfinite(g["jac"]).all()
        ends = max(float(S.kappa(S.CUSP, 0)), float(S.kappa(S.CUSP, 1)))
        assert W - g["val"][0, 0] >= ends * (1.0 - 1e-12)
        # still the derivative at the returned t_star: held where the majorant says anything -- after 14 nodes the incumbent is
        # the value at t = 1/4 or 3/4 (den's Bernstein coefficients are negative next to the cusp, so the bound of every
        # sub-curve that reaches towards it is +inf and the descent takes the left one first); from 2^-10 of the cusp on the
        # majorant answers inf (rho, the cancellation in den, grows without bound there)
        g = ctx.space_curvature_true_min_jac(S.CUSP[None], W, eps_rel=EPS, max_nodes=14)
        assert g["status"][0, 0] == _capi.MD_NODE_CAP and abs(g["t_star"][0, 0] - 0.5) >= 2.0 ** -8
        _hold_block("cusp", S.CUSP, float(g["t_star"][0, 0]), g["jac"][0, 0])
    finally:
        ctx.close()
    # degree 32 is refused, as is a context that is not in space
    for dim, deg in ((3, 32), (2, 5)):
        ctx = _capi.Context(N, dim, deg, 0, device=0)
        try:
            Yz = np.zeros((1, dim * N, deg + 1))
            for call in (lambda: ctx.space_curvature_true_min(Yz, W), lambda: ctx.space_curvature_true_min_jac(Yz, W),
                         lambda: ctx.space_curvature_poly(Yz)):
                with pytest.raises(_capi.ObtgError) as e:
                    call()
                assert e.value.code == ERR_UNSUPPORTED
            if dim == 2:       # free curves: any context
                r = ctx.bern_space_curvature(S.seeded(7, 1), eps_rel=EPS)
                assert r["status"][0] == _capi.MD_OK
                with pytest.raises(_capi.ObtgError) as e:
                    ctx.bern_space_curvature(np.zeros((1, 3, 33)))
                assert e.value.code == ERR_UNSUPPORTED
        finally:
            ctx.close()


def test_free_curves_and_bezier_space_curvature_max():
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd import bezier as bez
    helix = np.array([[1.0, 1.0, 0.0, -1.0], [0.0, 0.6, 1.2, 1.2], [0.0, 0.3, 0.6, 0.9]])
    k_max, t_max = bez.Bezier(helix).spaceCurvatureMax()
    ref = S.certified_max(helix, 0.0, Fraction(EPS))
    K, M = S.kappa_majorant(helix, t_max)
    assert ref['status'] == 'ok' and float(ref['L']) * (1 - 2e-9) - float((K + 1) * U * M) <= k_max <= float(ref['H']) + float((K + 1) * U * M)
    with pytest.raises(ValueError, match="must be three dimensional"):
        bez.Bezier(np.zeros((2, 4))).spaceCurvatureMax()
    with pytest.raises(RuntimeError):
        bez.Bezier(S.CUSP).spaceCurvatureMax(max_nodes=200)           # a budget that runs out raises
    ctx = _capi.Context(1, 2, 3, 0, device=0)
    try:
        for deg in (2, 7, 31):
            curves = np.stack([S.seeded(deg, 1), S.seeded(deg, 2)])
            r = ctx.bern_space_curvature(curves, eps_rel=EPS)
            assert (r["status"] == _capi.MD_OK).all()
            for i, yv in enumerate(curves):
                ref = S.certified_max(yv, 0.0, Fraction(EPS))
                assert ref['status'] == 'ok'
                _hold_value("free deg %d curve %d" % (deg, i), yv, S.coeffs(yv), ref, -float(r["k_max"][i]), float(r["t_max"][i]), EPS, 0.0)
        curves = np.stack([S.seeded(7, 1), S.seeded(7, 2)])
        r = ctx.bern_space_curvature(curves, eps_rel=EPS)
        dev = torch.device("cuda", 0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dc = torch.from_numpy(curves).to(dev)
            o = [torch.empty(2, dtype=torch.float64, device=dev) for _ in range(2)]
            ds = torch.empty(2, dtype=torch.int32, device=dev)
            ctx.bern_space_curvature_dev(dc.data_ptr(), 2, 8, o[0].data_ptr(), o[1].data_ptr(), ds.data_ptr(), eps_rel=EPS)
            o2 = [torch.empty(2, dtype=torch.float64, device=dev) for _ in range(2)]
            ctx.bern_space_curvature_dev(dc.data_ptr(), 2, 8, o2[0].data_ptr(), o2[1].data_ptr(), eps_rel=EPS)      # status is nullable
            torch.cuda.synchronize()
            for got, got2, k in zip(o, o2, ("k_max", "t_max")):
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(r[k])) and np.array_equal(_bits(got2.cpu().numpy()), _bits(r[k])), k
            assert np.array_equal(ds.cpu().numpy(), r["status"])
        finally:
            ctx.use_own_stream()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ BezOptimization
KMAX = 0.6
FD_SEED = 5


def _problem(**kw):
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=3, dimension=3, degree=5, minimizeGoal='TimeOpt', maxSep=0.9, maxSpeed=5.0,
                           initPoints=[(0, 0, 0), (1, 3, 1), (2, -2, 0.5)], finalPoints=[(6, 1, 2), (7, 4, 0), (8, 0, 3)], tf=8.0,
                           maxSpaceCurvature=KMAX, **kw)


def _certified(yv, rel):
    r = S.certified_max(yv, KMAX, rel)
    assert r['status'] == 'ok'
    return r


def fd_reference(Y, first, cols, fd_step):
    """per vehicle (gap, s, left_out, entries): the yardstick's own largest |central difference of certified maxima (step
    2^-17, brackets 1e-15) - envelope entry|, s = max(KMAX, m), and how many of the vehicle's entries have a yardstick t_star
    that moves by more than 1e-3 between x and x + fd_step e_k"""
    h = 2.0 ** -17
    rel = Fraction(1, 10 ** 15)
    out = []
    for v in range(Y.shape[0] // 3):
        yv = Y[3 * v:3 * v + 3]
        r0 = _certified(yv, rel)
        env = S.envelope_block(yv, r0['t'])
        gap, left, entries = 0.0, 0, 0
        for cc in range(3):
            for i in range(first, first + cols):
                up, dn, fw = yv.copy(), yv.copy(), yv.copy()
                up[cc, i] += h
                dn[cc, i] -= h
                fw[cc, i] += fd_step
                ru, rd, rf = _certified(up, rel), _certified(dn, rel), _certified(fw, Fraction(1, 10 ** 9))
                entries += 1
                left += abs(rf['t'] - r0['t']) > Fraction(1, 1000)
                cd = -(S._mp(ru['L']) - S._mp(rd['L'])) / (2 * h)
                gap = max(gap, float(abs(cd - env[cc][i])))
        out.append((gap, max(KMAX, float(r0['L'])), left, entries))
    return out


def test_closure_and_providers():
    """Row shapes; the kept batch; trueSpaceCurvatureMax; 'envelope' against 'fd' on 3 vehicles of degree 5.  Entries whose
    yardstick t_star moves by more than 1e-3 between x and x + h e_k may be left out, at most 5 % of them; the seed is chosen
    so that the yardstick leaves out none.  Bound per row, as the other families' tests derive it: the yardstick's own largest
    gap between a central difference of certified maxima and its envelope entry on the row, plus the provider's documented
    search slack TRUE_MIN_EPS_REL s / FD_STEP, doubled for the forward difference's curvature term, s = max(bound, m).  The tf
    column of a time-optimal problem without prescribed speeds is exactly 0 (speeds are prescribed for planar problems only)."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    bo = _problem()
    x = bo.generateGuess(std=0.4, seed=FD_SEED)
    Nv = 3
    rows = bo.maxSpaceCurvatureConstraints(x)
    assert rows.shape == (Nv,) and rows.dtype == np.float64
    raw = bo._ctx(False).space_curvature_true_min(bo.reshapeVector(x)[None], KMAX, eps_rel=bo.TRUE_MIN_EPS_REL)
    assert np.array_equal(_bits(rows), _bits(raw["val"][0]))
    k_max, t_max = bo.trueSpaceCurvatureMax(x)
    assert k_max.shape == t_max.shape == (Nv,) and np.allclose(KMAX - k_max, rows, rtol=0, atol=1e-9)
    plain = _problem(fdBatching=False)
    for k in range(x.size):
        xk = x.copy()
        xk[k] += opt.FD_STEP
        assert np.array_equal(_bits(bo.maxSpaceCurvatureConstraints(xk)), _bits(plain.maxSpaceCurvatureConstraints(xk))), k
    assert bo.fdBatchingStats['batches'] == 1 and bo.fdBatchingStats['served'] == x.size
    Je, Jf = bo.maxSpaceCurvatureJacobian(x, method='envelope'), bo.maxSpaceCurvatureJacobian(x, method='fd')
    assert Je.shape == Jf.shape == (Nv, x.size) and x.size == 3 * 3 * 4 + 1
    assert np.array_equal(Je[:, -1], np.zeros(Nv)) and (Jf[:, -1] == 0.0).all()
    with pytest.raises(ValueError, match="not built for the space curvature rows"):
        bo.maxSpaceCurvatureJacobian(x, method='exact')
    ref = fd_reference(bo.reshapeVector(x), bo._rv_parts()[1], bo._numCols, opt.FD_STEP)
    assert sum(r[2] for r in ref) == 0, "the seed leaves out none"
    gap, s = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    bound = 2.0 * (gap + bo.TRUE_MIN_EPS_REL * s / opt.FD_STEP)
    diff = np.abs(Je - Jf).max(axis=1)
    print("largest |envelope - fd| per row", diff, "bound", bound, "yardstick's own gap", gap, "largest entry", np.abs(Je).max())
    assert (diff <= bound).all()
    # a planar problem refuses before any device call
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    b2 = BezOptimization(numVeh=2, dimension=2, degree=5, maxSpaceCurvature=0.5, initPoints=[(0, 0), (3, 0)], finalPoints=[(6, 6), (0, 6.5)], tf=6.0)
    with pytest.raises(ValueError, match="must be three dimensional"):
        b2.maxSpaceCurvatureConstraints(b2.generateGuess(std=0.1, seed=1))


def test_a_solve_with_the_space_curvature_bound_active():
    """One time-optimal SLSQP problem, 2 vehicles of degree 5 in space that have to swerve round each other (maxSep = 1, speed
    at most 3, control-point rows for both), solved without the bound and then, from that solution, with maxSpaceCurvature =
    0.184 -- 0.9 of the unbounded solution's largest curvature, 0.2041 -- under both Jacobians.  Each vehicle's
    trueSpaceCurvatureMax is at most the bound plus ftol (SLSQP accepts a point whose constraint violation is below its acc =
    ftol).  Both solves stop where one more iteration changes tf by less than ftol and the rows are within ftol of feasible:
    with the rows' sensitivity d tf / d row bounded by tf / bound (a row moves by at most its bound while the time moves by at
    most itself), the two times differ by at most 2 ftol (1 + tf / bound) = 3e-8.  Measured on the MI355X: tf 2.575845245
    without the bound (65 iterations), 2.5794136716 with it under 'fd' (95 iterations) and under 'envelope' (125), the
    largest curvature 1e-11 and 4e-16 above the bound."""
    import scipy.optimize as sop
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    ftol = 1e-9
    kmax = 0.184

    def make(curv):
        return BezOptimization(numVeh=2, dimension=3, degree=5, minimizeGoal='TimeOpt', maxSep=1.0, maxSpeed=3.0,
                               initPoints=[(0, 0, 0), (6, 0.5, 0.3)], finalPoints=[(6, 0.2, 0), (0, 0, 0.4)], tf=6.0,
                               maxSpaceCurvature=curv)

    def solve(bo, x0, method):
        cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints, 'jac': bo.temporalSeparationJacobian},
                {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': bo.maxSpeedJacobian},
                {'type': 'ineq', 'fun': lambda x: x[-1:] - 0.1, 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
        if bo.model['maxSpaceCurvature'] is not None:
            cons.append({'type': 'ineq', 'fun': bo.maxSpaceCurvatureConstraints,
                         'jac': lambda x: bo.maxSpaceCurvatureJacobian(x, method=method)})
        return sop.minimize(bo.objectiveFunction, x0=x0, method='SLSQP', constraints=cons,
                            options={'maxiter': 400, 'ftol': ftol, 'disp': False})
    free = make(None)
    r0 = solve(free, free.generateGuess(std=0.3, seed=2), None)
    assert r0.status == 0, r0.message
    k0 = free.trueSpaceCurvatureMax(r0.x)[0].max()
    assert k0 > kmax * 1.05, k0                      # the bound cuts into the unconstrained solution
    tfs = {}
    for method in ('fd', 'envelope'):
        bo = make(kmax)
        r = solve(bo, r0.x, method)
        worst = bo.trueSpaceCurvatureMax(r.x)[0]
        print("unbounded: tf %.9f, max kappa %.6f; bounded at %.3f under %r: tf %.10f, max kappa - bound %s, SLSQP status %d after %d iterations"
              % (r0.fun, k0, kmax, method, r.fun, worst - kmax, r.status, r.nit))
        assert r.status == 0, r.message
        assert (worst <= kmax + ftol).all()
        assert worst.max() >= kmax - 1e-6 and r.fun >= r0.fun - ftol      # active, and it costs time
        tfs[method] = r.fun
    assert abs(tfs['fd'] - tfs['envelope']) <= 2 * ftol * (1 + tfs['fd'] / kmax), tfs
