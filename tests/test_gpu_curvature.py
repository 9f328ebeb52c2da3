"""The curvature rows on the device (obtg_curvature_poly, obtg_curvature_true_min[_jac], obtg_bern_curvature,
Bezier.curvatureRange, BezOptimization(maxCurvature=...)) against the exact-rational yardstick of tests/curvature_ref.py.

Shapes: N = 2 vehicles; degree 1 (degenerate), 2 (K = 5), 6 (workspace path), 10 (in-register path), 31 (K = 63, the last
lane), 32 (refused); B = 1 and B = 65 -- 260 items, so the lane step and the wave search both run beyond the first wave.
Regular inputs: per degree three curves of the seeded family on which the YARDSTICK's search ends with at most 32 waiting
and within max_nodes -- decided on the CPU before the device sees them -- plus the parabola, cycled through the batch.  Every
device status on them must be MD_OK.  Every bound is a majorant curvature_ref.py derives; none is a tuned number."""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curvature_ref as C  # noqa: E402

pytestmark = pytest.mark.gpu

N = 2
W = 1.0                   # max_curv
EPS = 1e-9
MAX_NODES = 100000
U = mpmath.mpf(2) ** -53
LISTED = (3, 5, 7, 8, 10, 15, 20)        # degrees whose coefficients stay in registers
ERR_ARG, ERR_UNSUPPORTED = -1, -5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_CASES = {}


def cases(deg):
    """[dict(yv, co, ref[2], values)]: the degree's distinct curves with the yardstick's coefficients, its certified search of
    both sides (the search that admitted the seed) and its 4097-point sample; computed once, shared, left unchanged"""
    if deg not in _CASES:
        out = []
        for yv in C.regular_curves(deg, 3, EPS, MAX_NODES, W):
            co = C.coeffs(yv)
            ref = [C.certified_max(yv, s, W, Fraction(EPS), MAX_NODES, co=co) for s in range(2)]
            assert all(r['status'] == 'ok' and r['waiting'] <= 32 for r in ref)
            out.append(dict(yv=yv, co=co, ref=ref, values=C.sample_values(yv, 4097, co)))
        _CASES[deg] = out
    return _CASES[deg]


def batch(deg, B):
    """Y[B][N * 2][deg + 1] and which[B][N]: vehicle v of row b is curve (N b + v) mod (number of curves)"""
    cs = cases(deg)
    which = np.array([[(N * b + v) % len(cs) for v in range(N)] for b in range(B)])
    return np.stack([np.concatenate([cs[i]['yv'] for i in row]) for row in which]), which


def _hold(deg, g, rows, which):
    """every check of a device result g (val, t_star, status, jac) of a batch on the yardstick's curves"""
    from optimalbeziertrajectorygeneration_amd import _capi
    cs = cases(deg)
    assert (g["status"] == _capi.MD_OK).all(), np.argwhere(g["status"] != _capi.MD_OK)
    first = {}
    worst = dict(val=0.0, coeff=0.0, block=0.0)
    for b in range(which.shape[0]):
        for v in range(N):
            for side in range(2):
                key = (which[b, v], side)
                if key in first:      # the same curve elsewhere in the batch: the same bits, whatever its position
                    b0, v0 = first[key]
                    for k in ("val", "t_star", "jac"):
                        assert np.array_equal(_bits(g[k][b, v, side]), _bits(g[k][b0, v0, side])), (k, b, v, side)
                    continue
                first[key] = (b, v)
                c = cs[key[0]]
                yv, co, ref = c['yv'], c['co'], c['ref'][side]
                out, t = float(g["val"][b, v, side]), float(g["t_star"][b, v, side])
                what = "deg %d curve %d side %d" % (deg, key[0], side)
                # t_star: a dyadic point of [0, 1] at a depth a bisection can reach
                assert 0.0 <= t <= 1.0 and C.depth_of(t) <= 64, what
                m = Fraction(W) - Fraction(out)              # the device's m_sigma, exactly as the row holds it
                K, M = C.kappa_majorant(yv, t, co=co)
                assert mpmath.isfinite(M), what
                maj = (K + 1) * U * (M + W)
                tol = Fraction(EPS) * max(Fraction(W), m)
                clamped = out == W
                if clamped:
                    assert t == 0.0 and not g["jac"][b, v, side].any(), what + ": a clamped side has t_star 0 and a zero block"
                else:
                    # out = max_curv - sigma kappa(t_star), against the rational kappa at the device's own t_star
                    want = W - C.SIGMA[side] * C.kappa(yv, t)
                    err = abs(mpmath.mpf(out) - want)
                    worst["val"] = max(worst["val"], float(err / maj))
                    assert err <= maj, (what, float(err), float(maj))
                # the yardstick's certified bracket holds the device's m_sigma within tol plus the majorant
                assert C._mp(ref['L']) - C._mp(tol) - maj <= C._mp(m) <= C._mp(ref['H']) + maj, (what, float(m), float(ref['L']), float(ref['H']))
                # no point of the 4097-point rational sample is above m_sigma + tol
                assert C.sample_exceeds(yv, side, max(m, 0) + tol, values=c['values']) == [], what
                if not clamped:
                    Kb, Mb = C.block_majorant(yv, t)
                    blk = C.envelope_block(yv, side, t)
                    for cc in range(2):
                        for i in range(deg + 1):
                            bound = mpmath.mpf("1.05") * Kb * U * Mb[cc][i]
                            assert mpmath.isfinite(bound), what
                            err = abs(mpmath.mpf(float(g["jac"][b, v, side, cc, i])) - blk[cc][i])
                            assert err <= bound, (what, cc, i, float(err), float(bound))
                            if bound:      # (t_star = 0 or 1: the columns away from that end are exact zeros on both sides)
                                worst["block"] = max(worst["block"], float(err / bound))
            # obtg_curvature_poly's rows: num then den, each within its majorant of the rational coefficient
            if (which[b, v], 'rows') not in first:
                first[(which[b, v], 'rows')] = True
                co = cs[which[b, v]]['co']
                for part in range(2):
                    for k in range(2 * deg + 1):
                        bound = C.coeff_count(deg) * C.UNIT * co[2 + part][k]
                        err = abs(Fraction(float(rows[b, v, part, k])) - co[part][k])
                        if bound:
                            worst["coeff"] = max(worst["coeff"], float(err / bound))
                        assert err <= bound, (deg, which[b, v], part, k)
    return worst


# 2: K = 5; 6: the workspace path; 31: K = 63; 3, 5, 7, 8, 10, 15, 20: every in-register instantiation
@pytest.mark.parametrize("deg", [2, 3, 5, 6, 7, 8, 10, 15, 20, 31])
def test_rows_against_the_yardstick(deg, monkeypatch):
    """B = 65 on the host path: values, t_star, the bracket, the sample, the coefficients and the blocks against the yardstick;
    the _jac call's out / t_star / status are the plain call's bits; a row alone (B = 1) has the bits it has as row 64; the
    two-launch form (OBTG_TRUE_MIN_JAC_FUSED=0) gives the fused form's bits; launches under OBTG_K_ANG_RATE: 1 in registers
    (2 with the blocks in their own launch), 2 / 3 through the workspace."""
    from optimalbeziertrajectorygeneration_amd import _capi
    B = 65
    Y, which = batch(deg, B)
    assert len(set(which.ravel())) == 4 and np.array_equal(which[64], which[0])
    ctx = _capi.Context(N, 2, deg, 0, device=0)
    try:
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        g = ctx.curvature_true_min_jac(Y, W, eps_rel=EPS, max_nodes=MAX_NODES)
        launches = [ctx.kernel_stats()["ang_rate"][1]]
        ctx.reset_kernel_stats()
        v = ctx.curvature_true_min(Y, W, eps_rel=EPS, max_nodes=MAX_NODES)
        stats = ctx.kernel_stats()
        launches.append(stats["ang_rate"][1])
        assert sum(n for _, n in stats.values()) == launches[1], stats
        ctx.set_profiling(False)
        assert launches == ([1, 1] if deg in LISTED else [3, 2]), launches
        assert g["val"].shape == (B, N, 2) and g["jac"].shape == (B, N, 2, 2, deg + 1)
        for k in ("val", "t_star"):
            assert np.array_equal(_bits(g[k]), _bits(v[k])), k
        assert np.array_equal(g["status"], v["status"])
        rows = ctx.curvature_poly(Y)
        assert rows.shape == (B, N, 2, 2 * deg + 1)
        worst = _hold(deg, g, rows, which)
        print("deg %d: largest |device - yardstick| / majorant: value %.3g, coefficient %.3g, block entry %.3g"
              % (deg, worst["val"], worst["coeff"], worst["block"]))
        # the parabola is in the batch: it never turns right, and turns left with kappa = 2 at its middle
        par = np.argwhere(which == 3)[0]
        assert g["val"][par[0], par[1], 1] == W and abs(g["val"][par[0], par[1], 0] - (W - 2.0)) <= 1e-9 * 2.0
        t_par = g["t_star"][par[0], par[1], 0]      # (degree 2 is the parabola itself; above, its float64 elevation)
        assert t_par == 0.5 if deg == 2 else abs(t_par - 0.5) <= 1e-3
        one = ctx.curvature_true_min_jac(Y[:1], W, eps_rel=EPS, max_nodes=MAX_NODES)
        for k in ("val", "t_star", "jac"):
            assert np.array_equal(_bits(one[k][0]), _bits(g[k][64])), k
        assert np.array_equal(one["status"][0], g["status"][64])
    finally:
        ctx.close()
    monkeypatch.setenv("OBTG_TRUE_MIN_JAC_FUSED", "0")
    ctx = _capi.Context(N, 2, deg, 0, device=0)
    try:
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        two = ctx.curvature_true_min_jac(Y, W, eps_rel=EPS, max_nodes=MAX_NODES)
        assert ctx.kernel_stats()["ang_rate"][1] == (2 if deg in LISTED else 3)
        for k in ("val", "t_star", "jac"):
            assert np.array_equal(_bits(two[k]), _bits(g[k])), "two-launch form: " + k
        assert np.array_equal(two["status"], g["status"])
    finally:
        ctx.close()


@pytest.mark.parametrize("deg", [6, 10])
@pytest.mark.parametrize("B", [1, 65])
def test_dev_twins(deg, B):
    """host and _dev give the same bits; t_star and status are nullable; dY = NULL inside an obtg_fd_view"""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    Y, _ = batch(deg, B)
    L = 2 * deg + 1
    ctx = _capi.Context(N, 2, deg, 0, device=0)
    try:
        g = ctx.curvature_true_min_jac(Y, W, eps_rel=EPS)
        rows = ctx.curvature_poly(Y)
        dev = torch.device("cuda", 0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dY = torch.from_numpy(Y).to(dev)
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
            i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
            dv, dt, dj, ds = f64(B, N, 2), f64(B, N, 2), f64(B, N, 2, 2, deg + 1), i32(B, N, 2)
            ctx.curvature_true_min_jac_dev(dY.data_ptr(), B, W, dv.data_ptr(), dj.data_ptr(), dt.data_ptr(), ds.data_ptr(), eps_rel=EPS)
            dv2, dj2 = f64(B, N, 2), f64(B, N, 2, 2, deg + 1)
            ctx.curvature_true_min_jac_dev(dY.data_ptr(), B, W, dv2.data_ptr(), dj2.data_ptr(), eps_rel=EPS)
            dv3, dt3, ds3 = f64(B, N, 2), f64(B, N, 2), i32(B, N, 2)
            ctx.curvature_true_min_dev(dY.data_ptr(), B, W, dv3.data_ptr(), dt3.data_ptr(), ds3.data_ptr(), eps_rel=EPS)
            dv4 = f64(B, N, 2)
            ctx.curvature_true_min_dev(dY.data_ptr(), B, W, dv4.data_ptr(), eps_rel=EPS)
            dr = f64(B, N, 2, L)
            ctx.curvature_poly_dev(dY.data_ptr(), B, dr.data_ptr())
            torch.cuda.synchronize()
            for got, k in ((dv, "val"), (dv2, "val"), (dv3, "val"), (dv4, "val"), (dt, "t_star"), (dt3, "t_star"), (dj, "jac"), (dj2, "jac")):
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(g[k])), k
            assert np.array_equal(ds.cpu().numpy(), g["status"]) and np.array_equal(ds3.cpu().numpy(), g["status"])
            assert np.array_equal(_bits(dr.cpu().numpy()), _bits(rows))
            if B == 1:
                n_rows = 1 + N * 2 * (deg - 1)                            # synth.fd_batch: the interior columns move
                Yfd = synth.fd_batch(Y[0], B=n_rows)
                want = ctx.curvature_true_min_jac(Yfd, W, eps_rel=EPS)
                fv, ft, fj, fs = f64(n_rows, N, 2), f64(n_rows, N, 2), f64(n_rows, N, 2, 2, deg + 1), i32(n_rows, N, 2)
                d0 = torch.from_numpy(np.ascontiguousarray(Y[0])).to(dev)
                ctx.fd_view_begin(d0.data_ptr(), 1, synth.FD_STEP, n_rows)
                try:
                    ctx.curvature_true_min_jac_dev(None, n_rows, W, fv.data_ptr(), fj.data_ptr(), ft.data_ptr(), fs.data_ptr(), eps_rel=EPS)
                finally:
                    ctx.fd_view_end()
                torch.cuda.synchronize()
                for got, k in ((fv, "val"), (ft, "t_star"), (fj, "jac")):
                    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[k])), "view: " + k
                assert np.array_equal(fs.cpu().numpy(), want["status"])
        finally:
            ctx.use_own_stream()
    finally:
        ctx.close()


def test_degenerate_rows_and_refusals():
    from optimalbeziertrajectorygeneration_amd import _capi
    # degree 1: num == 0, both rows are max_curv, the blocks zero
    ctx = _capi.Context(N, 2, 1, 0, device=0)
    try:
        Y = np.array([[[0.0, 2.0], [1.0, 5.0], [3.0, -1.0], [0.5, 0.25]]])
        g = ctx.curvature_true_min_jac(Y, 0.75)
        assert (g["val"] == 0.75).all() and (g["t_star"] == 0.0).all() and (g["status"] == _capi.MD_OK).all() and not g["jac"].any()
    finally:
        ctx.close()
    # degree 32 is refused, as is a context that is not planar; B = 0 is not an error
    ctx = _capi.Context(N, 2, 32, 0, device=0)
    try:
        for call in (lambda: ctx.curvature_true_min(np.zeros((1, 2 * N, 33)), W), lambda: ctx.curvature_true_min_jac(np.zeros((1, 2 * N, 33)), W),
                     lambda: ctx.curvature_poly(np.zeros((1, 2 * N, 33)))):
            with pytest.raises(_capi.ObtgError) as e:
                call()
            assert e.value.code == ERR_UNSUPPORTED
    finally:
        ctx.close()
    ctx = _capi.Context(N, 3, 5, 0, device=0)
    try:
        for call in (lambda: ctx.curvature_true_min(np.zeros((1, 3 * N, 6)), W), lambda: ctx.curvature_poly(np.zeros((1, 3 * N, 6)))):
            with pytest.raises(_capi.ObtgError) as e:
                call()
            assert e.value.code == ERR_ARG
    finally:
        ctx.close()
    for deg in (6, 10):
        ctx = _capi.Context(N, 2, deg, 0, device=0)
        try:
            # B == 0 is OBTG_OK and touches nothing (the C calls themselves: the Python layer does not pass an empty batch on)
            one, out = np.zeros((1, 2 * N, deg + 1)), np.full((1, N, 2), 7.0)
            p = lambda a: a.ctypes.data      # noqa: E731
            assert ctx._lib.obtg_curvature_true_min(ctx._h, p(one), 0, W, EPS, 100, p(out), None, None) == 0
            assert ctx._lib.obtg_curvature_true_min_jac(ctx._h, p(one), 0, W, EPS, 100, p(out), None, None, p(one)) == 0
            assert ctx._lib.obtg_curvature_poly(ctx._h, p(one), 0, p(out)) == 0
            assert ctx._lib.obtg_bern_curvature(ctx._h, p(one), 0, deg + 1, EPS, 100, p(out), p(out), p(out), p(out), None) == 0
            assert (out == 7.0).all()
            # a NaN control point in vehicle 0, vehicle 1 at rest (every control point the same)
            Y = np.stack([np.concatenate([C.seeded(deg, 0), np.stack((np.full(deg + 1, 2.5), np.full(deg + 1, -1.0)))])])
            Y[0, 1, 2] = np.nan
            g = ctx.curvature_true_min_jac(Y, W)
            assert np.isnan(g["val"][0, 0]).all() and np.isnan(g["t_star"][0, 0]).all() and np.isnan(g["jac"][0, 0]).all()
            assert (g["val"][0, 1] == W).all() and (g["t_star"][0, 1] == 0.0).all() and not g["jac"][0, 1].any()
            assert (g["status"] == _capi.MD_OK).all()
        finally:
            ctx.close()


@pytest.mark.parametrize("deg", [4, 5])
def test_a_curve_whose_speed_varies_widely(deg):
    """curvature_ref.WIDE_SPEED (degree 4: the workspace path; its float64 elevation to degree 5: in registers): den varies by
    far more than 5x across the nodes next to t = 0, where a bound that looks at the num_k > 0 alone closes too early and
    reports 0.02801 for side 1.  Admitted as the regular inputs are -- the yardstick's search ends with at most 32 waiting
    -- so every status must be MD_OK; no point of the 4097-point rational sample is above m_sigma + tol; the yardstick's
    bracket holds m_sigma; side 1's maximum is the 0.0349 near t = 0.046."""
    from optimalbeziertrajectorygeneration_amd import _capi
    yv = C.elevated(C.WIDE_SPEED, deg)
    co = C.coeffs(yv)
    values = C.sample_values(yv, 4097, co)
    ctx = _capi.Context(1, 2, deg, 0, device=0)
    try:
        for eps in (1e-6, 1e-9, 1e-12):
            ref = [C.certified_max(yv, s, W, Fraction(eps), MAX_NODES, co=co) for s in range(2)]
            assert all(r['status'] == 'ok' and r['waiting'] <= 32 for r in ref)
            g = ctx.curvature_true_min_jac(yv[None], W, eps_rel=eps, max_nodes=MAX_NODES)
            assert (g["status"] == _capi.MD_OK).all(), g["status"]
            for side in range(2):
                out, t = float(g["val"][0, 0, side]), float(g["t_star"][0, 0, side])
                m = Fraction(W) - Fraction(out)
                K, M = C.kappa_majorant(yv, t, co=co)
                maj = (K + 1) * U * (M + W)
                tol = Fraction(eps) * max(Fraction(W), m)
                assert mpmath.isfinite(M) and abs(mpmath.mpf(out) - (W - C.SIGMA[side] * C.kappa(yv, t))) <= maj
                assert C._mp(ref[side]['L']) - C._mp(tol) - maj <= C._mp(m) <= C._mp(ref[side]['H']) + maj, (eps, side, float(m))
                assert C.sample_exceeds(yv, side, m + tol, values=values) == [], (eps, side, float(m))
            assert abs((W - g["val"][0, 0, 1]) - 0.034917) < 2e-6 and abs(g["t_star"][0, 0, 1] - 0.0462) < 1e-3
        r = ctx.bern_curvature(yv, eps_rel=1e-9)
        assert (r["status"] == _capi.MD_OK).all() and abs(-r["k_min"][0] - 0.034917) < 2e-6
    finally:
        ctx.close()


def test_free_curves_on_device_memory_and_a_rest_to_rest_curve():
    """obtg_bern_curvature_dev gives the host call's bits.  A rest-to-rest curve (the first two and the last two control
    points coincide: den = 0 at both ends) offers no value at its ends: the free-curve search goes on from there to interior
    points -- it does not answer NaN with MD_OK from the first step -- and ends with a finite value met inside, or on a cap."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    curves = np.stack([C.seeded(7, 1), C.seeded(7, 2), C.elevated(C.PARABOLA, 7)])
    ctx = _capi.Context(1, 2, 3, 0, device=0)
    try:
        r = ctx.bern_curvature(curves, eps_rel=EPS)
        dev = torch.device("cuda", 0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dc = torch.from_numpy(curves).to(dev)
            o = [torch.empty(3, dtype=torch.float64, device=dev) for _ in range(4)]
            ds = torch.empty((3, 2), dtype=torch.int32, device=dev)
            ctx.bern_curvature_dev(dc.data_ptr(), 3, 8, *[a.data_ptr() for a in o], ds.data_ptr(), eps_rel=EPS)
            o2 = [torch.empty(3, dtype=torch.float64, device=dev) for _ in range(4)]
            ctx.bern_curvature_dev(dc.data_ptr(), 3, 8, *[a.data_ptr() for a in o2], eps_rel=EPS)      # status is nullable
            torch.cuda.synchronize()
            for got, got2, k in zip(o, o2, ("k_min", "t_min", "k_max", "t_max")):
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(r[k])) and np.array_equal(_bits(got2.cpu().numpy()), _bits(r[k])), k
            assert np.array_equal(ds.cpu().numpy(), r["status"])
        finally:
            ctx.use_own_stream()
        rest = np.array([[0.0, 0.0, 1.0, 3.0, 4.0, 4.0], [0.0, 0.0, 2.0, -1.0, 1.0, 1.0]])
        assert C.num_den(rest, 0.0)[1] == 0 and C.num_den(rest, 1.0)[1] == 0
        q = ctx.bern_curvature(rest, eps_rel=EPS, max_nodes=2000)
        for side, (k, t) in enumerate(((q["k_max"][0], q["t_max"][0]), (q["k_min"][0], q["t_min"][0]))):
            if q["status"][0, side] == _capi.MD_OK or np.isfinite(k):
                assert np.isfinite(k) and 0.0 < t < 1.0, (side, k, t)
                K, M = C.kappa_majorant(rest, t)
                assert abs(mpmath.mpf(float(k)) - C.kappa(rest, t)) <= (K + 1) * U * M
            else:
                assert q["status"][0, side] in (_capi.MD_NODE_CAP, _capi.MD_DEPTH_CAP)
        assert not ((q["status"][0] == _capi.MD_OK) & np.isnan([q["k_max"][0], q["k_min"][0]])).any()
    finally:
        ctx.close()


def test_the_semicubical_cusp_ends_on_a_cap():
    """x = (2t - 1)^3, y = (2t - 1)^2 as a degree-3 curve: the curvature is unbounded at t = 1/2, where the speed vanishes.
    max_nodes = 200: the call returns, the side that diverges (right turns) ends on a cap, and what it reports is a finite
    value at least as large as the ends' (where the search starts)."""
    from optimalbeziertrajectorygeneration_amd import _capi
    cusp = np.array([[-1.0, 1.0, -1.0, 1.0], [1.0, -1.0 / 3.0, -1.0 / 3.0, 1.0]])
    ctx = _capi.Context(1, 2, 3, 0, device=0)
    try:
        g = ctx.curvature_true_min_jac(cusp[None], W, eps_rel=EPS, max_nodes=200)
        assert g["status"][0, 0, 1] in (_capi.MD_NODE_CAP, _capi.MD_DEPTH_CAP), g["status"]
        assert np.isfinite(g["val"]).all() and np.isfinite(g["t_star"]).all()
        ends = max(float(-C.kappa(cusp, 0.0)), float(-C.kappa(cusp, 1.0)))
        assert W - g["val"][0, 0, 1] >= ends * (1.0 - 1e-12)
        assert g["val"][0, 0, 0] <= W
        r = ctx.bern_curvature(cusp, eps_rel=EPS, max_nodes=200)
        assert r["status"][0, 1] != _capi.MD_OK and np.isfinite(r["k_min"]).all() and r["k_min"][0] <= -ends * (1.0 - 1e-12)
    finally:
        ctx.close()


def test_free_curves_and_bezier_curvature_range():
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd import bezier as bez
    k_min, t_min, k_max, t_max = bez.Bezier(C.PARABOLA).curvatureRange()
    assert abs(k_max - 2.0) <= 2e-9 and t_max == 0.5
    assert abs(k_min - 2.0 / 5.0 ** 1.5) <= 1e-9 * k_min and t_min in (0.0, 1.0)
    with pytest.raises(ValueError, match="must be two dimensional"):
        bez.Bezier(np.zeros((3, 4))).curvatureRange()
    # any degree on any context: the yardstick's unclamped brackets hold the device's range
    ctx = _capi.Context(1, 3, 4, 0, device=0)
    try:
        for deg in (2, 7, 31):
            curves = np.stack([c['yv'] for c in cases(deg)]) if deg in _CASES else np.stack([C.seeded(deg, 1), C.seeded(deg, 2)])
            r = ctx.bern_curvature(curves, eps_rel=EPS)
            assert (r["status"] == _capi.MD_OK).all()
            for i, yv in enumerate(curves):
                lo, hi = C.curvature_range(yv, Fraction(EPS))
                for got, t, (a, b) in ((r["k_min"][i], r["t_min"][i], lo), (r["k_max"][i], r["t_max"][i], hi)):
                    K, M = C.kappa_majorant(yv, t)
                    slack = Fraction(EPS) * abs(b) + Fraction(float((K + 1) * U * M))
                    assert a - slack <= Fraction(float(got)) <= b + slack, (deg, i)
                    assert abs(mpmath.mpf(float(got)) - C.kappa(yv, t)) <= (K + 1) * U * M
        with pytest.raises(_capi.ObtgError) as e:
            ctx.bern_curvature(np.zeros((1, 2, 33)))
        assert e.value.code == ERR_UNSUPPORTED
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ BezOptimization
def _problem(**kw):
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='TimeOpt', maxSep=0.9, maxSpeed=5.0, maxAngRate=1.0,
                           initPoints=[(0, 0), (1, 3)], finalPoints=[(6, 1), (7, 4)], tf=8.0, maxCurvature=0.6, **kw)


def _certified(yv, side, rel):
    r = C.certified_max(yv, side, 0.6, rel)
    assert r['status'] == 'ok'
    return r


def test_closure_and_providers():
    """Row shapes; 'envelope' against 'fd' within the forward-difference bound the other families' tests use -- the yardstick's
    own largest |central difference of certified maxima (step 2^-17, brackets 1e-18) - envelope entry| on the row plus the
    provider's documented search slack TRUE_MIN_EPS_REL s / FD_STEP, doubled for the forward difference's curvature term, s =
    max(maxCurvature, m_sigma) -- and the tf column of a time-optimal problem without prescribed speeds: exactly 0."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    bo = _problem()
    x = bo.generateGuess(std=0.4, seed=5)
    Nv, nc = 2, 6
    rows = bo.maxCurvatureConstraints(x)
    assert rows.shape == (2 * Nv,) and rows.dtype == np.float64
    raw = bo._ctx(False).curvature_true_min(bo.reshapeVector(x)[None], 0.6, eps_rel=bo.TRUE_MIN_EPS_REL)
    assert np.array_equal(_bits(rows), _bits(raw["val"][0].ravel()))
    k_min, t_min, k_max, t_max = bo.trueCurvatureRange(x)
    assert k_min.shape == (Nv,) and (k_min <= k_max).all()
    assert np.allclose(np.minimum(0.6 - np.maximum(k_max, 0.0), 0.6 - np.maximum(-k_min, 0.0)), rows.reshape(Nv, 2).min(axis=1), rtol=0, atol=1e-9)
    plain = _problem(fdBatching=False)
    for k in range(x.size):
        xk = x.copy()
        xk[k] += opt.FD_STEP
        assert np.array_equal(_bits(bo.maxCurvatureConstraints(xk)), _bits(plain.maxCurvatureConstraints(xk))), k
    assert bo.fdBatchingStats['batches'] == 1 and bo.fdBatchingStats['served'] == x.size
    Je, Jf = bo.maxCurvatureJacobian(x, method='envelope'), bo.maxCurvatureJacobian(x, method='fd')
    assert Je.shape == Jf.shape == (2 * Nv, x.size) and x.size == 17
    assert np.array_equal(Je[:, -1], np.zeros(2 * Nv)) and (Jf[:, -1] == 0.0).all()
    # the yardstick's own gap between a central difference of certified maxima and its envelope entry
    Y = bo.reshapeVector(x)
    first, cols = bo._rv_parts()[1], bo._numCols
    h = 2.0 ** -17
    rel = Fraction(1, 10 ** 18)
    gap, s, tie = np.zeros(2 * Nv), np.zeros(2 * Nv), np.zeros(2 * Nv, bool)
    for v in range(Nv):
        yv = Y[2 * v:2 * v + 2]
        for side in range(2):
            r0 = _certified(yv, side, rel)
            s[2 * v + side] = max(0.6, float(r0['L']))
            if r0['L'] == 0:
                assert not Je[2 * v + side].any()
                continue
            env = C.envelope_block(yv, side, r0['t'])
            for cc in range(2):
                for i in range(first, first + cols):
                    up, dn = yv.copy(), yv.copy()
                    up[cc, i] += h
                    dn[cc, i] -= h
                    ru, rd = _certified(up, side, rel), _certified(dn, side, rel)
                    tie[2 * v + side] |= abs(ru['t'] - rd['t']) > Fraction(1, 1000)
                    cd = -(C._mp(ru['L']) - C._mp(rd['L'])) / (2 * h)
                    gap[2 * v + side] = max(gap[2 * v + side], float(abs(cd - env[cc][i])))
    assert not tie.any(), tie
    bound = 2.0 * (gap + bo.TRUE_MIN_EPS_REL * s / opt.FD_STEP)
    diff = np.abs(Je - Jf).max(axis=1)
    print("largest |envelope - fd| per row", diff, "bound", bound, "yardstick's own gap", gap, "largest entry", np.abs(Je).max())
    assert (diff <= bound).all()


def test_refusals_on_the_device_path():
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    bo = BezOptimization(numVeh=2, dimension=3, degree=5, maxCurvature=0.5, initPoints=[(0, 0, 0), (3, 0, 1)],
                         finalPoints=[(6, 6, 2), (0, 6.5, 1)], tf=6.0)
    x = bo.generateGuess(std=0.1, seed=1)
    with pytest.raises(ValueError, match="must be two dimensional"):
        bo.maxCurvatureConstraints(x)
    bo = BezOptimization(numVeh=2, dimension=2, degree=5, initPoints=[(0, 0), (3, 0)], finalPoints=[(6, 6), (0, 6.5)], tf=6.0)
    with pytest.raises(ValueError) as e:
        bo.maxCurvatureConstraints(bo.generateGuess(std=0.1, seed=1))
    assert str(e.value) == "maxCurvatureConstraints needs a bound: maxCurvature is None"


def test_a_solve_with_the_curvature_bound_active():
    """One SLSQP solve, 2 vehicles, degree 5, shortest paths (Euclidean goal) between poses that force a turn: without the bound
    the solution turns harder than maxCurvature; with it the bound is active at the solution, and trueCurvatureRange there is
    within the bound plus SLSQP's acc."""
    import scipy.optimize as sop
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    acc = 1e-8
    kmax = 0.4

    def make(curv):
        return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=0.5, maxSpeed=10.0, maxAngRate=10.0,
                               initPoints=[(0, 0), (0, 4)], finalPoints=[(4, 3), (4, 7)], initSpeeds=[1, 1], finalSpeeds=[1, 1],
                               initAngs=[0, 0], finalAngs=[np.pi / 2, np.pi / 2], tf=8.0, maxCurvature=curv)

    def solve(bo, x0):
        cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints}]
        if bo.model['maxCurvature'] is not None:
            cons.append({'type': 'ineq', 'fun': bo.maxCurvatureConstraints,
                         'jac': lambda x: bo.maxCurvatureJacobian(x, method='envelope')})
        return sop.minimize(bo.objectiveFunction, x0=x0, method='SLSQP', constraints=cons,
                            options={'maxiter': 200, 'ftol': acc, 'disp': False})
    free = make(None)
    r0 = solve(free, free.generateGuess(std=0))
    k0 = np.abs(np.array(free.trueCurvatureRange(r0.x))[[0, 2]]).max()
    assert k0 > kmax * 1.05, k0                      # the bound cuts into the unconstrained solution
    bo = make(kmax)
    r = solve(bo, r0.x)
    k_min, _, k_max, _ = bo.trueCurvatureRange(r.x)
    worst = max(np.abs(k_min).max(), np.abs(k_max).max())
    print("unbounded: max |kappa| %.6f; bounded at %.2f: max |kappa| %.9f, SLSQP status %d after %d iterations, objective %.6f -> %.6f"
          % (k0, kmax, worst, r.status, r.nit, r0.fun, r.fun))
    assert r.status == 0, r.message
    assert worst <= kmax + acc
    assert worst >= kmax - 1e-6 and r.fun >= r0.fun      # active, and it costs length
