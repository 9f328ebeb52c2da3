"""The true angular-rate rows and their envelope Jacobian on the device (obtg_ang_rate_poly, obtg_ang_rate_true_min[_jac],
BezOptimization(angRateRows='true_min'), maxAngularRateJacobian(method='envelope'), trueAngularRateRows) against the
exact-rational yardstick of tests/ang_envelope_ref.py.  Every device case is 3 vehicles and a few rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import ang_envelope_ref as A  # noqa: E402
import test_ang_envelope_ref as T  # noqa: E402
from util import RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3
W = 1.25
ERR_ARG = -1
BLOCK_TOL = 1e-13      # of the block's largest entry (the speed family measured 7.7e-16; the margin covers degree 31's recurrences)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _hold_blocks(g, Yb, tf, what, w=W):
    """every (vehicle, side)'s block within BLOCK_TOL of its own largest yardstick entry, d/dtf within BLOCK_TOL of the larger
    of its two terms (2 W den / T, 3 num / T: their difference may cancel), at the device's own t_star; returns the worst
    scaled differences (block, d/dtf)"""
    worst = [0.0, 0.0]
    for b in range(Yb.shape[0]):
        blk, dtf = A.envelope_blocks(Yb[b], tf[b], w, g["t_star"][b])
        for v in range(blk.shape[0]):
            for side in range(2):
                what_ = "%s row %d vehicle %d side %d" % (what, b, v, side)
                ref, got = blk[v, side], g["jac"][b, v, side]
                if not ref.any():
                    assert not got.any(), what_ + ": a zero block"
                else:
                    err = np.abs(got - ref).max() / np.abs(ref).max()
                    worst[0] = max(worst[0], err)
                    assert err <= BLOCK_TOL, (what_, err)
                den, num = A.den_num(Yb[b, 2 * v:2 * v + 2], tf[b], g["t_star"][b, v, side])
                scale = max(abs(2.0 * w * float(den)), abs(3.0 * float(num))) / tf[b]
                if scale == 0.0:
                    assert g["jac_tf"][b, v, side] == 0.0, what_ + ": a zero d/dtf"
                else:
                    err = abs(g["jac_tf"][b, v, side] - dtf[v, side]) / scale
                    worst[1] = max(worst[1], err)
                    assert err <= BLOCK_TOL, (what_ + " d/dtf", err)
    return worst


def _hold_values(g, Yb, tf, eps_rel, w=W):
    """val inside the yardstick's bracket [L, H] of the oracle's row: L - r <= val <= H + eps_rel s + r, s the row's largest
    coefficient, r = 1e-12 s for the rounding of the coefficients (device and oracle form them in different orders)"""
    for b in range(Yb.shape[0]):
        for v, sides in enumerate(A.true_rows(Yb[b], tf[b], w)):
            for side, y in enumerate(sides):
                s = float(y["s"])
                r = 1e-12 * s
                assert float(y["L"]) - r <= g["val"][b, v, side] <= float(y["H"]) + eps_rel * s + r, (b, v, side)


@pytest.mark.parametrize("B", [3, 50])
@pytest.mark.parametrize("deg", T.LISTED + T.UNLISTED)
def test_bits_and_blocks(deg, B):
    """B = 3: 18 items, a partial wave; B = 50: 300 items, across a wave and a workgroup.  (1) val, t_star, status of the _jac
    call are the bits of the value call, and both the bits of obtg_bern_extrema on obtg_ang_rate_poly's rows (the context
    has DEG_ELEV = 2: it does not enter); (2) obtg_ang_rate_poly against the oracle's coefficients within 1e-12 of the row's
    largest; (3) val inside the yardstick's bracket; (4) blocks and jac_tf against the yardstick at the device's own t_star;
    (5) launches under OBTG_K_ANG_RATE: 1 on the list, 2 / 3 off it."""
    from optimalbeziertrajectorygeneration_amd import _capi
    Yb, tf = T.batch(deg, B, N)
    fused = deg in T.LISTED
    ctx = _capi.Context(N, 2, deg, 2, device=0)
    try:
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        g = ctx.ang_rate_true_min_jac(Yb, tf, W, eps_rel=RTOL)
        stats = ctx.kernel_stats()
        assert stats["ang_rate"][1] == (1 if fused else 3) and sum(n for _, n in stats.values()) == stats["ang_rate"][1], stats
        ctx.reset_kernel_stats()
        v = ctx.ang_rate_true_min(Yb, tf, W, eps_rel=RTOL)
        stats = ctx.kernel_stats()
        ctx.set_profiling(False)
        assert stats["ang_rate"][1] == (1 if fused else 2) and sum(n for _, n in stats.values()) == stats["ang_rate"][1], stats
        assert g["val"].shape == (B, N, 2) and g["jac"].shape == (B, N, 2, 2, deg + 1) and g["jac_tf"].shape == (B, N, 2)
        assert ctx.deg_elev == 2
        rows = ctx.ang_rate_poly(Yb, tf, W)
        assert rows.shape == (B, N, 2, 2 * deg + 1)
        e = ctx.bern_extrema(rows.reshape(-1, 2 * deg + 1), eps_rel=RTOL, eps_abs=0.0)
        for k in ("val", "t_star"):
            assert np.array_equal(_bits(g[k]), _bits(v[k])), k
            assert np.array_equal(_bits(v[k]).ravel(), _bits(e[k])), k + " against obtg_bern_extrema of obtg_ang_rate_poly's rows"
        assert np.array_equal(g["status"], v["status"]) and np.array_equal(v["status"].ravel(), e["status"])
        assert (g["status"] == _capi.MD_OK).all()
        worst_c = 0.0
        for b in range(B):
            ref = A.ang_coeffs(Yb[b], tf[b], W)
            err = np.abs(rows[b] - ref).max(axis=2) / np.abs(ref).max(axis=2)
            worst_c = max(worst_c, err.max())
            assert (err <= 1e-12).all(), (b, err)
        _hold_values(g, Yb, tf, RTOL)
        worst = _hold_blocks(g, Yb, tf, "deg %d B %d" % (deg, B))
        print("deg %d B %d: largest scaled |device - yardstick|: coefficients %.3e, block %.3e, d/dtf %.3e"
              % (deg, B, worst_c, worst[0], worst[1]))
        if deg >= 3:
            inside = (g["t_star"] > 0.0) & (g["t_star"] < 1.0)
            assert inside.any() and (~inside).any(), "the case must hold interior and end minima"
        # a row alone: the bits it has inside the batch
        b = B - 1
        one = ctx.ang_rate_true_min_jac(Yb[b:b + 1], tf[b:b + 1], W, eps_rel=RTOL)
        for k in ("val", "t_star", "jac", "jac_tf"):
            assert np.array_equal(_bits(one[k][0]), _bits(g[k][b])), (k, b)
    finally:
        ctx.close()


@pytest.mark.parametrize("deg", [5, 10, 4])
def test_fused_and_two_launch_forms_give_the_same_bits(deg, monkeypatch):
    """OBTG_TRUE_MIN_JAC_FUSED=0, in a context of its own: the blocks in a launch of their own.  Launches under
    OBTG_K_ANG_RATE: 1 fused, 2 in the two-launch form; off the list 3 either way."""
    from optimalbeziertrajectorygeneration_amd import _capi
    Yb, tf = T.batch(deg, 5, N)
    got, launches = [], []
    for fused in (True, False):
        if not fused:
            monkeypatch.setenv("OBTG_TRUE_MIN_JAC_FUSED", "0")
        c = _capi.Context(N, 2, deg, 0, device=0)
        try:
            c.set_profiling(True)
            c.reset_kernel_stats()
            got.append(c.ang_rate_true_min_jac(Yb, tf, W, eps_rel=1e-12))
            stats = c.kernel_stats()
            launches.append(stats["ang_rate"][1])
            assert sum(n for _, n in stats.values()) == stats["ang_rate"][1], stats
        finally:
            c.close()
    monkeypatch.delenv("OBTG_TRUE_MIN_JAC_FUSED")
    assert launches == ([1, 2] if deg in T.LISTED else [3, 3]), launches
    a, b = got
    for k in ("val", "t_star", "jac", "jac_tf"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["status"], b["status"])


@pytest.mark.parametrize("deg", [5, 12])
def test_dev_twins(deg):
    """The _dev calls against the host calls, nullable outputs, and dY = NULL inside an obtg_fd_view."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi, synth
    B = 4
    Yb, tf = T.batch(deg, B, N)
    L = 2 * deg + 1
    ctx = _capi.Context(N, 2, deg, 0, device=0)
    try:
        g = ctx.ang_rate_true_min_jac(Yb, tf, W, eps_rel=RTOL)
        rows = ctx.ang_rate_poly(Yb, tf, W)
        dev = torch.device("cuda", 0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dY, dtf = torch.from_numpy(Yb).to(dev), torch.from_numpy(tf).to(dev)
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
            i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
            dv, dt, dg, dj, ds = f64(B, N, 2), f64(B, N, 2), f64(B, N, 2), f64(B, N, 2, 2, deg + 1), i32(B, N, 2)
            ctx.ang_rate_true_min_jac_dev(dY.data_ptr(), dtf.data_ptr(), B, W, dv.data_ptr(), dj.data_ptr(), dg.data_ptr(),
                                          dt.data_ptr(), ds.data_ptr(), eps_rel=RTOL)
            dv2, dj2 = f64(B, N, 2), f64(B, N, 2, 2, deg + 1)         # t_star, status and jac_tf are nullable
            ctx.ang_rate_true_min_jac_dev(dY.data_ptr(), dtf.data_ptr(), B, W, dv2.data_ptr(), dj2.data_ptr(), eps_rel=RTOL)
            dv3, dt3, ds3 = f64(B, N, 2), f64(B, N, 2), i32(B, N, 2)
            ctx.ang_rate_true_min_dev(dY.data_ptr(), dtf.data_ptr(), B, W, dv3.data_ptr(), dt3.data_ptr(), ds3.data_ptr(), eps_rel=RTOL)
            dv4 = f64(B, N, 2)
            ctx.ang_rate_true_min_dev(dY.data_ptr(), dtf.data_ptr(), B, W, dv4.data_ptr(), eps_rel=RTOL)
            dr = f64(B, N, 2, L)
            ctx.ang_rate_poly_dev(dY.data_ptr(), dtf.data_ptr(), B, W, dr.data_ptr())
            torch.cuda.synchronize()
            for got, k in ((dv, "val"), (dv2, "val"), (dv3, "val"), (dv4, "val"), (dt, "t_star"), (dt3, "t_star"), (dg, "jac_tf"),
                           (dj, "jac"), (dj2, "jac")):
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(g[k])), k
            assert np.array_equal(ds.cpu().numpy(), g["status"]) and np.array_equal(ds3.cpu().numpy(), g["status"])
            assert np.array_equal(_bits(dr.cpu().numpy()), _bits(rows))
            # inside a view: the finite-difference batch of ONE row, formed on the device; dY = NULL
            n_rows = 1 + N * 2 * (deg - 1)                            # synth.fd_batch: the interior columns move
            Yfd = synth.fd_batch(Yb[0], B=n_rows)
            tfd = np.full(n_rows, tf[0])
            want = ctx.ang_rate_true_min_jac(Yfd, tfd, W, eps_rel=RTOL)
            want_rows = ctx.ang_rate_poly(Yfd, tfd, W)
            d0, dtfd = torch.from_numpy(np.ascontiguousarray(Yb[0])).to(dev), torch.from_numpy(tfd).to(dev)
            fv, ft, fg, fj, fs = f64(n_rows, N, 2), f64(n_rows, N, 2), f64(n_rows, N, 2), f64(n_rows, N, 2, 2, deg + 1), i32(n_rows, N, 2)
            fv2, fr = f64(n_rows, N, 2), f64(n_rows, N, 2, L)
            ctx.fd_view_begin(d0.data_ptr(), 1, synth.FD_STEP, n_rows)
            try:
                ctx.ang_rate_true_min_jac_dev(None, dtfd.data_ptr(), n_rows, W, fv.data_ptr(), fj.data_ptr(), fg.data_ptr(),
                                              ft.data_ptr(), fs.data_ptr(), eps_rel=RTOL)
                ctx.ang_rate_true_min_dev(None, dtfd.data_ptr(), n_rows, W, fv2.data_ptr(), eps_rel=RTOL)
                ctx.ang_rate_poly_dev(None, dtfd.data_ptr(), n_rows, W, fr.data_ptr())
            finally:
                ctx.fd_view_end()
            torch.cuda.synchronize()
            for got, k in ((fv, "val"), (fv2, "val"), (ft, "t_star"), (fg, "jac_tf"), (fj, "jac")):
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[k])), "view: " + k
            assert np.array_equal(fs.cpu().numpy(), want["status"])
            assert np.array_equal(_bits(fr.cpu().numpy()), _bits(want_rows))
        finally:
            ctx.use_own_stream()
    finally:
        ctx.close()


def _ends_case(deg):
    """(Y[2 * 2][deg + 1], tf): vehicle 0 turns ever harder to the left (a spiral that tightens: the left row's minimum is at
    t = 1), vehicle 1 is the same path run backwards (a right turn that opens: the right row's minimum is at t = 0)"""
    u = np.arange(deg + 1) / deg
    th = 2.0 * u ** 2
    a = np.array([np.cumsum(np.cos(th)) / deg * 6.0, np.cumsum(np.sin(th)) / deg * 6.0])
    return np.concatenate([a, a[:, ::-1]]), 2.0


@pytest.mark.parametrize("deg", [5, 6])
def test_edge_rows(deg):
    """A vehicle at rest: zero coefficients, val = +0.0, t_star 0, zero block and d/dtf.  A straight line at constant speed:
    num = 0, both sides W |v|^2, status OK.  Minima at t_star = 0 and 1: only the block's first / last three columns are
    non-zero.  A NaN control point: NaN val, t_star, block and d/dtf, status OK.  max_nodes = 3: NODE_CAP, val not below the
    yardstick's lower bound, a finite block that is the yardstick's at the returned t_star."""
    from optimalbeziertrajectorygeneration_amd import _capi
    Yb, tfb = T.batch(deg, 1, 4)
    Y, tf = Yb[0].copy(), tfb[:1]
    c = _capi.Context(4, 2, deg, 0, device=0)
    try:
        Yr = Y.copy()
        Yr[2:4] = np.array([[1.25], [-3.5]])                       # vehicle 1 at rest
        Yr[4] = 0.5 + 3.0 * np.arange(deg + 1)                     # vehicle 2: a straight line, control points on integers and
        Yr[5] = -2.0 + 4.0 * np.arange(deg + 1)                    #   halves: every difference exact, x'' = y'' = 0 exactly
        Yr[6, 2] = np.nan                                          # vehicle 3: a NaN control point
        g = c.ang_rate_true_min_jac(Yr[None], tf, W, eps_rel=RTOL)
        v = c.ang_rate_true_min(Yr[None], tf, W, eps_rel=RTOL)
        rows = c.ang_rate_poly(Yr[None], tf, W)
        assert (g["status"] == _capi.MD_OK).all()
        assert np.array_equal(_bits(g["val"]), _bits(v["val"])) and np.array_equal(_bits(g["t_star"]), _bits(v["t_star"]))
        assert np.array_equal(_bits(rows[0, 1]), _bits(np.zeros((2, 2 * deg + 1))))
        assert np.array_equal(_bits(g["val"][0, 1]), _bits(np.zeros(2))) and (g["t_star"][0, 1] == 0.0).all()
        assert (g["jac"][0, 1] == 0.0).all() and (g["jac_tf"][0, 1] == 0.0).all()
        speed2 = (deg * 3.0 / tf[0]) ** 2 + (deg * 4.0 / tf[0]) ** 2
        # (x' is constant up to the rounding of elev(1)'s weights c/n + (n-c)/n, so num is zero up to a few ulp of W |v|^2)
        assert np.abs(rows[0, 2] - W * speed2).max() <= 1e-13 * W * speed2, "num = 0: both sides are the constant W |v|^2"
        assert np.abs(g["val"][0, 2] - W * speed2).max() <= 1e-13 * W * speed2
        assert np.abs(g["jac_tf"][0, 2] + 2.0 * W * speed2 / tf[0]).max() <= 1e-13 * 2.0 * W * speed2 / tf[0]
        assert np.isnan(g["val"][0, 3]).all() and np.isnan(g["t_star"][0, 3]).all() and np.isnan(g["jac"][0, 3]).all()
        assert np.isnan(g["jac_tf"][0, 3]).all() and np.isnan(rows[0, 3]).any()
        assert np.isfinite(g["val"][0, :3]).all() and np.isfinite(g["jac"][0, :3]).all() and np.isfinite(g["jac_tf"][0, :3]).all()
        g = c.ang_rate_true_min_jac(Y[None], tf, W, eps_rel=1e-14, max_nodes=3)
        v = c.ang_rate_true_min(Y[None], tf, W, eps_rel=1e-14, max_nodes=3)
        assert (g["status"] == _capi.MD_NODE_CAP).any() and np.array_equal(g["status"], v["status"])
        assert np.array_equal(_bits(g["val"]), _bits(v["val"])) and np.array_equal(_bits(g["t_star"]), _bits(v["t_star"]))
        for vv, sides in enumerate(A.true_rows(Y, tf[0], W)):
            for side, y in enumerate(sides):
                assert g["val"][0, vv, side] >= float(y["L"]) - 1e-12 * float(y["s"]), (vv, side)
        assert np.isfinite(g["jac"]).all() and np.isfinite(g["jac_tf"]).all()
        _hold_blocks(g, Y[None], tf, "node cap")
    finally:
        c.close()
    Ye, tfe = _ends_case(deg)
    we = 0.25                                                       # below the peak rate: the rows' minima are negative, at the tight end
    sides = A.true_rows(Ye, tfe, we)
    assert sides[0][0]["t"] == 1 and sides[1][1]["t"] == 0, "the yardstick alone: where this case has its minima"
    c = _capi.Context(2, 2, deg, 0, device=0)
    try:
        g = c.ang_rate_true_min_jac(Ye[None], np.array([tfe]), we, eps_rel=RTOL)
        assert (g["status"] == _capi.MD_OK).all()
        assert g["t_star"][0, 0, 0] == 1.0 and g["t_star"][0, 1, 1] == 0.0
        for blk, keep in ((g["jac"][0, 0, 0], [deg - 2, deg - 1, deg]), (g["jac"][0, 1, 1], [0, 1, 2])):
            assert (np.delete(blk, keep, axis=1) == 0.0).all() and (blk[:, keep] != 0.0).all(), (blk, keep)
        _hold_values(g, Ye[None], np.array([tfe]), RTOL, we)
        _hold_blocks(g, Ye[None], np.array([tfe]), "ends", we)
    finally:
        c.close()


def test_arguments_and_return_codes():
    """One check per sentence of the C ABI: the speed entry points' checks, dim != 2 -> OBTG_ERR_ARG, deg > 31 ->
    OBTG_ERR_UNSUPPORTED, optional t_star / status / jac_tf, B == 0 is OK."""
    from optimalbeziertrajectorygeneration_amd import _capi
    deg = 4
    Yb, tf = T.batch(deg, 2, N)
    L = 2 * deg + 1
    c = _capi.Context(N, 2, deg, 0, device=0)
    try:
        lib, h, p = c._lib, c._h, _capi._ptr
        out, ts, jac = np.empty((2, N, 2)), np.empty((2, N, 2)), np.empty((2, N, 2, 2, deg + 1))
        st, rows = np.zeros((2, N, 2), np.int32), np.empty((2, N, 2, L))
        full = c.ang_rate_true_min_jac(Yb, tf, W)
        # optional outputs
        assert lib.obtg_ang_rate_true_min(h, p(Yb), p(tf), 2, W, 1e-9, 100000, p(out), None, None) == 0
        assert np.array_equal(_bits(out), _bits(full["val"]))
        assert lib.obtg_ang_rate_true_min_jac(h, p(Yb), p(tf), 2, W, 1e-9, 100000, p(out), None, None, p(jac), None) == 0
        assert np.array_equal(_bits(out), _bits(full["val"])) and np.array_equal(_bits(jac), _bits(full["jac"]))
        # B == 0
        assert lib.obtg_ang_rate_poly(h, p(Yb), p(tf), 0, W, p(rows)) == 0
        assert lib.obtg_ang_rate_true_min(h, p(Yb), p(tf), 0, W, 1e-9, 100, p(out), p(ts), p(st)) == 0
        assert lib.obtg_ang_rate_true_min_jac(h, p(Yb), p(tf), 0, W, 1e-9, 100, p(out), p(ts), p(st), p(jac), None) == 0
        # null pointers, a negative batch, max_nodes < 1, a negative or NaN eps_rel
        bad = [lib.obtg_ang_rate_poly(h, None, p(tf), 2, W, p(rows)), lib.obtg_ang_rate_poly(h, p(Yb), None, 2, W, p(rows)),
               lib.obtg_ang_rate_poly(h, p(Yb), p(tf), 2, W, None), lib.obtg_ang_rate_poly(h, p(Yb), p(tf), -1, W, p(rows)),
               lib.obtg_ang_rate_poly(None, p(Yb), p(tf), 2, W, p(rows)),
               lib.obtg_ang_rate_true_min(h, None, p(tf), 2, W, 1e-9, 100, p(out), None, None),
               lib.obtg_ang_rate_true_min(h, p(Yb), None, 2, W, 1e-9, 100, p(out), None, None),
               lib.obtg_ang_rate_true_min(h, p(Yb), p(tf), 2, W, 1e-9, 100, None, None, None),
               lib.obtg_ang_rate_true_min(h, p(Yb), p(tf), -1, W, 1e-9, 100, p(out), None, None),
               lib.obtg_ang_rate_true_min(h, p(Yb), p(tf), 2, W, 1e-9, 0, p(out), None, None),
               lib.obtg_ang_rate_true_min(h, p(Yb), p(tf), 2, W, -1e-9, 100, p(out), None, None),
               lib.obtg_ang_rate_true_min(h, p(Yb), p(tf), 2, W, float("nan"), 100, p(out), None, None),
               lib.obtg_ang_rate_true_min_jac(h, p(Yb), p(tf), 2, W, 1e-9, 100, p(out), None, None, None, None),
               lib.obtg_ang_rate_true_min_jac(h, None, p(tf), 2, W, 1e-9, 100, p(out), None, None, p(jac), None),
               lib.obtg_ang_rate_true_min_dev(h, None, None, 2, W, 1e-9, 100, p(out), None, None),
               lib.obtg_ang_rate_true_min_jac_dev(h, None, p(tf), 2, W, 1e-9, 100, p(out), None, None, None, None)]
        assert bad == [ERR_ARG] * len(bad), bad
    finally:
        c.close()
    c3 = _capi.Context(N, 3, deg, 0, device=0)
    try:
        Y3 = np.zeros((1, N * 3, deg + 1))
        lib, h, p = c3._lib, c3._h, _capi._ptr
        one = np.ones(1)
        o3 = np.empty((1, N, 2, 2 * deg + 1))
        assert lib.obtg_ang_rate_poly(h, p(Y3), p(one), 1, W, p(o3)) == ERR_ARG
        assert lib.obtg_ang_rate_true_min(h, p(Y3), p(one), 1, W, 1e-9, 100, p(o3), None, None) == ERR_ARG
        assert lib.obtg_ang_rate_true_min_jac(h, p(Y3), p(one), 1, W, 1e-9, 100, p(o3), None, None, p(o3), None) == ERR_ARG
    finally:
        c3.close()
    big = _capi.Context(1, 2, 32, 0, device=0)
    try:
        for call in (big.ang_rate_poly, big.ang_rate_true_min, big.ang_rate_true_min_jac):
            with pytest.raises(_capi.ObtgError) as err:
                call(np.zeros((1, 2, 33)), 1.0, 1.0)
            assert err.value.code == _capi.ERR_UNSUPPORTED
    finally:
        big.close()


# ------------------------------------------------------------------ BezOptimization
def _dubins(**kw):
    """time-optimal, speeds and headings prescribed: tf moves columns 1 and -2 of every vehicle"""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, minSpeed=0.2, maxAngRate=1,
                           initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)], initSpeeds=[1, 1], finalSpeeds=[1, 1],
                           initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], **kw)


def _planar(**kw):
    """fixed tf, 3 vehicles, degree 6 (off the fused list)"""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=3, dimension=2, degree=6, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=3, minSpeed=0.1, maxAngRate=1,
                           tf=6.0, initPoints=[(0, 0), (3, 0), (6, 0.5)], finalPoints=[(6, 6), (0, 6.5), (3, 6)], **kw)


# (constructor, noise seed): the seeds are those at which the YARDSTICK ALONE, on the CPU, finds no tied row
# (test_ang_envelope_ref.yardstick_gap's third result) -- the envelope test below may leave out at most 1 row in 10
PROBLEMS = {"dubins": (_dubins, 7), "planar": (_planar, 4)}


def _x0(make, seed):
    bo = make(angRateRows='true_min')
    x = bo.generateGuess(std=0.3, seed=seed)
    if bo._timeopt():
        x[-1] = 9.0
    return bo, x


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_closures_and_providers(name):
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    make, seed = PROBLEMS[name]
    bo, x = _x0(make, seed)
    Nv = bo.model['numVeh']
    ctx = bo._ctx(False)
    first, cols = bo._rv_parts()[1], bo._numCols
    D = bo._dY_dtf() if bo._timeopt() else None
    Wm = bo.model['maxAngRate']
    raw = ctx.ang_rate_true_min(bo.reshapeVector(x)[None], bo._tf_of(x), Wm, eps_rel=bo.TRUE_MIN_EPS_REL)
    rows = bo.maxAngularRateConstraints(x)
    assert rows.shape == (2 * Nv,) and np.array_equal(_bits(rows), _bits(raw["val"][0].ravel()))
    val, t_star = bo.trueAngularRateRows(x)
    assert np.array_equal(_bits(val), _bits(raw["val"][0])) and np.array_equal(_bits(t_star), _bits(raw["t_star"][0]))
    # SciPy's forward differences: served from one batch, identical to direct calls
    plain = make(angRateRows='true_min', fdBatching=False)
    before = dict(bo.fdBatchingStats)
    for k in range(x.size):
        xk = x.copy()
        xk[k] += opt.FD_STEP
        assert np.array_equal(_bits(bo.maxAngularRateConstraints(xk)), _bits(plain.maxAngularRateConstraints(xk))), k
    assert bo.fdBatchingStats['served'] - before['served'] == x.size and bo.fdBatchingStats['batches'] - before['batches'] == 1
    # the envelope provider: dense [2N][n_x], free columns of the vehicle's own block, the tf column with the dY/dtf chain
    J = bo.maxAngularRateJacobian(x, method='envelope')
    assert J.shape == (2 * Nv, x.size) and np.isfinite(J).all()
    tf = float(bo._tf_of(x))
    r = ctx.ang_rate_true_min_jac(bo.reshapeVectors(x[None]), tf, Wm, eps_rel=bo.TRUE_MIN_EPS_REL)
    assert np.array_equal(_bits(r["val"]), _bits(raw["val"]))
    blk, dtf = A.envelope_blocks(bo.reshapeVector(x), tf, Wm, r["t_star"][0])
    want = A.scatter(blk, dtf, Nv, first, cols, D)
    n_pts = Nv * 2 * cols
    for i in range(2 * Nv):
        scale = np.abs(blk[i // 2, i % 2]).max()
        assert np.abs(J[i, :n_pts] - want[i, :n_pts]).max() <= BLOCK_TOL * scale, (name, i)
    if D is not None:
        assert D.any() and J.shape[1] == n_pts + 1
        for i in range(2 * Nv):
            den, num = A.den_num(bo.reshapeVector(x)[2 * (i // 2):2 * (i // 2) + 2], tf, r["t_star"][0, i // 2, i % 2])
            scale = max(abs(2.0 * Wm * float(den)), abs(3.0 * float(num))) / tf + np.abs(blk[i // 2, i % 2] * D.reshape(Nv, 2, -1)[i // 2]).sum()
            assert abs(J[i, -1] - want[i, -1]) <= 1e-12 * scale, (name, i)
        assert np.abs(want[:, -1] - dtf.ravel()).max() > 1e-6 * np.abs(dtf).max(), "the dY/dtf chain must matter in this case"
    with pytest.raises(ValueError, match="envelope"):
        bo.maxAngularRateJacobian(x, method='exact')
    other = make()
    with pytest.raises(ValueError, match="true_min"):
        other.maxAngularRateJacobian(x, method='envelope')
    assert other.maxAngularRateConstraints(x).shape == (Nv * (4 * bo.model['deg'] + 1),)


def test_three_dimensions_raise_the_reference_error():
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    bo = BezOptimization(numVeh=2, dimension=3, degree=5, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=3, minSpeed=0.1, maxAngRate=1,
                         tf=6.0, initPoints=[(0, 0, 0), (3, 0, 1)], finalPoints=[(6, 6, 2), (0, 6.5, 1)], angRateRows='true_min')
    x = bo.generateGuess(std=0.1, seed=1)
    with pytest.raises(ValueError, match="must be two dimensional"):
        bo.maxAngularRateConstraints(x)
    with pytest.raises(ValueError, match="must be two dimensional"):
        bo.maxAngularRateJacobian(x, method='envelope')
    with pytest.raises(ValueError, match="must be two dimensional"):
        bo.maxAngularRateJacobian(x, method='fd')


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_envelope_against_the_finite_difference_provider(name):
    """method='fd' (forward differences of the search itself, h = FD_STEP) against method='envelope', entry by entry.  The
    bound of a row is the yardstick's own largest |central difference of certified minima (step 2^-17, brackets 1e-20 s) -
    envelope entry at its own minimiser| on that row, plus the finite-difference provider's documented search slack
    TRUE_MIN_EPS_REL * s / FD_STEP, times 2 for the forward difference's curvature term -- the bound of
    test_gpu_speed_true_min.py.  Rows whose certified minimiser moves by more than 1e-3 between x +- h are ties and are left
    out, at most 1 row in 10."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    make, seed = PROBLEMS[name]
    bo, x = _x0(make, seed)
    Je, Jf = bo.maxAngularRateJacobian(x, method='envelope'), bo.maxAngularRateJacobian(x, method='fd')
    assert Je.shape == Jf.shape == (2 * bo.model['numVeh'], x.size)
    yard_gap, s, tie = T.yardstick_gap(bo, x)
    assert tie.sum() * 10 <= tie.size, tie
    bound = 2.0 * (yard_gap + bo.TRUE_MIN_EPS_REL * s / opt.FD_STEP)
    gap = np.abs(Je - Jf).max(axis=1)
    print("%s: largest |envelope - fd| per row" % name, gap, "bound", bound, "yardstick's own gap", yard_gap, "ties", tie,
          "largest entry", np.abs(Je).max())
    assert (gap[~tie] <= bound[~tie]).all()


def test_solve_with_the_true_angular_rate_rows():
    """example15's two solves at ftol = 1e-10: the control-point rows from the straight-line guess, the true rows from that
    solve's solution.  (1) Relaxation: at the control-point solution every true row is >= -1e-9 s, s the row's largest
    coefficient.  (2) From that start the true-row solve ends with tf not above the start's by more than 1e-9.  (3) On 2001
    sampled points |omega| <= W (1 + 1e-6) at the true-row solution.  SLSQP's status and iteration count are printed, not
    asserted (DESIGN.md 4.16 records them)."""
    import example15_true_angular_rate as ex
    bo_a, res_a = ex.solve('all', ftol=1e-10)
    val_a, t_a = bo_a.trueAngularRateRows(res_a.x)
    s_a = np.abs(bo_a._ctx(False).ang_rate_poly(bo_a.reshapeVector(res_a.x)[None], bo_a._tf_of(res_a.x), ex.MAX_ANG_RATE)[0]).max(axis=2)
    print("control-point rows: tf %.9f, %d iterations, status %d; true rows there / s:" % (res_a.fun, res_a.nit, res_a.status), val_a / s_a)
    assert (val_a >= -1e-9 * s_a).all(), (val_a, s_a)
    bo_t, res_t = ex.solve('true_min', ftol=1e-10, x0=res_a.x)
    val_t, t_t = bo_t.trueAngularRateRows(res_t.x)
    om = ex.angular_rate(bo_t, res_t.x, np.linspace(0.0, 1.0, 2001))
    print("true rows: tf %.9f, %d iterations, status %d (%s); true rows %s at %s; largest sampled |omega| per vehicle %s"
          % (res_t.fun, res_t.nit, res_t.status, res_t.message, val_t, t_t, np.abs(om).max(axis=1)))
    assert res_t.fun <= res_a.fun + 1e-9
    assert (np.abs(om) <= ex.MAX_ANG_RATE * (1.0 + 1e-6)).all(), np.abs(om).max(axis=1)
    assert bo_t.maxAngularRateConstraints(res_t.x).shape == (4,) and bo_a.maxAngularRateConstraints(res_a.x).shape == (2 * 41,)
