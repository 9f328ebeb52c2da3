"""The proximity rows on the device (obtg_ctx_set_proximity, obtg_proximity_poly, obtg_proximity_true[_jac]) against the two
layers of tests/proximity_ref.py: the float restatement gives the expected bits, the exact-rational layer the truth.  One batch
per (dim, degree) serves every test: N = 3 vehicles, Q = 2 points, B = 4 rows, P = 8 items holding every combination of
{reach, within} x {point, vehicle target} x {full window, proper window}; degrees 3, 5, 10 have kernels that form the
coefficients in registers, degree 4 goes through the workspace rows."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proximity_ref as PR  # noqa: E402
import test_proximity_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

N, B = PR.N_VEH, PR.B_ROWS
EPS = PR.EPS_REL
ERR_ARG, ERR_UNSUPPORTED = -1, -5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_dev = {}


def device(dim, deg):
    """The batch, what the yardstick says about it, and the device's answers, made once per configuration and left unchanged"""
    if (dim, deg) not in _dev:
        from optimalbeziertrajectorygeneration_amd import _capi
        bt, cs = T.cases(dim, deg)
        c = _capi.Context(N, dim, deg, 0, device=0)
        try:
            c.set_proximity(bt["items"], bt["params"], bt["pts"])
            poly = np.array(c.proximity_poly(bt["Y"]))
            val = c.proximity_true(bt["Y"], eps_rel=EPS)
            jac = c.proximity_true_jac(bt["Y"], eps_rel=EPS)
            want = {}
            for kind in (PR.WITHIN, PR.REACH):
                sel = bt["items"][:, 2] == kind
                want[kind] = (sel, c.bern_extrema(poly[:, sel].reshape(-1, 2 * deg + 1), want_max=bool(kind), eps_rel=EPS, eps_abs=0.0))
        finally:
            c.close()
        _dev[(dim, deg)] = dict(bt=bt, cs=cs, poly=poly, val={k: np.array(v) for k, v in val.items()},
                                jac={k: np.array(v) for k, v in jac.items()}, want=want)
    return _dev[(dim, deg)]


# ------------------------------------------------------------------------------------------------ 1. the coefficients
@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_poly_is_the_float_restatement(dim, deg):
    """obtg_proximity_poly equals the float restatement bit for bit; an item with the full window has the bits of
    fma(-1, obtg_temporal_sep's R = 0 row at max_sep = 0, (d/2) rho^2) for the same pair, the row formed by a context whose
    point obstacles are the family's points."""
    from optimalbeziertrajectorygeneration_amd import _capi
    d = device(dim, deg)
    bt, L = d["bt"], 2 * deg + 1
    assert d["poly"].shape == (B, 8, L)
    diff = np.argwhere(_bits(d["poly"]) != _bits(d["cs"]["rows"]))
    assert diff.size == 0, "(row, item, k) of the first coefficients that differ: %s" % diff[:8].tolist()
    c = _capi.Context(N, dim, deg, 0, point_obs=bt["pts"], device=0)
    try:
        sep = np.array(c.temporal_sep(bt["Y"], 0.0)).reshape(B, -1, L)
    finally:
        c.close()
    n_obj = N + PR.N_PTS
    pairs = [(i, j) for i in range(n_obj - 1) for j in range(i + 1, n_obj)]
    full = 0
    for p, (it, pr) in enumerate(zip(bt["items"], bt["params"])):
        if (pr[1], pr[2]) != (0.0, 1.0):
            continue
        full += 1
        row = sep[:, pairs.index((min(it[0], it[1]), max(it[0], it[1])))]
        off = (0.5 * dim) * (pr[0] * pr[0])
        want = np.array([[PR.fma(-1.0, v, off) for v in r] for r in row])
        assert np.array_equal(_bits(d["poly"][:, p]), _bits(want)), p
    assert full == 4


# ------------------------------------------------------------------------------------------------ 2. the search
@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_true_is_bern_extrema_of_the_rows(dim, deg):
    """val, bound, nodes, status are the bits of obtg_bern_extrema(eps_abs = 0, want_max = kind) on test 1's rows, t_star is
    fma(t_w, tau1 - tau0, tau0) of that call's parameter; on the fused degrees and on degree 4 alike.  The batch shows on the
    device what the yardstick promised: a search that splits, both signs of both kinds, extrema at window ends inside the
    curve and at the curve's ends."""
    from optimalbeziertrajectorygeneration_amd import _capi
    d = device(dim, deg)
    bt, g = d["bt"], d["val"]
    for kind, (sel, e) in d["want"].items():
        for k in ("val", "bound"):
            assert np.array_equal(_bits(g[k][:, sel]).ravel(), _bits(e[k])), (k, kind)
        for k in ("nodes", "status"):
            assert np.array_equal(g[k][:, sel].ravel(), e[k]), (k, kind)
        par = np.tile(bt["params"][sel], (B, 1))
        t_star = np.array([PR.curve_t(t, w[1], w[2]) for t, w in zip(e["t_star"], par)])
        assert np.array_equal(_bits(g["t_star"][:, sel]).ravel(), _bits(t_star)), kind
        assert (g["val"][:, sel] < 0).any() and (g["val"][:, sel] > 0).any(), kind
    assert (g["status"] == _capi.MD_OK).all() and (g["nodes"] > 1).any() and (g["nodes"] == 1).any()
    tau0, tau1 = bt["params"][:, 1][None], bt["params"][:, 2][None]
    at_end = (g["t_star"] == tau0) | (g["t_star"] == tau1)
    inside_curve = (g["t_star"] > 0.0) & (g["t_star"] < 1.0)
    assert (at_end & inside_curve).any(), "an extremum at a window end that is interior to the curve"
    assert (at_end & ~inside_curve).any(), "an extremum at tau = 0 or 1"
    assert ((g["t_star"] >= tau0) & (g["t_star"] <= tau1)).all()


# ------------------------------------------------------------------------------------------------ 3. the truth
@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_values_lie_in_the_exact_bracket(dim, deg):
    """Every val lies within the exact-rational bracket [L, H] of the item's row, widened on the side the search leaves open by
    its tolerance eps_rel * max |coefficient| and on both by the rounding allowance K 2^-53 M of proximity_ref.allowance (derived
    from the formation's operation count and majorant, not from any device output):
        within:  L - A <= val <= H + tol + A          reach:  L - tol - A <= val <= H + A"""
    d = device(dim, deg)
    bt, g = d["bt"], d["val"]
    worst = 0.0
    for r in range(B):
        for p, (it, pr) in enumerate(zip(bt["items"], bt["params"])):
            tr = d["cs"]["truth"][r * 8 + p]
            A = PR.allowance(bt["Y"][r], bt["pts"], dim, N, it, pr)
            tol = Fraction(EPS) * Fraction(float(np.abs(d["poly"][r, p]).max()))
            v = Fraction(float(g["val"][r, p]))
            lo, hi = (tr["L"] - A, tr["H"] + tol + A) if it[2] == PR.WITHIN else (tr["L"] - tol - A, tr["H"] + A)
            worst = max(worst, float(max(tr["L"] - v, v - tr["H"], 0) / (tol + A)))
            assert lo <= v <= hi, (r, p, float(lo - v), float(v - hi))
    print("dim %d deg %d: worst (distance outside the exact bracket) / (tol + allowance) = %.3g" % (dim, deg, worst))


# ------------------------------------------------------------------------------------------------ 4. the blocks
@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_blocks_are_the_negated_envelope_block(dim, deg):
    """jac equals the restatement of the negated envelope_block at the returned t_star, bit for bit, on the unrestricted
    control points; a t_star at a curve end leaves one non-zero column."""
    d = device(dim, deg)
    bt, g = d["bt"], d["jac"]
    assert g["jac"].shape == (B, 8, dim, deg + 1)
    for r in range(B):
        for p, it in enumerate(bt["items"]):
            t = float(g["t_star"][r, p])
            want = PR.envelope_float(bt["Y"][r], bt["pts"], dim, N, it, t)
            assert np.array_equal(_bits(g["jac"][r, p]), _bits(want)), (r, p)
            if t in (0.0, 1.0):
                assert (np.delete(g["jac"][r, p], 0 if t == 0.0 else deg, axis=1) == 0.0).all()


@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_blocks_against_a_central_difference_of_the_exact_extremum(dim, deg):
    """On EVERY item of the batch with a unique interior extremum (proximity_ref.unique_interior_items, from the float rows alone;
    test_proximity_ref confirms on the CPU that each configuration holds at least two) the block agrees with a central
    difference of the exact-rational extremum in a's first, middle and last control point of every coordinate.  The bound,
    from CPU-side quantities only: with cd_h the central difference at step h = 2^-8 and cd_h/2 at half of it,
        |jac - cd_h/2| <= |cd_h - cd_h/2|                    (the step: the O(h^2) term of cd_h/2 is a quarter of cd_h's)
                        + 3 d n F dt                         (t_star's resolution: |d block / dt| <= d (n F + 2 n F))
                        + 2 rel s / h                        (the exact brackets' width, rel = 1e-13)
    dt = (tau1 - tau0) 2 sqrt(2 (tol + A) / |g''(t*)|): a value within tol + A of the extremum lies that close to it (the factor
    2 covers the cubic term), g'' from the exact coefficients; F = max_q (max |a_q| + max |b_q|); the call uses eps_rel = 1e-12."""
    from optimalbeziertrajectorygeneration_amd import _capi
    d = device(dim, deg)
    bt = d["bt"]
    eps = 1e-12
    c = _capi.Context(N, dim, deg, 0, device=0)
    try:
        g = c.proximity_true_jac(bt["Y"], (bt["items"], bt["params"], bt["pts"]), eps_rel=eps)
    finally:
        c.close()
    pts = bt["pts"]
    todo = PR.unique_interior_items(bt, d["cs"]["rows"])
    assert len(todo) >= 2
    worst = 0.0
    for r, p in todo:
        y, it, pr = bt["Y"][r], bt["items"][p], bt["params"][p]
        a = int(it[0])
        ex = PR.item_exact(y, pts, dim, N, it, pr)
        tr = PR.extremum_exact(ex, int(it[2]))
        A = PR.allowance(y, pts, dim, N, it, pr)
        tol = Fraction(eps) * tr["s"]
        g2 = abs(PR.second_derivative_exact(ex, tr["t"]))
        dt = (pr[2] - pr[1]) * 2.0 * float(2 * (tol + A) / g2) ** 0.5
        ya, yb, _ = PR._pair(y, pts, dim, N, a, int(it[1]))
        F = max(np.abs(ya[q]).max() + np.abs(yb[q]).max() for q in range(dim))

        def cd(q, i, h):
            f = []
            for sg in (1.0, -1.0):
                y2 = y.copy()
                y2[a * dim + q, i] += sg * h
                t2 = PR.item_truth(y2, pts, dim, N, it, pr)
                f.append((t2["L"] + t2["H"]) / 2)
            return float((f[0] - f[1]) / Fraction(2 * h))
        h = 2.0 ** -8
        for q in range(dim):
            for i in (0, deg // 2, deg):
                c1, c2 = cd(q, i, h), cd(q, i, h / 2)
                bound = abs(c1 - c2) + 3 * dim * deg * F * dt + 2e-13 * float(tr["s"]) / (h / 2)
                err = abs(g["jac"][r, p, q, i] - c2)
                worst = max(worst, err / bound)
                assert err <= bound, (r, p, q, i, err, bound)
    print("dim %d deg %d: %d items, worst |jac - central difference| / bound = %.3g" % (dim, deg, len(todo), worst))


# ------------------------------------------------------------------------------------------------ 5. the forms agree
@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_forms_agree_bit_for_bit(dim, deg, monkeypatch):
    """The value and the _jac calls, the host and the _dev calls (nullable outputs omitted too), B = 1 against the batch, and a
    context created with OBTG_TRUE_MIN_JAC_FUSED=0 give the same bits."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    d = device(dim, deg)
    bt, v, g = d["bt"], d["val"], d["jac"]
    Y = bt["Y"]
    for k in ("val", "t_star", "bound"):
        assert np.array_equal(_bits(v[k]), _bits(g[k])), k
    for k in ("nodes", "status"):
        assert np.array_equal(v[k], g[k]), k
    tables = (bt["items"], bt["params"], bt["pts"])
    monkeypatch.setenv("OBTG_TRUE_MIN_JAC_FUSED", "0")
    c2 = _capi.Context(N, dim, deg, 0, device=0)
    monkeypatch.delenv("OBTG_TRUE_MIN_JAC_FUSED")
    c = _capi.Context(N, dim, deg, 2, device=0)                 # DEG_ELEV does not enter
    try:
        two = c2.proximity_true_jac(Y, tables, eps_rel=EPS)
        for k in ("val", "t_star", "bound", "jac"):
            assert np.array_equal(_bits(two[k]), _bits(g[k])), k
        assert np.array_equal(two["nodes"], g["nodes"]) and np.array_equal(two["status"], g["status"])
        for b in (0, B - 1):
            one = c.proximity_true_jac(Y[b:b + 1], tables, eps_rel=EPS)
            for k in ("val", "t_star", "bound", "jac"):
                assert np.array_equal(_bits(one[k][0]), _bits(g[k][b])), (k, b)
        dev = torch.device("cuda", 0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dY = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
            i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
            dv, dt, db, dn, ds, dj = f64(B, 8), f64(B, 8), f64(B, 8), i32(B, 8), i32(B, 8), f64(B, 8, dim, deg + 1)
            c.proximity_true_dev(dY.data_ptr(), B, dv.data_ptr(), dt.data_ptr(), db.data_ptr(), dn.data_ptr(), ds.data_ptr(),
                                 dj.data_ptr(), eps_rel=EPS)
            dv2, dj2 = f64(B, 8), f64(B, 8, dim, deg + 1)
            c.proximity_true_dev(dY.data_ptr(), B, dv2.data_ptr(), d_jac=dj2.data_ptr(), eps_rel=EPS)
            dv3, dt3 = f64(B, 8), f64(B, 8)
            c.proximity_true_dev(dY.data_ptr(), B, dv3.data_ptr(), dt3.data_ptr(), eps_rel=EPS)
            dp = f64(B, 8, 2 * deg + 1)
            c.proximity_poly_dev(dY.data_ptr(), B, dp.data_ptr())
            torch.cuda.synchronize()
        finally:
            c.use_own_stream()
        for got, k in ((dv, "val"), (dv2, "val"), (dv3, "val"), (dt, "t_star"), (dt3, "t_star"), (db, "bound"), (dj, "jac"), (dj2, "jac")):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(g[k])), k
        assert np.array_equal(dn.cpu().numpy(), g["nodes"]) and np.array_equal(ds.cpu().numpy(), g["status"])
        assert np.array_equal(_bits(dp.cpu().numpy()), _bits(d["poly"]))
        lib, h = c._lib, c._h                                       # the host call with its nullable outputs omitted
        out = np.zeros((B, 8))
        assert lib.obtg_proximity_true(h, _capi._ptr(Y), B, EPS, 100000, _capi._ptr(out), None, None, None, None) == 0
        assert np.array_equal(_bits(out), _bits(g["val"]))
    finally:
        c.close()
        c2.close()


# ------------------------------------------------------------------------------------------------ 6. arguments
@pytest.mark.parametrize("deg", [5, 4])
def test_arguments_and_non_finite_input(deg):
    """Each refusal against its status code; P = 0 clears; degree 32 answers OBTG_ERR_UNSUPPORTED; a NaN control point gives NaN
    val, t_star and bound with status OK and nodes 0 on the items that read it and leaves the other items' bits untouched
    (degree 5 fused, degree 4 through the workspace)."""
    from optimalbeziertrajectorygeneration_amd import _capi
    dim = 2
    d = device(dim, deg)
    bt = d["bt"]
    items, params, pts, Y = bt["items"], bt["params"], bt["pts"], bt["Y"]
    c = _capi.Context(N, dim, deg, 0, device=0)
    try:
        with pytest.raises(_capi.ObtgError) as err:                   # no items set
            c.proximity_true(Y)
        assert err.value.code == ERR_ARG
        with pytest.raises(_capi.ObtgError) as err:
            c.proximity_poly(Y)
        assert err.value.code == ERR_ARG

        def refused(it, pr):
            with pytest.raises(_capi.ObtgError) as e:
                c.set_proximity(np.array([it], np.int32), np.array([pr]), pts)
            assert e.value.code == ERR_ARG, (it, pr)
        ok = [0.5, 0.0, 1.0]
        refused([1, 1, 0], ok)                                        # a == b
        refused([N, 0, 0], ok)                                        # a vehicle index out of range
        refused([-1, 0, 0], ok)
        refused([0, N + PR.N_PTS, 1], ok)                             # a point index out of range
        refused([0, -1, 1], ok)
        refused([0, 1, 2], ok)                                        # a kind that is neither
        for rho in (0.0, -1.0, np.nan, np.inf):
            refused([0, 1, 0], [rho, 0.0, 1.0])
        for w in ((0.5, 0.5), (0.75, 0.25), (-0.25, 0.5), (0.5, 1.25), (np.nan, 1.0), (0.0, np.nan)):
            refused([0, 1, 0], [0.5, w[0], w[1]])
        assert c.len_proximity == 0
        c.set_proximity(items, params, pts)
        assert c.len_proximity == 8
        base = c.proximity_true_jac(Y[:1], eps_rel=EPS)
        for k in ("val", "t_star", "bound", "jac"):
            assert np.array_equal(_bits(base[k][0]), _bits(d["jac"][k][0])), k
        Yn = Y[:1].copy()
        Yn[0, 1 * dim + 1, 2] = np.nan                                # vehicle 1
        g = c.proximity_true_jac(Yn, eps_rel=EPS)
        bad = (items[:, 0] == 1) | (items[:, 1] == 1)
        assert bad.sum() == 4 and (g["status"] == _capi.MD_OK).all()
        for k in ("val", "t_star", "bound"):
            assert np.isnan(g[k][0, bad]).all(), k
            assert np.array_equal(_bits(g[k][0, ~bad]), _bits(base[k][0, ~bad])), k
        assert (g["nodes"][0, bad] == 0).all() and np.array_equal(g["nodes"][0, ~bad], base["nodes"][0, ~bad])
        assert np.isnan(g["jac"][0, bad]).all(axis=(1, 2)).all()
        assert np.array_equal(_bits(g["jac"][0, ~bad]), _bits(base["jac"][0, ~bad]))
        lib, h = c._lib, c._h
        out = np.zeros((1, 8))
        P_ = _capi._ptr
        assert lib.obtg_proximity_true(h, P_(Yn), 1, 1e-9, 100, None, None, None, None, None) == ERR_ARG               # null val
        assert lib.obtg_proximity_true(h, None, 1, 1e-9, 100, P_(out), None, None, None, None) == ERR_ARG              # null Y
        assert lib.obtg_proximity_true(h, P_(Yn), 1, 1e-9, 0, P_(out), None, None, None, None) == ERR_ARG              # max_nodes
        assert lib.obtg_proximity_true(h, P_(Yn), 1, -1.0, 100, P_(out), None, None, None, None) == ERR_ARG            # eps_rel
        assert lib.obtg_proximity_true_jac(h, P_(Yn), 1, 1e-9, 100, P_(out), None, None, None, None, None) == ERR_ARG  # null jac
        assert lib.obtg_proximity_true_dev(h, None, 1, 1e-9, 100, P_(out), None, None, None, None) == ERR_ARG          # no view form
        assert lib.obtg_proximity_poly_dev(h, None, 1, P_(out)) == ERR_ARG
        assert lib.obtg_proximity_poly(h, P_(Yn), 1, None) == ERR_ARG
        c.set_proximity(np.zeros((0, 3), np.int32), np.zeros((0, 3)))   # P = 0 clears
        assert c.len_proximity == 0
        with pytest.raises(_capi.ObtgError) as err:
            c.proximity_true(Y)
        assert err.value.code == ERR_ARG
    finally:
        c.close()
    line = _capi.Context(2, 1, 3, 0, device=0)
    try:
        with pytest.raises(_capi.ObtgError) as err:
            line.set_proximity(np.array([[0, 1, 0]], np.int32), np.array([[0.5, 0.0, 1.0]]))
        assert err.value.code == ERR_ARG
    finally:
        line.close()
    big = _capi.Context(2, 2, 32, 0, device=0)
    try:
        big.set_proximity(np.array([[0, 1, 0]], np.int32), np.array([[0.5, 0.0, 1.0]]))
        for call in (big.proximity_true, big.proximity_true_jac, big.proximity_poly):
            with pytest.raises(_capi.ObtgError) as err:
                call(np.zeros((1, 4, 33)))
            assert err.value.code == ERR_UNSUPPORTED
    finally:
        big.close()


# ------------------------------------------------------------------------------------------------ 7. the Python layer
WAYPOINTS = [(0, (2.5, 6.0), 0.75, (0.0, 0.5)), (1, 0, 4.5, (0.25, 0.75)), (1, (6.0, 6.5), 1.0)]
STAY = [(0, 1, 8.0), (1, (5.0, 5.0), 6.0, (0.5, 1.0))]


def _problem(timeopt=False, **kw):
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    goal = dict(minimizeGoal='TimeOpt') if timeopt else dict(minimizeGoal='Euclidean', tf=10.0)
    return BezOptimization(numVeh=2, dimension=2, degree=5, maxSep=1, maxSpeed=5, initPoints=[(0, 5), (3, 0)],
                           finalPoints=[(8, 4), (7, 10)], **goal, **kw)


def test_python_closure_accessor_and_providers():
    """proximityConstraints is the raw call and trueProximityMargins's val, both inside the exact bracket; the envelope provider
    is the device's blocks scattered with +1 to the entry's vehicle and -1 to a vehicle target (a point has none); against
    method='fd' (h = FD_STEP) row by row on a guess whose rows the CPU confirms to have one basin each: the device's gap may be
    the yardstick's own gap between its envelope block at the exact t* and the forward difference of the exact extremum with
    the same h (that gap holds the difference's truncation error), plus the search slack 2 eps_rel s / h of the device's
    difference quotient: each of its two values may sit eps_rel s off the true extremum.  _serve_key gains one trailing
    entry only while a list is set; the tf column of a time-optimal problem is an exact 0; Bezier.proximityMargin gives the
    same values for both kinds and for a curve target."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    from optimalbeziertrajectorygeneration_amd import bezier
    bo = _problem(waypoints=WAYPOINTS, stayWithin=STAY)
    none = _problem()
    x = bo.generateGuess(std=2.0, seed=19)          # (chosen on the CPU: every row of this guess has one interior basin)
    Nv, dim, deg = 2, 2, 5
    items, params, pts = opt._proximity_tables(WAYPOINTS, STAY, Nv, dim)
    P = len(items)
    assert P == 5 and items[:, 2].tolist() == [1, 1, 1, 0, 0] and pts.shape == (3, 2)
    Y = bo.reshapeVector(x)
    raw = bo._ctx(False).proximity_true_jac(Y[None], (items, params, pts), eps_rel=bo.TRUE_MIN_EPS_REL)
    rows = bo.proximityConstraints(x)
    val, t_star = bo.trueProximityMargins(x)
    assert rows.shape == (P,) and np.array_equal(_bits(rows), _bits(raw["val"][0])) and np.array_equal(_bits(val), _bits(rows))
    assert np.array_equal(_bits(t_star), _bits(raw["t_star"][0]))
    float_rows = PR.rows_float(Y[None], pts, dim, Nv, items, params)[0]
    truth = []
    for p in range(P):
        tr = PR.item_truth(Y, pts, dim, Nv, items[p], params[p])
        truth.append(tr)
        A = PR.allowance(Y, pts, dim, Nv, items[p], params[p])
        tol = Fraction(bo.TRUE_MIN_EPS_REL) * tr["s"]
        v = Fraction(float(rows[p]))
        lo, hi = (tr["L"] - A, tr["H"] + tol + A) if items[p, 2] == PR.WITHIN else (tr["L"] - tol - A, tr["H"] + A)
        assert lo <= v <= hi, p
        assert PR.unique_interior(float_rows[p], int(items[p, 2]))[0], "row %d of the guess must have one interior basin" % p
    # _serve_key
    key = bo._serve_key(True)
    bo.waypoints, bo.stayWithin = None, None
    without = bo._serve_key(True)
    bo.waypoints, bo.stayWithin = WAYPOINTS, STAY
    assert key[-1][0] == 'proximity' and without == key[:-1] and len(without) == len(none._serve_key(True))
    assert bo._serve_key(True) == key
    for call in (none.proximityConstraints, none.proximityJacobian, none.trueProximityMargins):
        with pytest.raises(ValueError, match="waypoints/stayWithin is None"):
            call(x)
    with pytest.raises(ValueError, match="not built for the proximity rows"):
        bo.proximityJacobian(x, method='exact')
    # the providers
    Je, Jf = bo.proximityJacobian(x, method='envelope'), bo.proximityJacobian(x, method='fd')
    first, cols = bo._rv_parts()[1], bo._numCols
    want = PR.scatter(raw["jac"][0], items, Nv, dim, first, cols)
    assert Je.shape == Jf.shape == (P, x.size) and np.array_equal(_bits(Je), _bits(want))
    per = dim * cols
    assert np.array_equal(Je[1, :per], -Je[1, per:]) and Je[1].any(), "a vehicle target: the second vehicle's block is the negation"
    assert not Je[0, per:].any() and Je[0, :per].any(), "a point target: only the entry's own vehicle"
    X, dx = bo._fd_rows(x)
    Ys = bo.reshapeVectors(X)
    worst = 0.0
    for p in range(P):
        tr = truth[p]
        ref_env = PR.scatter([PR.envelope_float(Y, pts, dim, Nv, items[p], PR.curve_t(float(tr["t"]), params[p, 1], params[p, 2]))
                              if q == p else np.zeros((dim, deg + 1)) for q in range(P)], items, Nv, dim, first, cols)[p]
        mid0 = (tr["L"] + tr["H"]) / 2
        ref_fd = np.zeros(x.size)
        for k in range(x.size):
            t2 = PR.item_truth(Ys[k + 1], pts, dim, Nv, items[p], params[p])
            ref_fd[k] = float(((t2["L"] + t2["H"]) / 2 - mid0) / Fraction(float(dx[k])))
        ref_gap = float(np.abs(ref_env - ref_fd).max())
        gap = float(np.abs(Je[p] - Jf[p]).max())
        bound = ref_gap + 2.0 * bo.TRUE_MIN_EPS_REL * float(tr["s"]) / float(dx.min())
        worst = max(worst, gap / bound)
        print("row %d: device |envelope - fd| %.3e, yardstick's %.3e, bound %.3e" % (p, gap, ref_gap, bound))
        assert gap <= bound, p
    print("worst |envelope - fd| / bound = %.3g" % worst)
    # a time-optimal problem: the rows do not depend on tf
    to = _problem(timeopt=True, waypoints=WAYPOINTS, stayWithin=STAY)
    xt = to.generateGuess(std=1.0, seed=3)
    xt[-1] = 10.0
    Jte, Jtf = to.proximityJacobian(xt, method='envelope'), to.proximityJacobian(xt, method='fd')
    assert Jte.shape == (P, xt.size) and not Jte[:, -1].any() and not Jtf[:, -1].any() and Jte[:, :-1].any()
    # Bezier.proximityMargin
    c0, c1 = bezier.Bezier(Y[:dim], tf=10.0), bezier.Bezier(Y[dim:], tf=10.0)
    assert c0.proximityMargin(WAYPOINTS[0][1], 0.75, 'reach', (0.0, 0.5), eps=bo.TRUE_MIN_EPS_REL) == (rows[0], t_star[0])
    assert c1.proximityMargin(c0, 4.5, 'reach', (0.25, 0.75), eps=bo.TRUE_MIN_EPS_REL) == (rows[1], t_star[1])
    assert c0.proximityMargin(c1, 8.0, 'within', eps=bo.TRUE_MIN_EPS_REL) == (rows[3], t_star[3])
    assert c1.proximityMargin((5.0, 5.0), 6.0, 'within', (0.5, 1.0), eps=bo.TRUE_MIN_EPS_REL) == (rows[4], t_star[4])
    with pytest.raises(ValueError, match="kind must be"):
        c0.proximityMargin((0.0, 0.0), 1.0, 'near')
    with pytest.raises(ValueError, match="same dimension, degree and span"):
        c0.proximityMargin(bezier.Bezier(Y[:dim], tf=5.0), 1.0)


# ------------------------------------------------------------------------------------------------ 8. one SLSQP solve
def test_solve_through_one_gate_each():
    """Two cars at degree 5, one gate each, which the solve without waypoints misses by more than the radius: both constrained
    solves succeed and end with every row >= -1e-9 * scale, judged by the exact-rational layer at the returned x (H, the upper
    end of the row's exact bracket; scale = the largest coefficient of the row's exact polynomial), not by the device."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
    import example26_waypoints_and_range as ex
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    gates = [ex.GATES[0][:3], ex.GATES[2][:3]]
    _, free = ex.solve(None, degree=5)
    _, _, d_free = ex.margins(free.x, 5, gates, None)
    assert free.success and (d_free > 2 * ex.RADIUS).all(), "the solve without waypoints must miss both gates by more than the radius"
    items, params, pts = opt._proximity_tables(gates, None, 2, 2)
    for method in ('fd', 'envelope'):
        bo, res = ex.solve(method, degree=5, x0=free.x, waypoints=gates, stay_within=None)
        Y = bo.reshapeVector(res.x)
        worst = None
        for p in range(2):
            tr = PR.item_truth(Y, pts, 2, 2, items[p], params[p])
            worst = tr["H"] / tr["s"] if worst is None else min(worst, tr["H"] / tr["s"])
            assert tr["H"] >= -Fraction(1, 10 ** 9) * tr["s"], (method, p, float(tr["H"]), float(tr["s"]))
        print("%s: objective %.9f against %.9f without gates, %d iterations, status %d, smallest exact row / scale %.3e; the free "
              "solve passes %.3f and %.3f from the gates" % (method, res.fun, free.fun, res.nit, res.status, float(worst), d_free[0], d_free[1]))
        assert res.success, (method, res.message)
