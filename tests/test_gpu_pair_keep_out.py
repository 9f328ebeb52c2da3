"""The polytopic vehicle-to-vehicle separation rows on the device (obtg_pair_keep_out[_euclid]_true_min[_jac][_dev];
BezOptimization(separationRegion=...)) against the STATIC keep-out calls on the relative curves, bit for bit, and against the
yardstick of tests/pair_keep_out_ref.py.  A batch is N = 4 vehicles (P = 6 pairs), B = 5 rows: 30 items a call; what the batches
hold (negative rows, searches that split) and how many provider rows are generic is confirmed on the CPU
(tests/test_pair_keep_out_ref.py).  DESIGN.md 4.27."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import pair_keep_out_ref as ref  # noqa: E402

N, B = ref.N_VEH, ref.B_ROWS
P = N * (N - 1) // 2
EPS = 1e-12
ERR_ARG, ERR_UNSUPPORTED = -1, -5
KEYS = {"faces": ("val", "t_star", "face", "lam", "bound", "nodes", "status"),
        "euclidean": ("val", "t_star", "faces", "dir", "bound", "nodes", "status")}
CASES = [(dim, metric) for dim in (2, 3) for metric in ref.METRICS]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _pair(ctx, metric, jac):
    return getattr(ctx, "pair_keep_out_%strue_min%s" % ("euclid_" if metric == "euclidean" else "", "_jac" if jac else ""))


def _static(ctx, metric, jac):
    return getattr(ctx, "keep_out_%strue_min%s" % ("euclid_" if metric == "euclidean" else "", "_jac" if jac else ""))


def _static_tables(H, n):
    """the region as the one obstacle of n vehicles: VO = (p, 0)"""
    return H, np.array([0, len(H)], np.int32), np.stack((np.arange(n), np.zeros(n, int)), axis=1).astype(np.int32)


def _numpy_rel(Y, n_veh, dim):
    pa, pb = np.triu_indices(n_veh, 1)
    V = Y.reshape(Y.shape[0], n_veh, dim, -1)
    return V[:, pa] - V[:, pb]


# ------------------------------------------------------------------------------------------------ 1, 2. rel, pair order, identity
@pytest.mark.gpu
@pytest.mark.parametrize("deg", ref.DEGREES)
@pytest.mark.parametrize("dim,metric", CASES)
def test_rel_and_identity_with_the_static_call(dim, metric, deg):
    """rel is Y_i - Y_j as NumPy forms it, bit for bit, in the order of np.triu_indices; and EVERY output of the pair call equals
    the static call of the same metric on a context of P vehicles whose control points are the rows of rel, the region their one
    obstacle -- bit for bit, all 30 items.  Per case an item with nodes > 1 and one with a negative row."""
    from optimalbeziertrajectorygeneration_amd import _capi
    Y = ref.batch(deg, dim, ref.seed_of(deg, dim))
    pair_ctx, static_ctx = _capi.Context(N, dim, deg, 0, device=0), _capi.Context(P, dim, deg, 0, device=0)
    try:
        for name, make in ref.REGIONS[dim]:
            H = make()
            r = _pair(pair_ctx, metric, True)(Y, H, eps_rel=EPS)
            assert pair_ctx.len_pair_keep_out == P and r["val"].shape == (B, P)
            want = _numpy_rel(Y, N, dim)
            assert np.array_equal(_bits(r["rel"]), _bits(want)), (name, "rel")
            s = _static(static_ctx, metric, True)(np.ascontiguousarray(r["rel"].reshape(B, P * dim, deg + 1)), _static_tables(H, P),
                                                  eps_rel=EPS)
            _same(r, s, KEYS[metric] + ("jac",), (name, metric, deg))
            assert (r["status"] == 0).all() and np.isfinite(r["val"]).all() and np.isfinite(r["jac"]).all()
            assert (r["nodes"] > 1).any() and (r["val"] < 0.0).any(), (name, metric, deg)
            assert (r["bound"] <= r["val"]).all()
    finally:
        pair_ctx.close()
        static_ctx.close()


# ------------------------------------------------------------------------------------------------ 3. agreement between forms
def _dev_call(ctx, torch, Y, dim, deg, metric, jac):
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        Bn = Y.shape[0]
        dY = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
        eu = metric == "euclidean"
        d = {"val": f64(Bn, P), "t_star": f64(Bn, P), ("faces" if eu else "face"): i32(Bn, P, 3 if eu else 2),
             ("dir" if eu else "lam"): f64(Bn, P, dim) if eu else f64(Bn, P), "bound": f64(Bn, P), "nodes": i32(Bn, P),
             "status": i32(Bn, P), "rel": f64(Bn, P, dim, deg + 1)}
        if jac:
            d["jac"] = f64(Bn, P, dim, deg + 1)
        k = KEYS[metric]
        ctx.pair_keep_out_true_min_dev(dY.data_ptr(), Bn, d["val"].data_ptr(), d["t_star"].data_ptr(), d[k[2]].data_ptr(),
                                       d[k[3]].data_ptr(), d["bound"].data_ptr(), d["nodes"].data_ptr(), d["status"].data_ptr(),
                                       d["rel"].data_ptr(), d["jac"].data_ptr() if jac else None, euclid=eu, eps_rel=EPS)
        v2 = f64(Bn, P)                                                     # the value call, every nullable output omitted
        ctx.pair_keep_out_true_min_dev(dY.data_ptr(), Bn, v2.data_ptr(), euclid=eu, eps_rel=EPS)
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    out = {key: x.cpu().numpy() for key, x in d.items()}
    out["val_only"] = v2.cpu().numpy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dim,metric", CASES)
def test_forms_agree(dim, metric):
    """The value call and the _jac call, the host and the _dev calls, and a row alone (B = 1): bit for bit."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    deg = 5
    Y = ref.batch(deg, dim, ref.seed_of(deg, dim))
    H = ref.REGIONS[dim][1][1]()                    # the region without symmetry
    keys = KEYS[metric] + ("rel",)
    ctx = _capi.Context(N, dim, deg, 0, device=0)
    try:
        rj = _pair(ctx, metric, True)(Y, H, eps_rel=EPS)
        rv = _pair(ctx, metric, False)(Y, eps_rel=EPS)           # (the region stays on the context)
        _same(rj, rv, keys, "value call")
        assert "jac" not in rv
        for jac in (False, True):
            d = _dev_call(ctx, torch, Y, dim, deg, metric, jac)
            _same(rj, d, keys + (("jac",) if jac else ()), "_dev, jac %s" % jac)
            assert np.array_equal(_bits(d["val_only"]), _bits(rj["val"]))
        for b in (0, B - 1):
            one = _pair(ctx, metric, True)(Y[b:b + 1], eps_rel=EPS)
            for k in keys + ("jac",):
                assert np.array_equal(_bits(one[k][0]), _bits(rj[k][b])), ("row alone", b, k)
        shifted = _pair(ctx, metric, False)(Y, margin=0.25, eps_rel=EPS)
        assert np.array_equal(_bits(shifted["val"]), _bits(rj["val"] - 0.25)) and np.array_equal(_bits(shifted["t_star"]), _bits(rj["t_star"]))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. edge cases
@pytest.mark.gpu
@pytest.mark.parametrize("dim,metric", CASES)
def test_nan_vehicle_identical_vehicles_and_one_vehicle(dim, metric):
    from optimalbeziertrajectorygeneration_amd import _capi
    deg = 3
    Y = ref.batch(deg, dim, ref.seed_of(deg, dim))
    H = ref.REGIONS[dim][0][1]()
    pa, pb = np.triu_indices(N, 1)
    keys = KEYS[metric] + ("rel", "jac")
    ctx = _capi.Context(N, dim, deg, 0, device=0)
    try:
        good = _pair(ctx, metric, True)(Y, H, eps_rel=EPS)
        # a NaN in vehicle 2 of row 1, an infinity in vehicle 0 of row 3: exactly the pairs that contain them
        Yb = Y.copy()
        Yb[1, 2 * dim, 1] = np.nan
        Yb[3, 0 * dim + dim - 1, deg] = np.inf
        r = _pair(ctx, metric, True)(Yb, eps_rel=EPS)
        hit = np.zeros((B, P), bool)
        hit[1] = (pa == 2) | (pb == 2)
        hit[3] = (pa == 0) | (pb == 0)
        assert hit.sum() == 6
        fk = KEYS[metric][2]
        for k in ("val", "t_star", "bound", KEYS[metric][3], "rel", "jac"):
            assert np.isnan(r[k][hit]).all(), k
        assert (r[fk][hit] == -1).all() and (r["nodes"][hit] == 0).all() and (r["status"] == 0).all()
        for k in keys:
            assert np.array_equal(_bits(r[k][~hit]), _bits(good[k][~hit])), k
        # two identical vehicles: D = 0, the origin: max_f (-b_f) - margin exactly (the normalised b under the Euclidean metric)
        Yi = Y.copy()
        Yi[2].reshape(N, dim, deg + 1)[3] = Yi[2].reshape(N, dim, deg + 1)[1]
        margin = 0.125
        r = _pair(ctx, metric, False)(Yi, margin=margin, eps_rel=EPS)
        p13 = int(np.flatnonzero((pa == 1) & (pb == 3))[0])
        b_f = H[:, -1] / (np.linalg.norm(H[:, :-1], axis=1) if metric == "euclidean" else 1.0)
        assert r["val"][2, p13] == np.max(-b_f) - margin and r["t_star"][2, p13] == 0.0 and r["nodes"][2, p13] == 1
        assert (r["rel"][2, p13] == 0.0).all()
    finally:
        ctx.close()
    one = _capi.Context(1, dim, deg, 0, device=0)                        # N = 1: P = 0, OBTG_OK, nothing written
    try:
        one.set_pair_keep_out(H)
        assert one.len_pair_keep_out == 0
        r = _pair(one, metric, True)(np.zeros((2, dim, deg + 1)), eps_rel=EPS)
        assert r["val"].shape == (2, 0) and r["jac"].shape == (2, 0, dim, deg + 1)
    finally:
        one.close()


@pytest.mark.gpu
def test_error_codes_and_independence_of_the_obstacle_tables():
    """No region, a context whose d is 1: OBTG_ERR_ARG; more than 16 faces, K > 32: OBTG_ERR_UNSUPPORTED; more than 128 features:
    OBTG_ERR_UNSUPPORTED from the Euclidean pair calls only; F = 0 clears.  keepOut tables and a motion on the same context do not
    disturb the pair rows, and the region does not disturb theirs."""
    import math
    import keep_out_ref as K
    from optimalbeziertrajectorygeneration_amd import _capi
    deg, dim = 3, 2
    Y = ref.batch(deg, dim, 7)
    H = ref.oblique_triangle()
    ctx = _capi.Context(N, dim, deg, 0, device=0)
    try:
        for metric in ref.METRICS:
            with pytest.raises(_capi.ObtgError) as e:
                _pair(ctx, metric, False)(Y)
            assert e.value.code == ERR_ARG                                   # no region
        assert ctx.len_pair_keep_out == 0
        with pytest.raises(_capi.ObtgError) as e:
            ctx.set_pair_keep_out(np.hstack((np.ones((17, 2)), np.ones((17, 1)))))
        assert e.value.code == ERR_UNSUPPORTED                               # 17 faces
        for bad in (0.0, -1.0):
            Hb = H.copy()
            Hb[1, -1] = bad
            with pytest.raises(_capi.ObtgError) as e:
                ctx.set_pair_keep_out(Hb)
            assert e.value.code == ERR_ARG                                   # the origin is not strictly inside
        assert ctx.len_pair_keep_out == 0
        good = {m: _pair(ctx, m, True)(Y, H, eps_rel=EPS) for m in ref.METRICS}
        assert ctx.len_pair_keep_out == P
        # obstacle tables and a motion on the same context: the pair rows keep their bits, and so do the obstacle rows
        obs = K.tables(K.obstacles(dim), N)
        before = ctx.keep_out_true_min(Y, obs, eps_rel=EPS)
        ctx.set_keep_out_motion(np.zeros((dim, 2)).ravel(), np.array([0, 2, 2], np.int32), np.array([1.0, 1.0]))
        for m in ref.METRICS:
            _same(_pair(ctx, m, True)(Y, eps_rel=EPS), good[m], KEYS[m] + ("rel", "jac"), "beside keepOut and a motion")
        ctx.set_keep_out(*obs)                                               # (new tables: the motion is gone)
        ctx.set_pair_keep_out(ref.unit_square())
        ctx.set_pair_keep_out(H)
        _same(ctx.keep_out_true_min(Y, eps_rel=EPS), before, KEYS["faces"], "keepOut beside the region")
        # a NaN face: NaN rows, status OK
        Hn = H.copy()
        Hn[0, 0] = np.nan
        r = ctx.pair_keep_out_true_min(Y, Hn, eps_rel=EPS)
        assert np.isnan(r["val"]).all() and (r["status"] == 0).all() and (r["nodes"] == 0).all()
        ctx.set_pair_keep_out(np.zeros((0, dim + 1)))                        # F = 0 clears
        assert ctx.len_pair_keep_out == 0
        with pytest.raises(_capi.ObtgError) as e:
            ctx.pair_keep_out_true_min(Y)
        assert e.value.code == ERR_ARG
    finally:
        ctx.close()
    ctx = _capi.Context(N, 1, deg, 0, device=0)                              # a context whose d is 1
    try:
        with pytest.raises(_capi.ObtgError) as e:
            ctx.set_pair_keep_out(np.array([[1.0, 1.0], [-1.0, 1.0]]))
        assert e.value.code == ERR_ARG
        with pytest.raises(_capi.ObtgError) as e:
            ctx.pair_keep_out_true_min(np.zeros((1, N, deg + 1)))
        assert e.value.code == ERR_ARG
    finally:
        ctx.close()
    ctx = _capi.Context(2, 2, 32, 0, device=0)                               # K = 33
    try:
        ctx.set_pair_keep_out(ref.unit_square())
        for metric in ref.METRICS:
            with pytest.raises(_capi.ObtgError) as e:
                _pair(ctx, metric, False)(np.zeros((1, 4, 33)))
            assert e.value.code == ERR_UNSUPPORTED
    finally:
        ctx.close()
    # more than 128 features (a many-sided pyramid around the origin), 3-D: the Euclidean pair calls only
    k = 15
    th = 2 * math.pi * np.arange(k) / k
    Hp = np.vstack((np.column_stack((np.cos(th), np.sin(th), np.full(k, 0.5), np.ones(k))), [[0.0, 0.0, -1.0, 1.0]]))
    Y3 = ref.batch(deg, 3, 8)
    ctx = _capi.Context(N, 3, deg, 0, device=0)
    try:
        ctx.set_pair_keep_out(Hp)                                            # the setter takes it
        assert (ctx.pair_keep_out_true_min(Y3)["status"] == 0).all()         # and so does the faces metric
        for call in (ctx.pair_keep_out_euclid_true_min, ctx.pair_keep_out_euclid_true_min_jac):
            with pytest.raises(_capi.ObtgError) as e:
                call(Y3)
            assert e.value.code == ERR_UNSUPPORTED
        assert (ctx.pair_keep_out_euclid_true_min(Y3, ref.box113())["status"] == 0).all()     # a new region: new tables
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. Python rules
@pytest.mark.gpu
def test_python_rules():
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    sq = ref.unit_square()
    A, b = sq[:, :2], sq[:, 2]
    kw = dict(numVeh=2, degree=3, minimizeGoal='Euclidean', maxSep=0.5, tf=1.0)
    kw2 = dict(dimension=2, initPoints=[(3, 3), (0, 0)], finalPoints=[(4, 4), (1, 5)], **kw)
    for bad_b in (np.array([1.0, 1.0, 0.0, 1.0]), np.array([1.0, -1.0, 1.0, 1.0]), np.array([1.0, np.inf, 1.0, 1.0]),
                  np.array([1.0, np.nan, 1.0, 1.0])):
        with pytest.raises(ValueError, match="finite and > 0"):
            BezOptimization(separationRegion=(A, bad_b), **kw2)
    for bad in ((A,), (A, np.ones(3)), (np.ones((4, 3)), b), [(A, b)], (np.ones((17, 2)), np.ones(17))):
        with pytest.raises(ValueError):
            BezOptimization(separationRegion=bad, **kw2)
    with pytest.raises(ValueError, match="dimension 2 or 3"):
        BezOptimization(dimension=1, initPoints=[(3,), (0,)], finalPoints=[(4,), (1,)], separationRegion=(np.ones((1, 1)), np.ones(1)), **kw)
    with pytest.raises(ValueError, match="'faces' or 'euclidean'"):
        BezOptimization(separationRegion=(A, b), separationRegionMetric='round', **kw2)
    with pytest.raises(ValueError, match="finite"):
        BezOptimization(separationRegion=(A, b), separationRegionMargin=np.nan, **kw2)
    bo = BezOptimization(separationRegion=(A, b), **kw2)
    x = bo.generateGuess(std=0)
    with pytest.raises(ValueError, match="not built for the separation-region rows"):
        bo.separationRegionJacobian(x, method='exact')
    with pytest.raises(ValueError):
        bo.separationRegionJacobian(x, method='central')
    none = BezOptimization(**kw2)
    for call in (none.separationRegionConstraints, none.separationRegionJacobian, none.trueSeparationRegionClearances):
        with pytest.raises(ValueError, match="separationRegion is None"):
            call(x)
    # _serve_key: one trailing entry, only while the region is set -- its bytes, the margin and the metric
    key = bo._serve_key(True)
    assert key[-1] == ('separationRegion', sq.tobytes(), 0.0, 'faces')
    bo.separationRegion = None                      # (on the same object: a key holds the identities of the model's arrays)
    without = bo._serve_key(True)
    assert without == key[:-1] and len(without) == len(none._serve_key(True))
    bo.separationRegion = (A, b)
    bo.separationRegionMetric = 'euclidean'
    assert bo._serve_key(True)[-1][-1] == 'euclidean' and bo._serve_key(True)[:-1] == without
    bo.separationRegionMargin = 0.5
    assert bo._serve_key(True)[-1][2] == 0.5
    bo.separationRegionMetric = 'round'             # edited in place afterwards
    with pytest.raises(ValueError, match="'faces' or 'euclidean'"):
        bo.separationRegionConstraints(x + 1e-3)


# ------------------------------------------------------------------------------------------------ 6. providers
def _scatter_pairs(bo, blk, D):
    """Dense [P][n_x] from the first vehicle's blocks [P][dim][n + 1]: +block in vehicle i's free columns, -block in vehicle j's;
    D (time-optimal): the tf column, the blocks along dY/dtf of both vehicles"""
    Nv, dim = bo.model['numVeh'], bo.model['dim']
    first, cols = bo._rv_parts()[1], bo._numCols
    pa, pb = np.triu_indices(Nv, 1)
    J = np.zeros((pa.size, Nv * dim * cols))
    for p, (i, j) in enumerate(zip(pa, pb)):
        free = blk[p][:, first:first + cols].reshape(-1)
        J[p, i * dim * cols:(i + 1) * dim * cols] = free
        J[p, j * dim * cols:(j + 1) * dim * cols] = -free
    if D is None:
        return J
    D = np.asarray(D, dtype=np.float64).reshape(Nv, dim, -1)
    col = np.array([float((blk[p] * (D[i] - D[j])).sum()) for p, (i, j) in enumerate(zip(pa, pb))])
    return np.hstack((J, col[:, None]))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("name", sorted(ref.PROBLEMS))
def test_closure_providers_and_envelope_against_fd(name, metric):
    """Planar degree 5, three vehicles, prescribed speeds, time-optimal, the square; space degree 6, three vehicles, the box.  The
    closure is the raw call's val; the accessor its outputs; the envelope provider the raw blocks scattered with +1 and -1, its tf
    column dY/dtf alone; 'envelope' against 'fd' on every generic row with the acceptance of the keep-out provider tests: the
    device's gap may be twice the yardstick's own gap (its block against its forward difference, same h, same input) plus 1e-9.
    Measured on the MI355X: planar faces 1.255e-04 (the yardstick's own 1.255e-04), planar Euclidean 9.35e-08 (9.35e-08), space
    2.544e-04 (2.544e-04) under both metrics; 3 of 3 rows compared in each."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    bo, x = ref.provider_input(name, separationRegionMetric=metric)
    Nv, dim, deg = bo.model['numVeh'], bo.model['dim'], bo.model['deg']
    H = opt._separation_region_table(bo.separationRegion, dim)
    pa, pb = np.triu_indices(Nv, 1)
    Pn = pa.size
    Y = bo.reshapeVector(x)
    raw = _pair(bo._ctx(False), metric, True)(Y[None], H, eps_rel=bo.TRUE_MIN_EPS_REL)
    rows = bo.separationRegionConstraints(x)
    assert rows.shape == (Pn,) and np.array_equal(_bits(rows), _bits(raw["val"][0]))
    acc = bo.trueSeparationRegionClearances(x)
    want_keys = ("val", "t_star") + KEYS[metric][2:4] + ("status",)
    assert set(acc) == set(want_keys)
    for k in want_keys:
        assert np.array_equal(_bits(acc[k]), _bits(raw[k][0])), k
    shifted = ref.provider_input(name, separationRegionMetric=metric, separationRegionMargin=0.125)[0]
    assert np.array_equal(_bits(shifted.separationRegionConstraints(x)), _bits(raw["val"][0] - 0.125))
    Je, Jf = bo.separationRegionJacobian(x, method='envelope'), bo.separationRegionJacobian(x, method='fd')
    assert Je.shape == Jf.shape == (Pn, x.size) and np.isfinite(Je).all()
    D = bo._dY_dtf() if bo._timeopt() else None
    want = _scatter_pairs(bo, raw["jac"][0], D)
    assert np.array_equal(_bits(Je), _bits(want)) or np.abs(Je - want).max() <= 1e-15
    if D is not None:                               # the explicit tf part is an exact 0: the column is dY/dtf alone
        Dv = np.asarray(D).reshape(Nv, dim, -1)
        col = np.array([float((raw["jac"][0][p] * (Dv[i] - Dv[j])).sum()) for p, (i, j) in enumerate(zip(pa, pb))])
        assert np.abs(Je[:, -1] - col).max() <= 1e-15
    reg = ref.Region(H, metric)
    cols = bo._numCols
    n_pts = Nv * dim * cols
    X, dx = bo._fd_rows(x)
    Ys = bo.reshapeVectors(X)
    V0 = ref.vehicles(Y, Nv)
    compared, worst, worst_ref = 0, 0.0, 0.0
    for p, (i, j) in enumerate(zip(pa, pb)):
        D0 = ref.relative(V0[i], V0[j])
        if not reg.generic(D0, bo.TRUE_MIN_EPS_REL):
            continue
        compared += 1
        r0 = reg.search(D0, bo.TRUE_MIN_EPS_REL)
        blk = reg.block(D0, r0)
        ref_env = _scatter_pairs(bo, [blk if q == p else np.zeros((dim, deg + 1)) for q in range(Pn)], D)[p]
        ref_fd = np.zeros(x.size)
        for k in range(x.size):
            if k < n_pts and k // (dim * cols) not in (i, j):
                continue
            Vk = ref.vehicles(Ys[k + 1], Nv)
            ref_fd[k] = (reg.search(ref.relative(Vk[i], Vk[j]), bo.TRUE_MIN_EPS_REL)["val"] - r0["val"]) / dx[k]
        ref_gap = float(np.abs(ref_env - ref_fd).max())
        gap = float(np.abs(Je[p] - Jf[p]).max())
        worst, worst_ref = max(worst, gap), max(worst_ref, ref_gap)
        print("%s, %s, row %d: device |envelope - fd| %.3e, yardstick's %.3e" % (name, metric, p, gap, ref_gap))
        assert gap <= 2.0 * ref_gap + 1e-9, (name, metric, p)
    print("%s, %s: largest device gap %.3e, largest yardstick gap %.3e, %d of %d rows compared" % (name, metric, worst, worst_ref, compared, Pn))
    assert 2 * compared >= Pn


# ------------------------------------------------------------------------------------------------ 7. the example
@pytest.mark.gpu
def test_example_downwash_boxes():
    """example25: the maxSep-only solution violates the box (a negative region row); both box solves -- the fd and the envelope
    Jacobian -- end with every region row >= -1e-8.  SLSQP is local: the objectives and iteration counts are printed, not asserted."""
    import example25_downwash_boxes as ex
    sphere, fd, env = ex.run()
    rs, rf, re_ = ex.region_rows(sphere.x), ex.region_rows(fd.x), ex.region_rows(env.x)
    for what, res, rows in (("maxSep alone", sphere, rs), ("box, fd", fd, rf), ("box, envelope", env, re_)):
        print("%s: objective %.9f, %d iterations, status %d, box rows %s" % (what, res.fun, res.nit, res.status, rows.tolist()))
    assert rs.min() < 0.0
    assert (rf >= -1e-8).all() and (re_ >= -1e-8).all()
