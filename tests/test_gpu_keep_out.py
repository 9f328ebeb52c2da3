"""The keep-out rows and their envelope Jacobian on the device (obtg_keep_out_true_min[_jac], obtg_bern_keep_out,
BezOptimization(keepOut=.., keepOutMargin=..), keepOutJacobian, trueKeepOutClearances, Bezier.keepOutClearance) against the
yardstick of tests/keep_out_ref.py.  Every device case is N = 3 vehicles, B = 5 rows, every vehicle against two obstacles --
planar: the unit square and an oblique triangle; in space: a box and a tetrahedron (test_keep_out_ref.shared: the seeds are
chosen there, on the CPU, so that every batch holds a kink, a smooth interior minimum, an end minimiser, a penetrating item
and a far item)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import keep_out_ref as K  # noqa: E402
import test_keep_out_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

N, B = T.N, T.B
ERR_ARG = -1
EPS = 1e-12
KEYS = ("val", "t_star", "face", "lam", "bound", "nodes", "status")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _curve(Y, b, v, dim):
    return Y[b, v * dim:(v + 1) * dim]


# ------------------------------------------------------------------------------------------------ 1. values, identity, blocks
@pytest.mark.parametrize("dim", T.DIMS)
@pytest.mark.parametrize("deg", T.DEGS)
def test_values_identity_and_blocks(deg, dim):
    """Value: val + margin is max_f g_f(t_star) in exact rationals within K 2^-53 M (keep_out_ref.value_allowance: K = d + n D
    for the dyadic t_star = k / 2^D); bound <= the yardstick's minimum <= val up to that rounding; val - bound <= tol; the
    yardstick's own search within 2 tol.  Identity: the same bits from the value and the _jac call, host and _dev, a row alone
    and B = 1, obtg_bern_keep_out on the same curve; a margin moves val and bound only.  Blocks: within 1e-9 of the
    exact-rational block at the device's own (t_star, face, lam); lam within 1e-9 of the exact weights there; the faces are
    the exact rule's on generic items; exact zeros off an end minimiser's column; every batch holds a kink whose block is
    not within 1e-3 of either one-face block (a kink whose weights are 0.9999 and 0.0001 is within it, rightly)."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    Y, obs, H, off, VO, rep = T.shared(deg, dim)
    P = VO.shape[0]
    ctx = _capi.Context(N, dim, deg, 2, device=0)                       # (DEG_ELEV = 2: it does not enter)
    try:
        assert ctx.len_keep_out == 0
        ctx.set_keep_out(H, off, VO)
        assert ctx.len_keep_out == P
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        g = ctx.keep_out_true_min_jac(Y, eps_rel=EPS)
        stats = ctx.kernel_stats()
        ctx.set_profiling(False)
        assert stats["speed"][1] == 1 and sum(n for _, n in stats.values()) == 1, stats
        v = ctx.keep_out_true_min(Y, (H, off, VO), eps_rel=EPS)
        assert g["jac"].shape == (B, P, dim, deg + 1) and g["val"].shape == (B, P) and g["face"].shape == (B, P, 2)
        _same(g, v, KEYS, "the _jac call against the value call")
        assert (g["status"] == _capi.MD_OK).all()
        m = ctx.keep_out_true_min_jac(Y, margin=0.25, eps_rel=EPS)
        _same(m, g, ("t_star", "face", "lam", "nodes", "status", "jac"), "a margin")
        assert np.array_equal(m["val"], g["val"] - 0.25) and np.array_equal(m["bound"], g["bound"] - 0.25)
        for b in (0, B - 1):                                            # a row alone, B = 1
            one = ctx.keep_out_true_min_jac(Y[b:b + 1], eps_rel=EPS)
            for k in KEYS + ("jac",):
                assert np.array_equal(_bits(one[k][0]), _bits(g[k][b])), (k, b)
        for o in range(len(obs)):                                       # the free-curve call on the same curves
            sel = np.flatnonzero(VO[:, 1] == o)
            curves = np.array([[_curve(Y, b, VO[p, 0], dim) for p in sel] for b in range(B)]).reshape(B * sel.size, dim, deg + 1)
            f = ctx.bern_keep_out(curves, H[off[o]:off[o + 1]], eps_rel=EPS)
            assert np.array_equal(_bits(f["val"]), _bits(g["val"][:, sel].ravel()))
            assert np.array_equal(_bits(f["t_star"]), _bits(g["t_star"][:, sel].ravel()))
            assert np.array_equal(f["status"], g["status"][:, sel].ravel())
        dev = torch.device("cuda", 0)                                   # _dev = host, nullable outputs omitted
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            dY = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
            i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
            d = dict(val=f64(B, P), t_star=f64(B, P), face=i32(B, P, 2), lam=f64(B, P), bound=f64(B, P), nodes=i32(B, P),
                     status=i32(B, P), jac=f64(B, P, dim, deg + 1))
            ctx.keep_out_true_min_jac_dev(dY.data_ptr(), B, d["val"].data_ptr(), d["jac"].data_ptr(), d["t_star"].data_ptr(),
                                          d["face"].data_ptr(), d["lam"].data_ptr(), d["bound"].data_ptr(), d["nodes"].data_ptr(),
                                          d["status"].data_ptr(), eps_rel=EPS)
            dv2, dt2 = f64(B, P), f64(B, P)
            ctx.keep_out_true_min_dev(dY.data_ptr(), B, dv2.data_ptr(), dt2.data_ptr(), eps_rel=EPS)
            o = 0
            sel = np.flatnonzero(VO[:, 1] == o)
            dc = torch.from_numpy(np.ascontiguousarray(np.array([_curve(Y, 0, VO[p, 0], dim) for p in sel]))).to(dev)
            dfv, dft = f64(sel.size), f64(sel.size)
            ctx.bern_keep_out_dev(dc.data_ptr(), sel.size, dim, deg + 1, H[off[o]:off[o + 1]], dfv.data_ptr(), dft.data_ptr(), eps_rel=EPS)
            torch.cuda.synchronize()
        finally:
            ctx.use_own_stream()
        _same({k: x.cpu().numpy() for k, x in d.items()}, g, KEYS + ("jac",), "_dev against host")
        assert np.array_equal(_bits(dv2.cpu().numpy()), _bits(g["val"])) and np.array_equal(_bits(dt2.cpu().numpy()), _bits(g["t_star"]))
        assert np.array_equal(_bits(dfv.cpu().numpy()), _bits(g["val"][0, sel])) and np.array_equal(_bits(dft.cpu().numpy()), _bits(g["t_star"][0, sel]))
    finally:
        ctx.close()

    kinds, skipped, worst_blk, worst_val, two_faced = set(), 0, 0.0, 0.0, 0
    for b in range(B):
        for p, (vv, o) in enumerate(VO.tolist()):
            Pc, Ho, f0 = _curve(Y, b, vv, dim), H[off[o]:off[o + 1]], int(off[o])
            r = rep[b][p]["row"]
            val, t, bound = g["val"][b, p], g["t_star"][b, p], g["bound"][b, p]
            tol = EPS * r["s"]
            assert 0.0 <= t <= 1.0 and g["nodes"][b, p] >= 1 and g["nodes"][b, p] % 2 == 1
            # value
            exact, _ = K.G_at(Pc, Ho, t)
            allow = K.value_allowance(Pc, Ho, t)
            worst_val = max(worst_val, abs(float(exact - K.fr(val))) / allow)
            assert abs(exact - K.fr(val)) <= K.fr(allow), (b, p)
            round_ = K.value_allowance(Pc, Ho, 2.0 ** -52)              # (the deepest dyadic: what any bound may carry)
            ref = K.search(Pc, Ho, EPS)
            assert bound <= ref["val"] + round_ and ref["bound"] - round_ <= val, (b, p)
            assert bound <= val and val - bound <= tol, (b, p)
            assert abs(val - ref["val"]) <= 2.0 * tol + round_, (b, p)
            # blocks
            f1, f2, lam, blk = int(g["face"][b, p, 0]) - f0, int(g["face"][b, p, 1]), g["lam"][b, p], g["jac"][b, p]
            f2 = f2 - f0 if f2 >= 0 else -1
            assert 0 <= f1 < Ho.shape[0] and -1 <= f2 < Ho.shape[0] and f2 != f1 and 0.0 <= lam <= 1.0
            want = K.block_float(Ho, deg, t, f1, f2, lam)
            worst_blk = max(worst_blk, float(np.abs(blk - want).max()))
            assert np.abs(blk - want).max() <= 1e-9, (b, p)
            if t in (0.0, 1.0):
                kinds.add("end")
                col = 0 if t == 0.0 else deg
                assert f2 == -1 and lam == 1.0
                assert (np.delete(blk, col, axis=1) == 0.0).all() and np.array_equal(blk[:, col], Ho[f1, :dim]), (b, p)
                continue
            if not rep[b][p]["generic"]:
                skipped += 1
                continue
            e1, e2, elam = K.active(Pc, Ho, t, tol)
            assert {f1, f2} == {e1, e2}, (b, p, "the faces of the exact rule at the device's t_star")
            assert abs(lam - float(K.lam_at(Pc, Ho, t, f1, f2))) <= 1e-9, (b, p)
            if f2 >= 0:
                kinds.add("kink")
                two_faced += all(np.abs(blk - K.block_float(Ho, deg, t, f, -1, 1)).max() > 1e-3 for f in (f1, f2))
            else:
                kinds.add("smooth")
            if val < 0.0:
                kinds.add("penetrating")
            if val > 10.0:
                kinds.add("far")
    if (g["val"] > 10.0).any():
        kinds.add("far")
    if (g["val"] < 0.0).any():
        kinds.add("penetrating")
    print("deg %d dim %d: largest |block - exact| %.3e, largest share of K 2^-53 M %.3f, nodes mean %.1f max %d, skipped %d, "
          "two-faced kinks %d" % (deg, dim, worst_blk, worst_val, g["nodes"].mean(), g["nodes"].max(), skipped, two_faced))
    assert skipped <= (B * P) // 10
    assert two_faced >= 1, "the batch holds a kink whose block is neither face's own: a one-face implementation fails here"
    assert {"end", "kink", "penetrating", "far"} <= kinds and (deg == 1 or "smooth" in kinds), kinds


# ------------------------------------------------------------------------------------------------ 2. edge cases
def test_edge_cases():
    """NaN or inf in a control point or a face: NaN outputs, status OK, the other items untouched.  max_nodes = 3: NODE_CAP
    with a valid bracket.  17 faces: OBTG_ERR_UNSUPPORTED.  No tables, bad tables, null pointers, dY = NULL: OBTG_ERR_ARG."""
    from optimalbeziertrajectorygeneration_amd import _capi
    deg, dim = 5, 2
    Y, obs, H, off, VO, rep = T.shared(deg, dim)
    P = VO.shape[0]
    c = _capi.Context(N, dim, deg, 0, device=0)
    try:
        with pytest.raises(_capi.ObtgError) as err:                   # no tables set
            c.keep_out_true_min(Y)
        assert err.value.code == ERR_ARG
        good = c.keep_out_true_min_jac(Y[:1], (H, off, VO), eps_rel=EPS)
        Yn = Y[:1].copy()
        Yn[0, 1 * dim + 1, 2] = np.nan                                # vehicle 1
        Yn[0, 2 * dim, 0] = np.inf                                    # vehicle 2
        g = c.keep_out_true_min_jac(Yn, eps_rel=EPS)
        bad = VO[:, 0] >= 1
        assert (g["status"] == _capi.MD_OK).all()
        for k in ("val", "t_star", "lam", "bound"):
            assert np.isnan(g[k][0, bad]).all() and np.array_equal(_bits(g[k][0, ~bad]), _bits(good[k][0, ~bad])), k
        assert np.isnan(g["jac"][0, bad]).all() and np.array_equal(_bits(g["jac"][0, ~bad]), _bits(good["jac"][0, ~bad]))
        assert (g["face"][0, bad] == -1).all() and (g["nodes"][0, bad] == 0).all()
        Hb = H.copy()
        Hb[1, 0] = np.nan                                             # a face of obstacle 0
        Hb[int(off[1]), dim] = np.inf                                 # a face of obstacle 1: every item is bad
        g = c.keep_out_true_min_jac(Y[:1], (Hb, off, VO), eps_rel=EPS)
        assert np.isnan(g["val"]).all() and np.isnan(g["jac"]).all() and (g["status"] == _capi.MD_OK).all()
        # the node budget
        c.set_keep_out(H, off, VO)
        full = c.keep_out_true_min(Y, eps_rel=EPS)
        cap = c.keep_out_true_min(Y, eps_rel=EPS, max_nodes=3)
        capped = cap["status"] == _capi.MD_NODE_CAP
        assert capped.any() and (cap["status"][~capped] == _capi.MD_OK).all()
        assert (cap["nodes"][capped] == 3).all() and (full["nodes"][capped] > 3).all() and (full["nodes"][~capped] <= 3).all()
        assert (cap["bound"] <= full["val"]).all() and (full["val"] <= cap["val"]).all() and (cap["bound"] <= cap["val"]).all()
        _same({k: x[~capped] for k, x in cap.items()}, {k: x[~capped] for k, x in full.items()}, KEYS, "items that end in time")
        # argument errors
        for offx, VOx in ((off, [[N, 0]]), (off, [[-1, 0]]), (off, [[0, 2]]), (off, [[0, -1]]), ([0, 4, 4], [[0, 0]]), ([0, 5, 4], [[0, 0]]),
                          ([1, 4, 7], [[0, 0]])):
            with pytest.raises(_capi.ObtgError) as err:
                c.set_keep_out(H, offx, VOx)
            assert err.value.code == ERR_ARG, (offx, VOx)
        with pytest.raises(_capi.ObtgError) as err:
            c.set_keep_out(np.ones((17, 3)), [0, 17], [[0, 0]])
        assert err.value.code == _capi.ERR_UNSUPPORTED
        with pytest.raises(_capi.ObtgError) as err:
            c.bern_keep_out(Y[0, :dim], np.ones((17, 3)))
        assert err.value.code == _capi.ERR_UNSUPPORTED
        _same(c.keep_out_true_min(Y, eps_rel=EPS), full, KEYS, "refused tables change nothing")
        lib, h = c._lib, c._h
        out = np.zeros((1, P))
        Y1 = np.ascontiguousarray(Y[:1])
        nul = (None,) * 6
        assert lib.obtg_keep_out_true_min(h, _capi._ptr(Y1), 1, 0.0, 1e-9, 100, None, *nul) == ERR_ARG                 # null out
        assert lib.obtg_keep_out_true_min(h, None, 1, 0.0, 1e-9, 100, _capi._ptr(out), *nul) == ERR_ARG               # null Y
        assert lib.obtg_keep_out_true_min(h, _capi._ptr(Y1), 1, 0.0, 1e-9, 0, _capi._ptr(out), *nul) == ERR_ARG       # max_nodes
        assert lib.obtg_keep_out_true_min(h, _capi._ptr(Y1), 1, 0.0, -1.0, 100, _capi._ptr(out), *nul) == ERR_ARG     # eps_rel
        assert lib.obtg_keep_out_true_min_jac(h, _capi._ptr(Y1), 1, 0.0, 1e-9, 100, _capi._ptr(out), *nul, None) == ERR_ARG   # null jac
        assert lib.obtg_keep_out_true_min_dev(h, None, 1, 0.0, 1e-9, 100, _capi._ptr(out), *nul) == ERR_ARG           # no view form
        c.set_keep_out(H, off, np.zeros((0, 2), np.int32))            # P = 0 clears
        assert c.len_keep_out == 0
        with pytest.raises(_capi.ObtgError) as err:
            c.keep_out_true_min(Y)
        assert err.value.code == ERR_ARG
    finally:
        c.close()
    line = _capi.Context(1, 1, 3, 0, device=0)
    try:
        with pytest.raises(_capi.ObtgError) as err:
            line.set_keep_out(np.array([[1.0, 2.0]]), [0, 1], [[0, 0]])
        assert err.value.code == ERR_ARG
    finally:
        line.close()
    big = _capi.Context(1, 2, 32, 0, device=0)
    try:
        big.set_keep_out(np.array([[1.0, 0.0, 2.0]]), [0, 1], [[0, 0]])
        with pytest.raises(_capi.ObtgError) as err:
            big.keep_out_true_min(np.zeros((1, 2, 33)))
        assert err.value.code == _capi.ERR_UNSUPPORTED
    finally:
        big.close()


def test_python_refusals():
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    from optimalbeziertrajectorygeneration_amd import bezier
    sq = K.unit_square()
    kw = dict(numVeh=1, degree=3, minimizeGoal='Euclidean', maxSep=1, tf=1.0)
    with pytest.raises(ValueError, match="dimension 2 or 3"):
        BezOptimization(dimension=4, initPoints=[(0, 0, 0, 0)], finalPoints=[(1, 1, 1, 1)], keepOut=[(np.ones((1, 4)), np.ones(1))], **kw)
    for bad in (sq, [(sq[0],)], [(sq[0], np.ones(3))], []):
        with pytest.raises(ValueError):
            BezOptimization(dimension=2, initPoints=[(3, 3)], finalPoints=[(4, 4)], keepOut=bad, **kw)
    bo = BezOptimization(dimension=2, initPoints=[(3, 3)], finalPoints=[(4, 4)], keepOut=[sq], **kw)
    x = bo.generateGuess(std=0)
    with pytest.raises(ValueError, match="not built for the keep-out rows"):
        bo.keepOutJacobian(x, method='exact')
    none = BezOptimization(dimension=2, initPoints=[(3, 3)], finalPoints=[(4, 4)], **kw)
    for call in (none.keepOutConstraints, none.keepOutJacobian, none.trueKeepOutClearances):
        with pytest.raises(ValueError, match="keepOut is None"):
            call(x)
    with pytest.raises(ValueError):
        bezier.Bezier(np.zeros((4, 3))).keepOutClearance(np.ones((1, 4)), np.ones(1))
    with pytest.raises(ValueError):
        bezier.Bezier(np.zeros((2, 3))).keepOutClearance(np.ones((2, 3)), np.ones(2))


# ------------------------------------------------------------------------------------------------ 3. BezOptimization
def _dubins(**kw):
    """time-optimal, speeds prescribed: tf moves columns 1 and -2 of every vehicle"""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, minSpeed=0.2, maxAngRate=1,
                           initPoints=[(-3, 2), (3, -3)], finalPoints=[(5, 1), (3.5, 4)], initSpeeds=[1, 1], finalSpeeds=[1, 1],
                           initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], keepOut=K.obstacles(2), **kw)


def _space(**kw):
    """3-D, fixed tf, degree 6"""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=3, dimension=3, degree=6, minimizeGoal='Euclidean', maxSep=0.9, maxSpeed=3, minSpeed=0.1, tf=6.0,
                           initPoints=[(-3, -2, -1), (5, -2, 1), (0, -3, 2)], finalPoints=[(5, 3, 1), (-2, 3, 0.5), (3.5, 4, -1)],
                           keepOut=K.obstacles(3), **kw)


# (constructor, noise and seed of the guess, tf of the guess): the yardstick alone says that every row of these guesses is
# generic and that both hold kinks, a smooth interior minimum and a penetrating row (chosen on the CPU)
PROBLEMS = {"dubins": (_dubins, 1.5, 1, 6.0), "space": (_space, 1.5, 13, None)}


def _x0(name, **kw):
    make, std, seed, tf = PROBLEMS[name]
    bo = make(**kw)
    x = bo.generateGuess(std=std, seed=seed)
    if bo._timeopt():
        x[-1] = tf
    return bo, x


def _scatter(bo, blk, VO, D):
    """Dense [P][n_x] from blocks [P][dim][n + 1]: the free columns in the owner's columns; D (time-optimal): dY/dtf"""
    Nv, dim = bo.model['numVeh'], bo.model['dim']
    first, cols = bo._rv_parts()[1], bo._numCols
    J = np.zeros((VO.shape[0], Nv * dim * cols))
    for p, (v, _) in enumerate(VO.tolist()):
        J[p, v * dim * cols:(v + 1) * dim * cols] = blk[p][:, first:first + cols].reshape(-1)
    if D is None:
        return J
    D = np.asarray(D, dtype=np.float64).reshape(Nv, dim, -1)
    col = np.array([float((blk[p] * D[v]).sum()) for p, (v, _) in enumerate(VO.tolist())])
    return np.hstack((J, col[:, None]))


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_closure_providers_and_envelope_against_fd(name):
    """The closure is the raw call, served from one batch under SciPy's differences; keepOutMargin shifts it; the envelope
    provider is the device's blocks scattered to the owner's columns, the tf column dY/dtf alone.  'envelope' against 'fd'
    (h = FD_STEP), row by row on the generic rows: the device's gap may be twice the yardstick's own gap between its envelope
    block and its forward difference with the same h on the same input, plus 1e-9 (t_star moving within tol is the only other
    source).  Measured on the MI355X: dubins 6.509e-05 (the yardstick's own 6.510e-05), space 2.040e-04 (2.040e-04) --
    the search slack eps_rel s / h of the difference quotient, common to both."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    from optimalbeziertrajectorygeneration_amd import bezier
    bo, x = _x0(name)
    Nv, dim, deg = bo.model['numVeh'], bo.model['dim'], bo.model['deg']
    H, off, VO = opt._keep_out_tables(bo.keepOut, Nv, dim)
    P = VO.shape[0]
    assert P == Nv * 2
    ctx = bo._ctx(False)
    Y = bo.reshapeVector(x)
    raw = ctx.keep_out_true_min_jac(Y[None], (H, off, VO), eps_rel=bo.TRUE_MIN_EPS_REL)
    rows = bo.keepOutConstraints(x)
    assert rows.shape == (P,) and np.array_equal(_bits(rows), _bits(raw["val"][0]))
    shifted = _x0(name, keepOutMargin=0.125)[0]
    assert np.array_equal(shifted.keepOutConstraints(x), rows - 0.125)
    assert shifted._serve_key(True) != bo._serve_key(True) and bo._serve_key(True)[-1][0] == 'keepOut'
    plain = _x0(name, fdBatching=False)[0]
    before = dict(bo.fdBatchingStats)
    bo.keepOutConstraints(x)
    for k in range(x.size):
        xk = x.copy()
        xk[k] += opt.FD_STEP
        assert np.array_equal(_bits(bo.keepOutConstraints(xk)), _bits(plain.keepOutConstraints(xk))), k
    assert bo.fdBatchingStats['served'] - before['served'] == x.size and bo.fdBatchingStats['batches'] - before['batches'] == 1
    acc = bo.trueKeepOutClearances(x)
    for k, kk in (("val", "val"), ("t_star", "t_star"), ("face", "face"), ("lam", "lam"), ("status", "status")):
        assert np.array_equal(_bits(acc[k]), _bits(raw[kk][0])), k
    cl, tc = bezier.Bezier(Y[:dim]).keepOutClearance(*bo.keepOut[1])
    assert cl == raw["val"][0, 1] and tc == raw["t_star"][0, 1]
    # the providers
    Je, Jf = bo.keepOutJacobian(x, method='envelope'), bo.keepOutJacobian(x, method='fd')
    assert Je.shape == Jf.shape == (P, x.size) and np.isfinite(Je).all()
    D = bo._dY_dtf() if bo._timeopt() else None
    want = _scatter(bo, raw["jac"][0], VO, D)
    assert np.array_equal(_bits(Je), _bits(want)) or np.abs(Je - want).max() <= 1e-15
    if D is not None:
        assert D.any() and np.abs(Je[:, -1]).max() > 0
    # the yardstick's own gap, same h, same input
    first, cols = bo._rv_parts()[1], bo._numCols
    n_pts = Nv * dim * cols
    X, dx = bo._fd_rows(x)
    Ys = bo.reshapeVectors(X)
    compared, worst, worst_ref = 0, 0.0, 0.0
    for p, (v, o) in enumerate(VO.tolist()):
        Ho = H[off[o]:off[o + 1]]
        rp = K.report(Y[v * dim:(v + 1) * dim], Ho, bo.TRUE_MIN_EPS_REL)
        if not rp["generic"]:
            continue
        compared += 1
        ref_env = _scatter(bo, [rp["row"]["jac"] if q == p else np.zeros((dim, deg + 1)) for q in range(P)], VO, D)[p]
        v0 = K.search(Y[v * dim:(v + 1) * dim], Ho, bo.TRUE_MIN_EPS_REL)["val"]
        ref_fd = np.zeros(x.size)
        for k in range(x.size):
            if k < n_pts and k // (dim * cols) != v:
                continue
            ref_fd[k] = (K.search(Ys[k + 1][v * dim:(v + 1) * dim], Ho, bo.TRUE_MIN_EPS_REL)["val"] - v0) / dx[k]
        ref_gap = float(np.abs(ref_env - ref_fd).max())
        gap = float(np.abs(Je[p] - Jf[p]).max())
        worst, worst_ref = max(worst, gap), max(worst_ref, ref_gap)
        print("%s row %d (%s): device |envelope - fd| %.3e, yardstick's %.3e" % (name, p, rp["kind"], gap, ref_gap))
        assert gap <= 2.0 * ref_gap + 1e-9, (name, p)
    print("%s: largest device gap %.3e, largest yardstick gap %.3e, %d of %d rows compared" % (name, worst, worst_ref, compared, P))
    assert compared == P, "the guesses were chosen with generic rows only"


# ------------------------------------------------------------------------------------------------ 4. one SLSQP solve
def test_solve_around_a_square():
    """example22 at degree 5: the unconstrained optimum drives through the square; both constrained solves end with every
    clearance >= -1e-9 and the same tf to 1e-6; the true distance of the result (minDist2Poly) is at least the clearance.
    Measured on the MI355X: tf 2.896326733 without the obstacle (car 0 0.370161 deep); 'fd' 4.134170344 (11 iterations, smallest
    clearance -9.7e-14); 'envelope' 4.134170344 (10 iterations, smallest clearance 2.1e-13); minDist2Poly 0.000000 for both."""
    import example22_keep_out_obstacles as ex
    _, free = ex.solve(None)
    c_free = ex.clearances(free.x)["val"]
    _, fd = ex.solve('fd', x0=free.x)
    _, env = ex.solve('envelope', x0=free.x)
    c_fd, c_env = ex.clearances(fd.x)["val"], ex.clearances(env.x)["val"]
    d_fd, d_env = ex.distances(fd.x), ex.distances(env.x)
    print("tf without the obstacle %.9f (smallest clearance %.6f); 'fd' %.9f (%d iterations, status %d, smallest clearance %.3e, "
          "minDist2Poly %.6f); 'envelope' %.9f (%d iterations, status %d, smallest clearance %.3e, minDist2Poly %.6f)"
          % (free.fun, c_free.min(), fd.fun, fd.nit, fd.status, c_fd.min(), d_fd.min(), env.fun, env.nit, env.status, c_env.min(),
             d_env.min()))
    assert free.success and c_free.min() < 0.0, "the unconstrained optimum must drive through the square"
    assert fd.success and env.success
    assert (c_fd >= -1e-9).all() and (c_env >= -1e-9).all()
    assert abs(fd.fun - env.fun) <= 1e-6
    assert (d_fd >= c_fd - 1e-9).all() and (d_env >= c_env - 1e-9).all()
