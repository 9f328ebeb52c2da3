"""Keep-out rows against obstacles that move, on the device (obtg_ctx_set_keep_out_motion, obtg_keep_out_moving_true_min[_jac],
obtg_bern_keep_out_moving, BezOptimization(keepOutMotion=..), Bezier.keepOutClearance(motion=..)) against the yardstick of
tests/moving_keep_out_ref.py and against the STATIC calls, which tests/test_gpu_keep_out.py holds to exact rationals.

Every batch is N = 3 vehicles, B = 5 rows whose tf all differ, every vehicle against keep_out_ref.obstacles(dim), both moving
(moving_keep_out_ref.motions); curve degrees 1, 3, 5, 10, 20, motion degrees 0, 1, 3 and n, r = tf[0] / T in {1, 0.5, 0.3}
(the other rows' ratios are smaller).  The curves are test_keep_out_ref's shared batches."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import keep_out_ref as K  # noqa: E402
import moving_keep_out_ref as MK  # noqa: E402
import test_keep_out_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

N, B = T.N, T.B
ERR_ARG = -1
EPS = 1e-12
KEYS = ("val", "t_star", "face", "lam", "bound", "nodes", "status")
DEGS = (1, 3, 5, 10, 20)
RATIOS = (1.0, 0.5, 0.3)
# the seed of a batch's motions is 7 deg + m, but where that leaves a batch without one of the kinds test_batches asks for (chosen
# on the CPU with the yardstick alone: dim 3, degree 20, m = 3 had no end minimiser at r = 1)
MOTION_SEED = {(3, 20, 3): 1}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _curve(Y, b, v, dim):
    return Y[b, v * dim:(v + 1) * dim]


def motion_degrees(deg):
    return sorted({m for m in (0, 1, 3, deg) if m <= deg})


def case(deg, dim, m, r):
    """(Y, H, off, VO, Qs, motion tables, tf[B]) of a batch; obstacle 1's span is a quarter longer than obstacle 0's"""
    Y = K.batch(deg, dim, T.SEEDS[(dim, deg)], N, B)
    H, off, VO = K.tables(K.obstacles(dim), N)
    Qs = MK.motions(dim, m, MOTION_SEED.get((dim, deg, m), 7 * deg + m))
    tf, span = MK.spans(r, B)
    Q, q_off = MK.motion_tables(Qs)
    return Y, H, off, VO, Qs, (Q, q_off, np.array([span, 1.25 * span])), tf


def static_on_rel(_capi, rel, H, off, VO, dim, deg, margin=0.0):
    """The STATIC _jac call on a context whose vehicles are the rows of rel[B][P], item p pairing vehicle p with its obstacle"""
    Bn, P = rel.shape[:2]
    ctx = _capi.Context(P, dim, deg, 0, device=0)
    try:
        VO2 = np.stack((np.arange(P), VO[:, 1]), axis=1).astype(np.int32)
        return ctx.keep_out_true_min_jac(np.ascontiguousarray(rel.reshape(Bn, P * dim, deg + 1)), (H, off, VO2), margin=margin,
                                         eps_rel=EPS)
    finally:
        ctx.close()


def _dev_call(ctx, torch, Y, tf, P, dim, deg):
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        Bn = Y.shape[0]
        dY, dtf = torch.from_numpy(np.ascontiguousarray(Y)).to(dev), torch.from_numpy(np.ascontiguousarray(tf)).to(dev)
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)        # noqa: E731
        d = dict(val=f64(Bn, P), t_star=f64(Bn, P), face=i32(Bn, P, 2), lam=f64(Bn, P), bound=f64(Bn, P), nodes=i32(Bn, P),
                 status=i32(Bn, P), rel=f64(Bn, P, dim, deg + 1), jac=f64(Bn, P, dim, deg + 1), jac_tf=f64(Bn, P))
        ctx.keep_out_moving_true_min_jac_dev(dY.data_ptr(), dtf.data_ptr(), Bn, d["val"].data_ptr(), d["jac"].data_ptr(),
                                             d["jac_tf"].data_ptr(), d["t_star"].data_ptr(), d["face"].data_ptr(), d["lam"].data_ptr(),
                                             d["bound"].data_ptr(), d["nodes"].data_ptr(), d["status"].data_ptr(), d["rel"].data_ptr(),
                                             eps_rel=EPS)
        dv2, dt2 = f64(Bn, P), f64(Bn, P)                               # the value call, nullable outputs omitted
        ctx.keep_out_moving_true_min_dev(dY.data_ptr(), dtf.data_ptr(), Bn, dv2.data_ptr(), dt2.data_ptr(), eps_rel=EPS)
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    out = {k: x.cpu().numpy() for k, x in d.items()}
    return out, dv2.cpu().numpy(), dt2.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1, 2, 4, 5: the batches
@pytest.mark.parametrize("dim", T.DIMS)
@pytest.mark.parametrize("deg", DEGS)
def test_batches(deg, dim):
    """Per motion degree and ratio.  (1) rel within moving_keep_out_ref.rel_allowance of the exact rationals.  (2) every
    output of the moving _jac call equals, bit for bit, the static _jac call on a context whose vehicles are the rows of rel.
    (4) jac_tf within 1e-9 |a^| max|E'| / tf of the exact formula at the device's own (t_star, faces, lam), plus what the
    device's E leaves in E' = n (E1 - E0) when that scale is 0 or nearly (a motion of degree 0: E' is an exact 0, the device's
    E constant within its allowance): 2 n (allowance + 3 (n - 1) 2^-53 max |Q|) per coordinate -- the allowance of E and the
    n - 1 levels of its evaluation at t_star, three roundings each -- times |a^|_1 t / tf.
    (5) the same bits from the value call, the _dev calls, a row alone and obtg_bern_keep_out_moving.  Every batch holds a
    kink, an end minimiser, a penetrating item and a far item; no item is left out of any check.
    Measured on the MI355X (printed per case): rel uses at most 0.188 of its allowance (degree 1, space; 0.012 at degree 20);
    jac_tf is at most 1.2e-14 of its scale from the exact formula (degree 20, planar)."""
    import torch
    from optimalbeziertrajectorygeneration_amd import _capi
    worst_share, worst_tf = 0.0, 0.0
    ctx = _capi.Context(N, dim, deg, 0, device=0)
    try:
        for m in motion_degrees(deg):
            for r in RATIOS:
                Y, H, off, VO, Qs, motion, tf = case(deg, dim, m, r)
                P = VO.shape[0]
                assert len(set(tf.tolist())) == B
                ctx.set_keep_out(H, off, VO)
                ctx.set_keep_out_motion(*motion)
                ctx.set_profiling(True)
                ctx.reset_kernel_stats()
                g = ctx.keep_out_moving_true_min_jac(Y, tf, eps_rel=EPS)
                stats = ctx.kernel_stats()
                ctx.set_profiling(False)
                assert stats["speed"][1] == 1 and sum(n for _, n in stats.values()) == 1, stats       # one kernel, one launch
                assert (g["status"] == _capi.MD_OK).all() and np.isfinite(g["jac_tf"]).all()
                # every kind is in the batch
                assert (g["face"][..., 1] >= 0).any(), "a kink"
                assert ((g["t_star"] == 0.0) | (g["t_star"] == 1.0)).any(), "an end minimiser"
                assert (g["val"] < 0.0).any() and (g["val"] > 10.0).any(), "a penetrating item and a far item"
                # (2) one body
                s = static_on_rel(_capi, g["rel"], H, off, VO, dim, deg)
                _same(g, s, KEYS + ("jac",), ("the static call on rel", m, r))
                # (5) call forms
                v = ctx.keep_out_moving_true_min(Y, tf, (H, off, VO), motion, eps_rel=EPS)
                _same(v, g, KEYS + ("rel",), "the value call")
                d, dv2, dt2 = _dev_call(ctx, torch, Y, tf, P, dim, deg)
                _same(d, g, KEYS + ("rel", "jac", "jac_tf"), "_dev against host")
                assert np.array_equal(_bits(dv2), _bits(g["val"])) and np.array_equal(_bits(dt2), _bits(g["t_star"]))
                for b in (0, B - 1):
                    one = ctx.keep_out_moving_true_min_jac(Y[b:b + 1], tf[b:b + 1], eps_rel=EPS)
                    for k in KEYS + ("rel", "jac", "jac_tf"):
                        assert np.array_equal(_bits(one[k][0]), _bits(g[k][b])), (k, b)
                for o in range(2):
                    sel = np.flatnonzero(VO[:, 1] == o)
                    curves = np.array([[_curve(Y, b, VO[p, 0], dim) for p in sel] for b in range(B)]).reshape(B * sel.size, dim, deg + 1)
                    f = ctx.bern_keep_out_moving(curves, H[off[o]:off[o + 1]], Qs[o], np.repeat(tf / motion[2][o], sel.size), eps_rel=EPS)
                    assert np.array_equal(_bits(f["val"]), _bits(g["val"][:, sel].ravel()))
                    assert np.array_equal(_bits(f["t_star"]), _bits(g["t_star"][:, sel].ravel()))
                    assert np.array_equal(f["status"], g["status"][:, sel].ravel())
                # (1) and (4) against exact rationals
                for b in range(B):
                    for o in range(2):
                        rr = MK.ratio(tf[b], motion[2][o])
                        E = MK.motion_points(Qs[o], rr, deg)
                        Ho, f0 = H[off[o]:off[o + 1]], int(off[o])
                        for p in np.flatnonzero(VO[:, 1] == o):
                            Pc = _curve(Y, b, VO[p, 0], dim)
                            allow = MK.rel_allowance(Pc, Qs[o])
                            for c in range(dim):
                                err = max(abs(Fraction(g["rel"][b, p, c, i]) - (Fraction(Pc[c, i]) - E[c][i])) for i in range(deg + 1))
                                worst_share = max(worst_share, float(err / Fraction(allow[c])))
                                assert err <= Fraction(allow[c]), ("rel", m, r, b, p, c)
                            t, lam = g["t_star"][b, p], g["lam"][b, p]
                            f1, f2 = int(g["face"][b, p, 0]) - f0, int(g["face"][b, p, 1])
                            f2 = f2 - f0 if f2 >= 0 else -1
                            want = MK.jac_tf(E, Ho, t, f1, f2, lam, tf[b])
                            scale = MK.jac_tf_scale(E, Ho, f1, f2, lam, tf[b])
                            a1 = float(sum(abs(x) for x in MK.a_hat(Ho, f1, f2, lam)))
                            floor = a1 * 2.0 * deg * (float(allow.max()) + 3.0 * (deg - 1) * 2.0 ** -53 * np.abs(Qs[o]).max()) * t / tf[b]
                            err = abs(float(Fraction(g["jac_tf"][b, p]) - want))
                            if scale > 0.0:
                                worst_tf = max(worst_tf, err / scale)
                            assert err <= 1e-9 * scale + floor, ("jac_tf", m, r, b, p, err, scale)
    finally:
        ctx.close()
    print("degree %d, dim %d: rel uses at most %.3f of its allowance; jac_tf at most %.3e of its scale" % (deg, dim, worst_share, worst_tf))


# ------------------------------------------------------------------------------------------------ 3. identities
@pytest.mark.parametrize("dim", T.DIMS)
def test_identities(dim):
    """An all-zero motion: the static call's bits on Y, jac_tf == 0.  m = n at r = 1: the static call's bits on the host's
    P - Q.  One obstacle static and one moving in the same tables: the static one's items are the static call's, tf and all,
    with jac_tf an exact 0, the moving one's items those of the call in which both move."""
    from optimalbeziertrajectorygeneration_amd import _capi
    deg = 5
    Y, H, off, VO, Qs, motion, tf = case(deg, dim, deg, 1.0)
    P = VO.shape[0]
    ctx = _capi.Context(N, dim, deg, 0, device=0)
    try:
        ctx.set_keep_out(H, off, VO)
        st = ctx.keep_out_true_min_jac(Y, eps_rel=EPS)
        zero = MK.motion_tables([np.zeros((dim, 4)), np.zeros((dim, 1))])
        z = ctx.keep_out_moving_true_min_jac(Y, tf, None, (*zero, motion[2]), eps_rel=EPS)
        _same(z, st, KEYS + ("jac",), "an all-zero motion")
        assert np.array_equal(_bits(z["rel"]), _bits(np.array([[_curve(Y, b, v, dim) for v, _ in VO.tolist()] for b in range(B)])))
        assert (z["jac_tf"] == 0.0).all()
        # m = n, r = 1: every row alone, its tf the motion's span
        for b in range(B):
            span = np.array([tf[b], tf[b]])
            one = ctx.keep_out_moving_true_min_jac(Y[b:b + 1], tf[b:b + 1], None, (motion[0], motion[1], span), eps_rel=EPS)
            host = np.array([[_curve(Y, b, v, dim) - Qs[o] for v, o in VO.tolist()]])
            assert np.array_equal(_bits(one["rel"]), _bits(host)), b
            _same(one, static_on_rel(_capi, host, H, off, VO, dim, deg), KEYS + ("jac",), ("m = n, r = 1", b))
        # mixed tables
        both = ctx.keep_out_moving_true_min_jac(Y, tf, None, motion, eps_rel=EPS)
        mixed = ctx.keep_out_moving_true_min_jac(Y, tf, None, (*MK.motion_tables([None, Qs[1]]), motion[2]), eps_rel=EPS)
        still, moves = VO[:, 1] == 0, VO[:, 1] == 1
        for k in KEYS + ("jac",):
            assert np.array_equal(_bits(mixed[k][:, still]), _bits(st[k][:, still])), k
        for k in KEYS + ("jac", "jac_tf", "rel"):
            assert np.array_equal(_bits(mixed[k][:, moves]), _bits(both[k][:, moves])), k
        assert (_bits(mixed["jac_tf"][:, still]) == 0).all(), "an exact +0"
        assert np.abs(both["jac_tf"][:, still]).max() > 0.0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. edge cases
@pytest.mark.parametrize("dim", T.DIMS)
def test_edge_cases(dim):
    """NaN in Q or tf, tf <= 0: NaN outputs of that item (rel, jac, jac_tf too; face -1, nodes 0), status OK, the others
    untouched.  r > 1 answers finite rows (the continuation; no bound claimed).  The error codes of
    obtg_ctx_set_keep_out_motion; a call without a motion; obtg_ctx_set_keep_out clears the motion."""
    from optimalbeziertrajectorygeneration_amd import _capi
    deg = 5
    Y, H, off, VO, Qs, motion, tf = case(deg, dim, 3, 0.5)
    P = VO.shape[0]
    c = _capi.Context(N, dim, deg, 0, device=0)
    try:
        c.set_keep_out(H, off, VO)
        full = c.keep_out_moving_true_min_jac(Y, tf, None, motion, eps_rel=EPS)
        allkeys = KEYS + ("rel", "jac", "jac_tf")

        def nan_items(r, bad):
            for k in ("val", "t_star", "lam", "bound", "jac_tf"):
                assert np.isnan(r[k][bad]).all() and np.isfinite(r[k][~bad]).all(), k
            assert np.isnan(r["rel"][bad]).all() and np.isnan(r["jac"][bad]).all()
            assert (r["face"][bad] == -1).all() and (r["nodes"][bad] == 0).all() and (r["status"] == _capi.MD_OK).all()
            _same({k: r[k][~bad] for k in allkeys}, {k: full[k][~bad] for k in allkeys}, allkeys, "the other items")

        for badval in (np.nan, np.inf):
            Qn = [Qs[0].copy(), Qs[1].copy()]
            Qn[1][dim - 1, 1] = badval
            r = c.keep_out_moving_true_min_jac(Y, tf, None, (*MK.motion_tables(Qn), motion[2]), eps_rel=EPS)
            nan_items(r, np.broadcast_to(VO[:, 1] == 1, (B, P)))
        for badtf in (np.nan, np.inf, 0.0, -1.0):
            tfn = tf.copy()
            tfn[2] = badtf
            bad = np.zeros((B, P), bool)
            bad[2] = True
            nan_items(c.keep_out_moving_true_min_jac(Y, tfn, None, motion, eps_rel=EPS), bad)
        # r > 1: tf beyond both spans
        over = c.keep_out_moving_true_min_jac(Y, 1.5 * motion[2].max() * np.ones(B), None, motion, eps_rel=EPS)
        assert all(np.isfinite(over[k]).all() for k in ("val", "t_star", "lam", "bound", "rel", "jac", "jac_tf"))
        assert (over["status"] == _capi.MD_OK).all()
        # the error codes
        Q, q_off, span = motion
        for qo, sp, O in (([0, 4], span[:1], 1), ([1, 5, 9], span, 2), ([0, 4, 3], span, 2), (q_off, [1.0, 0.0], 2), (q_off, [1.0, -2.0], 2),
                          (q_off, [np.inf, 1.0], 2), (q_off, [1.0, np.nan], 2)):
            with pytest.raises(_capi.ObtgError) as err:
                c.set_keep_out_motion(Q, qo, sp)
            assert err.value.code == ERR_ARG, (qo, sp)
        with pytest.raises(_capi.ObtgError) as err:
            c.set_keep_out_motion(np.zeros(dim * (deg + 2)), [0, deg + 2, deg + 2], span)          # m > n
        assert err.value.code == _capi.ERR_UNSUPPORTED
        with pytest.raises(_capi.ObtgError) as err:
            c.bern_keep_out_moving(Y[0, :dim], H[:off[1]], np.zeros((dim, deg + 2)))
        assert err.value.code == _capi.ERR_UNSUPPORTED
        c.set_keep_out_motion(*motion)
        _same(c.keep_out_moving_true_min_jac(Y, tf, eps_rel=EPS), full, allkeys, "refused motions change nothing")
        lib, h = c._lib, c._h
        out, Y1, tf1 = np.zeros((1, P)), np.ascontiguousarray(Y[:1]), np.ascontiguousarray(tf[:1])
        nul = (None,) * 7
        ptr = _capi._ptr
        assert lib.obtg_keep_out_moving_true_min(h, ptr(Y1), ptr(tf1), 1, 0.0, 1e-9, 100, None, *nul) == ERR_ARG             # null out
        assert lib.obtg_keep_out_moving_true_min(h, None, ptr(tf1), 1, 0.0, 1e-9, 100, ptr(out), *nul) == ERR_ARG           # null Y
        assert lib.obtg_keep_out_moving_true_min(h, ptr(Y1), None, 1, 0.0, 1e-9, 100, ptr(out), *nul) == ERR_ARG            # null tf
        assert lib.obtg_keep_out_moving_true_min_jac(h, ptr(Y1), ptr(tf1), 1, 0.0, 1e-9, 100, ptr(out), *nul, None, None) == ERR_ARG
        assert lib.obtg_keep_out_moving_true_min_dev(h, None, ptr(tf1), 1, 0.0, 1e-9, 100, ptr(out), *nul) == ERR_ARG       # no view form
        # obtg_ctx_set_keep_out clears the motion; so does O = 0
        c.set_keep_out(H, off, VO)
        with pytest.raises(_capi.ObtgError) as err:
            c.keep_out_moving_true_min(Y, tf)
        assert err.value.code == ERR_ARG
        c.set_keep_out_motion(*motion)
        c.set_keep_out_motion(np.zeros(0), np.zeros(1, np.int32), np.zeros(0))
        with pytest.raises(_capi.ObtgError) as err:
            c.keep_out_moving_true_min(Y, tf)
        assert err.value.code == ERR_ARG
        _same(c.keep_out_true_min_jac(Y, eps_rel=EPS), static_on_rel(_capi, np.array(
            [[_curve(Y, b, v, dim) for v, _ in VO.tolist()] for b in range(B)]), H, off, VO, dim, deg), KEYS + ("jac",), "static again")
        c.set_keep_out(H, off, np.zeros((0, 2), np.int32))
        with pytest.raises(_capi.ObtgError) as err:
            c.set_keep_out_motion(*motion)                                # no keep-out tables set
        assert err.value.code == ERR_ARG
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 7. BezOptimization
def provider_motion(dim):
    """obstacle 0 along a straight line, obstacle 1 along a cubic, both on [0, 8]"""
    Qs = MK.motions(dim, 3, 11)
    return [(np.ascontiguousarray(Qs[0][:, :2]), 8.0), (Qs[1], 8.0)]


def _dubins(**kw):
    """planar, degree 5, time-optimal, speeds prescribed: tf moves columns 1 and -2 of every vehicle AND the obstacles"""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, minSpeed=0.2, maxAngRate=1,
                           initPoints=[(-3, 2), (3, -3)], finalPoints=[(5, 1), (3.5, 4)], initSpeeds=[1, 1], finalSpeeds=[1, 1],
                           initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], keepOut=K.obstacles(2), keepOutMotion=provider_motion(2), **kw)


def _space(**kw):
    """3-D, degree 6, time-optimal: tf moves the obstacles alone"""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    return BezOptimization(numVeh=3, dimension=3, degree=6, minimizeGoal='TimeOpt', maxSep=0.9, maxSpeed=3, minSpeed=0.1,
                           initPoints=[(-3, -2, -1), (5, -2, 1), (0, -3, 2)], finalPoints=[(5, 3, 1), (-2, 3, 0.5), (3.5, 4, -1)],
                           keepOut=K.obstacles(3), keepOutMotion=provider_motion(3), **kw)


# (constructor, noise and seed of the guess, tf of the guess): the yardstick alone says that every row of these guesses is
# generic (chosen on the CPU)
PROBLEMS = {"dubins": (_dubins, 1.5, 1, 6.0), "space": (_space, 1.5, 13, 6.0)}


def provider_x0(name, **kw):
    make, std, seed, tf = PROBLEMS[name]
    bo = make(**kw)
    x = bo.generateGuess(std=std, seed=seed)
    x[-1] = tf
    return bo, x


def yardstick_gaps(bo, x):
    """per row (generic, kind, envelope row [n_x], forward-difference row [n_x]) of the yardstick alone on bo's input: the
    envelope row is the exact block at the search's own minimiser scattered to the owner's columns, its tf column the block
    along dY/dtf plus the exact d row / d tf; the differences are those of the searched row of the rounded relative points"""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    Nv, dim, deg = bo.model['numVeh'], bo.model['dim'], bo.model['deg']
    H, off, VO = opt._keep_out_tables(bo.keepOut, Nv, dim)
    first, cols = bo._rv_parts()[1], bo._numCols
    n_pts = Nv * dim * cols
    D = bo._dY_dtf().reshape(Nv, dim, -1)
    X, dx = bo._fd_rows(x)
    Ys = bo.reshapeVectors(X)
    out = []
    for p, (v, o) in enumerate(VO.tolist()):
        Ho, (Qo, To) = H[off[o]:off[o + 1]], bo.keepOutMotion[o]
        r = MK.row(Ys[0][v * dim:(v + 1) * dim], Qo, To, x[-1], Ho, bo.TRUE_MIN_EPS_REL)
        rp = K.report(r["D"], Ho, bo.TRUE_MIN_EPS_REL)
        blk = K.block_float(Ho, deg, r["t"], r["f1"], r["f2"], r["lam"])
        env = np.zeros(x.size)
        env[v * dim * cols:(v + 1) * dim * cols] = blk[:, first:first + cols].reshape(-1)
        env[-1] = float((blk * D[v]).sum()) + r["jac_tf"]
        fd = np.zeros(x.size)
        for k in range(x.size):
            if k < n_pts and k // (dim * cols) != v:
                continue
            fd[k] = (MK.searched_row(Ys[k + 1][v * dim:(v + 1) * dim], Qo, To, X[k + 1, -1], Ho, bo.TRUE_MIN_EPS_REL)["val"] - r["val"]) / dx[k]
        out.append((rp["generic"], rp["kind"], env, fd))
    return out


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_providers_envelope_against_fd_with_the_tf_column(name):
    """The closure is the raw moving call; the envelope provider is the device's blocks scattered to the owner's columns,
    its tf column the block along dY/dtf plus jac_tf.  'envelope' against 'fd' (h = FD_STEP) row by row, the tf column
    included: the device's gap may be twice the yardstick's own gap on the same input plus 1e-9, as
    test_gpu_keep_out.py::test_closure_providers_and_envelope_against_fd allows.  The key of a kept FD batch ends with the
    motion's entry, and only while a motion is set.  Measured on the MI355X: dubins 1.683e-04 (the yardstick's own 1.683e-04;
    tf column 4.235e-05 against 4.234e-05), space 3.612e-04 (3.612e-04; tf column 3.142e-04 both)."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    bo, x = provider_x0(name)
    Nv, dim = bo.model['numVeh'], bo.model['dim']
    H, off, VO = opt._keep_out_tables(bo.keepOut, Nv, dim)
    P = VO.shape[0]
    motion = bo._keep_out_motion()
    Y = bo.reshapeVector(x)
    raw = bo._ctx(False).keep_out_moving_true_min_jac(Y[None], x[-1:], (H, off, VO), motion, eps_rel=bo.TRUE_MIN_EPS_REL)
    rows = bo.keepOutConstraints(x)
    assert rows.shape == (P,) and np.array_equal(_bits(rows), _bits(raw["val"][0]))
    acc = bo.trueKeepOutClearances(x)
    for k in ("val", "t_star", "face", "lam", "status"):
        assert np.array_equal(_bits(acc[k]), _bits(raw[k][0])), k
    key = bo._serve_key(True)
    assert key[-1][0] == 'keepOutMotion' and key[-2][0] == 'keepOut'
    bo.keepOutMotion = None
    still = bo._serve_key(True)
    assert still == key[:-1] and still[-1][0] == 'keepOut'
    assert not np.array_equal(bo.keepOutConstraints(x), rows), "without the motion: the static rows"
    bo.keepOutMotion = provider_motion(dim)
    plain = provider_x0(name, fdBatching=False)[0]
    before = dict(bo.fdBatchingStats)
    bo.keepOutConstraints(x)
    for k in range(x.size):
        xk = x.copy()
        xk[k] += opt.FD_STEP
        assert np.array_equal(_bits(bo.keepOutConstraints(xk)), _bits(plain.keepOutConstraints(xk))), k
    assert bo.fdBatchingStats['served'] - before['served'] == x.size and bo.fdBatchingStats['batches'] - before['batches'] == 1
    Je, Jf = bo.keepOutJacobian(x, method='envelope'), bo.keepOutJacobian(x, method='fd')
    assert Je.shape == Jf.shape == (P, x.size) and np.isfinite(Je).all()
    D = bo._dY_dtf().reshape(Nv, dim, -1)
    tf_col = np.array([float((raw["jac"][0, p] * D[v]).sum()) for p, (v, _) in enumerate(VO.tolist())]) + raw["jac_tf"][0]
    assert np.abs(Je[:, -1] - tf_col).max() <= 1e-13 * max(1.0, np.abs(tf_col).max()) and np.abs(raw["jac_tf"]).max() > 0
    compared, worst, worst_ref = 0, 0.0, 0.0
    for p, (generic, kind, env, fd) in enumerate(yardstick_gaps(bo, x)):
        if not generic:
            continue
        compared += 1
        ref_gap, gap = float(np.abs(env - fd).max()), float(np.abs(Je[p] - Jf[p]).max())
        ref_tf, gap_tf = abs(env[-1] - fd[-1]), abs(Je[p, -1] - Jf[p, -1])
        worst, worst_ref = max(worst, gap), max(worst_ref, ref_gap)
        print("%s row %d (%s): device |envelope - fd| %.3e (tf column %.3e), yardstick's %.3e (tf column %.3e)"
              % (name, p, kind, gap, gap_tf, ref_gap, ref_tf))
        assert gap <= 2.0 * ref_gap + 1e-9, (name, p)
    print("%s: largest device gap %.3e, largest yardstick gap %.3e, %d of %d rows compared" % (name, worst, worst_ref, compared, P))
    assert compared == P, "the guesses were chosen with generic rows only"


def test_bezier_clearance_with_a_motion():
    """Bezier.keepOutClearance(motion=..): the motion cut down to the curve's span on the host, then r = 1 -- the free-curve
    call on the restricted control points, and within the search's tolerance the context call at r = span / T."""
    from optimalbeziertrajectorygeneration_amd import _capi, bezier
    A, b = K.unit_square()
    H = np.hstack((A, b[:, None]))
    P = np.array([[-3.0, 0.5, 1.0, 4.0], [2.5, -1.0, 3.0, 0.5]])
    Q = np.array([[0.0, 2.0, -1.0], [0.5, 0.0, 1.5]])
    curve, motion = bezier.Bezier(P, t0=0.0, tf=2.0), bezier.Bezier(Q, t0=0.0, tf=5.0)
    val, t = curve.keepOutClearance(A, b, motion=motion)
    ctx = _capi.Context(1, 2, 3, 0, device=0)
    try:
        Qr = ctx.bern_restrict(Q, (0.0, 5.0), (0.0, 2.0))
        f = ctx.bern_keep_out_moving(P, H, Qr, eps_rel=1e-12)
        assert (val, t) == (float(f["val"][0]), float(f["t_star"][0]))
        g = ctx.bern_keep_out_moving(P, H, Q, 0.4, eps_rel=1e-12)
        assert abs(val - g["val"][0]) <= 1e-11
    finally:
        ctx.close()
    ref = MK.searched_row(P, Q, 5.0, 2.0, H)
    assert abs(val - ref["val"]) <= 2 * ref["tol"] + 1e-13
    still, _ = curve.keepOutClearance(A, b)
    assert still != val


# ------------------------------------------------------------------------------------------------ 8. the example
def test_example_solves_end_feasible():
    """example23: both scenes end feasible under both Jacobians, every clearance >= -1e-9 as trueKeepOutClearances of the
    scene's own (moving) square says; without the obstacle car 0 is inside the square at some moment in both scenes.
    Measured on the MI355X: parked tf 4.134170344 under both methods (11 and 10 iterations), crossing 2.971259128 (22 and 20),
    smallest clearance -1.3e-11."""
    import example22_keep_out_obstacles as ex22
    import example23_moving_obstacle as ex
    _, free = ex22.solve(None)
    assert free.success
    for scene in ex.SCENES:
        c_free = ex.clearances(scene, free.x)["val"]
        assert c_free.min() < 0.0, "the unconstrained optimum must drive through the square"
        for method in ('fd', 'envelope'):
            _, res = ex.solve(scene, method, free.x)
            c = ex.clearances(scene, res.x)
            print("%s, %r: tf %.9f (%d iterations, status %d), clearances %s at s = %s"
                  % (scene, method, res.fun, res.nit, res.status, c["val"].tolist(), c["t_star"].tolist()))
            assert res.success and (c["val"] >= -1e-9).all(), (scene, method)
