"""Separation minima of trajectories on different time spans on the MI355X: obtg_one_vs_many_min_spans[_dev] and
obtg_bern_restrict, `Bezier.add / sub(align=True)`, `_temporalAlignment` and the sequential planner's spans, held to the
reference's own values (tests/golden/aligned.npz, written by tests/golden/gen_aligned.py) at the project's 1e-9
(tests/util.py), to obtg_one_vs_many_min bit for bit where no curve is cut, and to SciPy's finite differences."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aligned_ref as A  # noqa: E402
from util import assert_close  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligned.npz")


def _capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    return _capi


def _groups(fx):
    return [(str(g), int(d), int(n)) for g, d, n in zip(fx["groups"], fx["dims"], fx["degs"])]


def _spans(rng, n):
    """n spans in [0, 10]: sorted uniform pairs, every fourth one a copy of its neighbour's start or end"""
    s = np.sort(rng.uniform(0.0, 10.0, size=(n, 2)), axis=1)
    s[:, 1] = np.maximum(s[:, 1], s[:, 0] + 0.25)
    for i in range(3, n, 4):
        s[i, (i // 4) % 2] = s[i - 1, (i // 4) % 2]
        if not s[i, 0] < s[i, 1]:
            s[i] = s[i - 1]
    return s


@pytest.mark.gpu
def test_minima_are_the_references():
    """every fixture pair (the diagonal of a B x K call of all first curves against all second curves), R in {0, 10}: 1e-9
    where the spans overlap, the caller's no_overlap value exactly where the reference returned None -- for two such
    values -- and nowhere else.  The degree-4 group runs the runtime-degree form."""
    capi, fx = _capi(), np.load(GOLDEN)
    max_sep = float(fx["max_sep"])
    assert not (capi.fast_kernels(3, 4) & 1)
    for g, dim, deg in _groups(fx):
        c1, c2, s1, s2, none = (fx[g + k] for k in ("_c1", "_c2", "_s1", "_s2", "_none"))
        for R in (int(r) for r in fx["elevs"]):
            ctx = capi.Context(1, dim, deg, R, device=capi.default_device())
            try:
                tables = [ctx.one_vs_many_min_spans(c1, s1, c2, s2, max_sep, no_overlap=v) for v in (np.inf, 12345.0)]
                assert np.isinf(ctx.one_vs_many_min_spans(c1, s1, c2, s2, max_sep)[0, 0]) == bool(
                    max(s1[0, 0], s2[0, 0]) >= min(s1[0, 1], s2[0, 1]))          # (the default is inf)
            finally:
                ctx.close()
            ref = fx["%s_min%d" % (g, R)]
            for v, full in zip((np.inf, 12345.0), tables):
                assert full.shape == (len(none), len(none))
                got = np.diagonal(full)
                assert ((got == v) == none).all(), "%s R=%d: the no-overlap mask differs" % (g, R)
                worst = assert_close(got[~none], ref[~none], what="%s R=%d minima vs the reference" % (g, R))
                # the whole table's mask: a >= e, touching spans included
                a = np.maximum(s1[:, None, 0], s2[None, :, 0])
                e = np.minimum(s1[:, None, 1], s2[None, :, 1])
                assert ((full == v) == (a >= e)).all(), "%s R=%d: mask of the whole table" % (g, R)
            assert np.array_equal(tables[0][np.isfinite(tables[0])], tables[1][np.isfinite(tables[0])])
            # off the diagonal: a block against the restatement (itself held to the reference by test_aligned_ref.py)
            blk = A.one_vs_many(c1[:6], s1[:6], c2[20:40], s2[20:40], R, max_sep)
            assert_close(tables[0][:6, 20:40], blk, what="%s R=%d block vs the restatement" % (g, R))
            print("%s R=%d: %d pairs with overlap, worst scaled error %.2e" % (g, R, int((~none).sum()), worst))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("R", [0, 10])
def test_equal_spans_take_no_split(dim, R):
    """all spans equal: no curve is cut, and the values are obtg_one_vs_many_min's bit for bit"""
    capi = _capi()
    rng = np.random.default_rng(40 + dim + R)
    for deg in (3, 5, 10):
        one = rng.uniform(-5, 5, size=(7, dim, deg + 1))
        many = rng.uniform(-5, 5, size=(150, dim, deg + 1))
        ctx = capi.Context(1, dim, deg, R, device=capi.default_device())
        try:
            ref = ctx.one_vs_many_min(one, many, 0.9)
            for span in ((0.0, 1.0), (2.5, 9.75)):
                got = ctx.one_vs_many_min_spans(one, np.tile(span, (7, 1)), many, np.tile(span, (150, 1)), 0.9)
                assert np.array_equal(got, ref), "dim %d degree %d R %d span %s" % (dim, deg, R, span)
        finally:
            ctx.close()


@pytest.mark.gpu
def test_table_is_its_rows_and_dev_is_host():
    """a B x K call == its rows computed one candidate at a time, bit for bit, with K changing between calls on ONE context
    (specialised and runtime-degree form); the _dev form on torch tensors == the host form"""
    import torch
    capi = _capi()
    rng = np.random.default_rng(77)
    for dim, deg in ((3, 5), (2, 10), (3, 4)):
        ctx = capi.Context(1, dim, deg, 10, device=capi.default_device())
        try:
            one, so = rng.uniform(-5, 5, size=(9, dim, deg + 1)), _spans(rng, 9)
            many, sm = rng.uniform(-5, 5, size=(300, dim, deg + 1)), _spans(rng, 300)
            for K in (1, 5, 29, 300, 64):
                full = ctx.one_vs_many_min_spans(one, so, many[:K], sm[:K], 0.9, no_overlap=1.0e6)
                assert full.shape == (9, K)
                for b in range(9):
                    row = ctx.one_vs_many_min_spans(one[b], so[b], many[:K], sm[:K], 0.9, no_overlap=1.0e6)
                    assert np.array_equal(full[b], row[0]), (dim, deg, K, b)
                d_one, d_many = torch.from_numpy(one).cuda(), torch.from_numpy(many[:K].copy()).cuda()
                d_out = torch.full((9, K), -1.0, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                ctx.one_vs_many_min_spans_dev(d_one.data_ptr(), so, 9, d_many.data_ptr(), sm[:K], K, 0.9, d_out.data_ptr(),
                                              no_overlap=1.0e6)
                ctx.sync()
                assert np.array_equal(d_out.cpu().numpy(), full), (dim, deg, K)
            assert (full == 1.0e6).any() and (full != 1.0e6).any()
        finally:
            ctx.close()


@pytest.mark.gpu
def test_alignment_add_sub_and_argument_errors():
    """obtg_bern_restrict / _temporalAlignment against the reference's aligned control points, add / sub(align=True)
    against its sums and differences (None where it returned None), and the argument errors"""
    capi, fx = _capi(), np.load(GOLDEN)
    from optimalbeziertrajectorygeneration_amd import bezier
    ctx = capi.scratch_context()
    for g, dim, deg in _groups(fx):
        c1, c2, s1, s2, none = (fx[g + k] for k in ("_c1", "_c2", "_s1", "_s2", "_none"))
        ov = np.flatnonzero(~none)
        ends = fx[g + "_ends"][ov]
        assert np.array_equal(ends[:, 0], np.maximum(s1[ov, 0], s2[ov, 0])) and np.array_equal(ends[:, 1], np.minimum(s1[ov, 1], s2[ov, 1]))
        # every overlapping pair's two curves in ONE call: rows = (pair, curve, dimension)
        rows = np.stack([c1[ov], c2[ov]], axis=1).reshape(-1, deg + 1)
        span = np.repeat(np.stack([s1[ov], s2[ov]], axis=1).reshape(-1, 2), dim, axis=0)
        out = ctx.bern_restrict(rows, span, np.repeat(ends, 2 * dim, axis=0)).reshape(len(ov), 2, dim, deg + 1)
        assert_close(out[:, 0], fx[g + "_a1"][ov], what=g + " bern_restrict, first curves")
        assert_close(out[:, 1], fx[g + "_a2"][ov], what=g + " bern_restrict, second curves")
        for i in range(0, len(none), 3):
            b1 = bezier.Bezier(c1[i], t0=s1[i, 0], tf=s1[i, 1])
            b2 = bezier.Bezier(c2[i], t0=s2[i, 0], tf=s2[i, 1])
            dv, sm = b1.sub(b2, align=True), b1.add(b2, align=True)
            assert (dv is None) == (sm is None) == bool(none[i]), (g, i)
            if none[i]:
                continue
            n1, n2 = bezier._temporalAlignment(b1, b2)
            what = "%s pair %d " % (g, i)
            assert (n1.t0, n1.tf) == (n2.t0, n2.tf) == (dv.t0, dv.tf) == (sm.t0, sm.tf) == tuple(fx[g + "_ends"][i]), what
            assert_close(n1.cpts, fx[g + "_a1"][i], what=what + "_temporalAlignment c1")
            assert_close(n2.cpts, fx[g + "_a2"][i], what=what + "_temporalAlignment c2")
            assert_close(dv.cpts, fx[g + "_a1"][i] - fx[g + "_a2"][i], what=what + "sub")
            assert_close(sm.cpts, fx[g + "_add"][i], what=what + "add")
            assert_close(dv.normSquare().elev(10).cpts, fx[g + "_rows10"][i], what=what + "sub.normSquare.elev(10)")
    # a curve that needs no cut comes back as it went in
    row = np.arange(6.0)[None]
    assert np.array_equal(ctx.bern_restrict(row, (1.0, 4.0), (1.0, 4.0)), row)
    # argument errors: a target outside the span, an empty or reversed target; a span with t0 >= tf
    for span, target in (((0.0, 5.0), (-1.0, 4.0)), ((0.0, 5.0), (1.0, 6.0)), ((0.0, 5.0), (2.0, 2.0)), ((0.0, 5.0), (3.0, 2.0))):
        with pytest.raises(capi.ObtgError) as ei:
            ctx.bern_restrict(row, span, target)
        assert ei.value.code == -1, (span, target)
    c35 = capi.Context(1, 3, 5, 10, device=capi.default_device())
    try:
        one, many = np.zeros((2, 3, 6)), np.ones((4, 3, 6))
        good1, good4 = np.tile((0.0, 1.0), (2, 1)), np.tile((0.0, 1.0), (4, 1))
        for bad in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0)):
            b1, b4 = good1.copy(), good4.copy()
            b1[1], b4[3] = bad, bad
            for so, sm in ((b1, good4), (good1, b4)):
                with pytest.raises(capi.ObtgError) as ei:
                    c35.one_vs_many_min_spans(one, so, many, sm, 0.9)
                assert ei.value.code == -1, bad
    finally:
        c35.close()


@pytest.mark.gpu
def test_planner_with_staggered_departures():
    """nonlcon_jac with spans == SciPy's approx_derivative of nonlcon entry for entry (both pairings; rows of pairs that
    are never in the air together are 0 and their constraint value is NO_OVERLAP); a staggered plan of 12 vehicles in the
    crowded volume of the existing planner test runs, and every converged vehicle clears every earlier one on the overlap
    of their spans to -1e-6, that test's criterion."""
    from scipy.optimize._numdiff import approx_derivative
    from optimalbeziertrajectorygeneration_amd import sequential as SS
    nveh = 12
    rng = np.random.default_rng(2)
    fin = 100.0 * np.concatenate([0.35 + 0.3 * rng.random((nveh, 2)), np.ones((nveh, 1))], axis=1)
    t0s = 2.5 * np.arange(nveh)                       # one departure every 2.5 s, 10 s of flight: four vehicles share the air
    t0s[5] = t0s[4]                                   # (two leave together: equal spans inside a staggered plan)
    params = SS.Parameters(nveh, 3, 3, 100.0, 2.5, finalpts=fin, seed=4, t0s=t0s, tfs=t0s + 10.0)
    params.inipts[:, :2] = 35.0 + 30.0 * rng.random((nveh, 2))
    spans = np.stack([params.t0s, params.tfs], axis=1)
    traj, results, _ = SS.plan(params, pairing='new_vs_all', with_jac=True)
    assert traj.shape == (nveh * 3, 4) and len(results) == nveh
    ok = [r.success for r in results]
    # (staggering only takes constraints away from the existing test's problem, whose bound this is)
    assert sum(ok) >= nveh - 4, [r.message for r in results if not r.success]
    for i in range(1, nveh):
        if ok[i]:
            c = SS.new_vs_all(traj[3 * i:3 * i + 3], traj[:3 * i], 3, params.dsafe, spans=spans[:i], new_span=spans[i])
            assert c.min() >= -1e-6, i
            apart = spans[:i, 1] <= spans[i, 0]
            assert (c[0][apart] == SS.NO_OVERLAP).all() and (c[0][~apart] != SS.NO_OVERLAP).all()
    x = SS.initguess(7, params) + rng.normal(0, 0.5, 6)
    for pairing in ('reference', 'new_vs_all'):
        J = SS.nonlcon_jac(x, 7, traj[:21], 8, params, pairing)
        Jn = approx_derivative(lambda z: SS.nonlcon(z, 7, traj[:21], 8, params, pairing), x, method='2-point',
                               abs_step=SS.FD_STEP)
        assert J.shape == Jn.shape == (7, 6) and np.array_equal(J, Jn), pairing
        assert np.isfinite(J).all()
    J = SS.nonlcon_jac(x, 7, traj[:21], 8, params, 'new_vs_all')
    apart = spans[:7, 1] <= spans[7, 0]
    assert apart.any() and (J[apart] == 0).all() and (J[~apart] != 0).any()
    # the spans as a keyword are the parameters' spans
    plain = SS.Parameters(nveh, 3, 3, 100.0, 2.5, finalpts=fin, seed=4)
    plain.inipts[:] = params.inipts
    assert np.array_equal(SS.nonlcon(x, 7, traj[:21], 8, plain, 'new_vs_all', spans=spans), SS.nonlcon(x, 7, traj[:21], 8, params, 'new_vs_all'))
    # without spans the planner's calls are the ones they were
    assert np.array_equal(SS.nonlcon(x, 7, traj[:21], 8, plain, 'new_vs_all'), SS.new_vs_all(
        SS.reshape(x, np.atleast_2d([]), 3, plain.inipts[7], plain.finalpts[7]), traj[:21], 3, plain.dsafe)[0])
