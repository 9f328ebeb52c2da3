"""The reduced separation forms on non-finite control points (include/obtg.h, "Non-finite control points"): every entry
point that returns a pair's minimum, or its k smallest control points, in every launch form, against the device's OWN full
rows of the same context through the NumPy expectation of tests/nonfinite_rows_ref.py -- a clean row (all elements finite)
keeps the bits of its minimum, a dirty one (any NaN or +-inf element) is NaN, and the active form's indices stay 0 .. k-1
there.  Batch row 0 is never planted: every comparison also shows clean rows keeping their bits beside dirty ones.  The shapes
of tests/golden/nonfinite_rows.npz are compared with the reference's values as well (NaN in the same places).

Which kernel a case reaches (bern_kernels.hip unless named; constraint_rows_ref.sep_form is asserted per case):
  temporal_sep_min[_range][_dev]   dispatch_ns<0, true> -> k_normsq_elev<.., MINONLY, ELEV> (normsq_elev_body, bern_device.h),
                                   staged whole, by slots, in row-window tiles; any degree: generic_normsq_elev_tail, min_only
  temporal_sep_active[_dev]        the same kernels' Smallest4 epilogue; any degree: k_select_smallest over the full rows
  temporal_sep_fd_min_rows_dev     k_tsep_fd, min_only;  temporal_sep_min_dev inside a view: k_normsq_elev<MINONLY> with p.fd
  one_vs_many_min[_spans][_dev]    one_vs_many_value; any degree with spans: k_generic_one_vs_many_spans -> the generic tail
All of them reduce through RowMin (bern_device.h).

Against the library of the commit before RowMin the assertions below failed as the code predicted (run once, on MI355X):
see DESIGN.md 4.5b for the list.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_rows_ref as C  # noqa: E402
import nonfinite_rows_ref as NF  # noqa: E402
from util import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

MS = NF.MAX_SEP
B = NF.B
assert B == 2


@pytest.fixture(scope="module")
def capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    assert _capi.device_count() > 0, "these tests need the GPU"
    return _capi


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def fix(golden_dir):
    return np.load(os.path.join(golden_dir, "nonfinite_rows.npz"))


class Checks(object):
    """Every comparison of one test is made; then the failures raise together."""

    def __init__(self):
        self.n, self.failed = 0, []

    def same(self, got, want, what):
        self.n += 1
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape or not np.array_equal(got, want, equal_nan=True):
            detail = ""
            if got.shape == want.shape and got.dtype.kind == "f":
                bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
                detail = " (%d of %d differ; first: got %r, want %r)" % (int(bad.sum()), got.size, got[bad].ravel()[0], want[bad].ravel()[0])
            elif got.shape == want.shape:
                bad = got != want
                detail = " (%d of %d differ; first: got %r, want %r)" % (int(bad.sum()), got.size, got[bad].ravel()[0], want[bad].ravel()[0])
            self.failed.append(what + detail)

    def true(self, cond, what):
        self.n += 1
        if not cond:
            self.failed.append(what)

    def done(self):
        assert not self.failed, "%d of %d comparisons failed:\n%s" % (len(self.failed), self.n, "\n".join(self.failed[:40]))


def _cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan_out(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _reduced_forms(ck, torch, ctx, Yb, what, rng=None, ks=(1, 2, 3, 4)):
    """Every reduced form of the context on the batch Yb against its own full rows; rng = (pair_begin, pair_count): the
    device entry points on that range only (the host ones take every pair)."""
    P = ctx.num_pairs
    L = ctx.len_temporal_sep // P
    nb = Yb.shape[0]
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        dY = _cuda(torch, Yb)
        b0, cnt = rng if rng is not None else (0, P)
        full = _nan_out(torch, (nb, cnt * L))
        ctx.temporal_sep_dev(dY.data_ptr(), nb, MS, full.data_ptr(), b0, cnt)
        mdev = _nan_out(torch, (nb, cnt))
        ctx.temporal_sep_min_dev(dY.data_ptr(), nb, MS, mdev.data_ptr(), b0, cnt)
        adev = {}
        for k in ks:
            v = _nan_out(torch, (nb, cnt * k))
            i = torch.full((nb, cnt * k), -7, dtype=torch.int32, device="cuda")
            v_only = _nan_out(torch, (nb, cnt * k))
            ctx.temporal_sep_active_dev(dY.data_ptr(), nb, MS, k, v.data_ptr(), i.data_ptr(), b0, cnt)
            ctx.temporal_sep_active_dev(dY.data_ptr(), nb, MS, k, v_only.data_ptr(), None, b0, cnt)
            adev[k] = (v, i, v_only)
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    full = full.cpu().numpy().reshape(nb, cnt, L)
    want_min = NF.reduced_min(full)
    dirty = ~NF.clean(full)
    ck.same(mdev.cpu().numpy(), want_min, "%s: temporal_sep_min_dev" % what)
    for k, (v, i, v_only) in adev.items():
        wv, wi = NF.reduced_active(full, k)
        ck.same(v.cpu().numpy().reshape(nb, cnt, k), wv, "%s: temporal_sep_active_dev k = %d, values" % (what, k))
        ck.same(i.cpu().numpy().reshape(nb, cnt, k), wi, "%s: temporal_sep_active_dev k = %d, indices" % (what, k))
        ck.same(v_only.cpu().numpy(), v.cpu().numpy(), "%s: temporal_sep_active_dev k = %d without indices" % (what, k))
    ck.same(adev[1][0].cpu().numpy(), mdev.cpu().numpy(), "%s: active k = 1 is temporal_sep_min" % what)
    if rng is None:
        host_full = ctx.temporal_sep(Yb, MS).reshape(nb, P, L)
        ck.same(host_full, full, "%s: temporal_sep host and _dev" % what)
        ck.same(ctx.temporal_sep_min(Yb, MS), want_min, "%s: temporal_sep_min" % what)
        begin, count = P // 3 + 1, max(1, P // 2)
        ck.same(ctx.temporal_sep_min(Yb, MS, begin, count), want_min[:, begin:begin + count], "%s: temporal_sep_min over pairs [%d, %d)" % (what, begin, begin + count))
        for k in ks:
            v, i = ctx.temporal_sep_active(Yb, MS, k, True)
            wv, wi = NF.reduced_active(full, k)
            ck.same(v.reshape(nb, P, k), wv, "%s: temporal_sep_active k = %d, values" % (what, k))
            ck.same(i.reshape(nb, P, k), wi, "%s: temporal_sep_active k = %d, indices" % (what, k))
            ck.true(bool((i >= 0).all() and (i < L).all()), "%s: temporal_sep_active k = %d, an index outside 0 .. %d" % (what, k, L - 1))
    return full, dirty


def _shape_inputs(N, d, n, R, M):
    if (N, d, n, M) == (NF.FIX_ROWS["n_veh"], NF.FIX_ROWS["dim"], NF.FIX_ROWS["deg"], 0):
        return NF.fixture_rows_input(None)
    return NF.batch(5000 + 10 * n + R, N, d, n)


ALL_SHAPES = [(s, "k_normsq_elev<MINONLY%s>" % (", ELEV" if s[4] else "")) for s in NF.FAST_SHAPES] + \
             [(s, "k_generic_normsq_elev") for s in NF.GENERIC_SHAPES]


@pytest.mark.parametrize("case,kernel", ALL_SHAPES, ids=[c[0][0] for c in ALL_SHAPES])
def test_min_and_active_on_planted_rows(capi, torch, case, kernel):
    name, N, d, n, R, M = case
    f = C.sep_form(N + M, d, n, R, B, min_only=True)
    assert f["kernel"] == kernel and (f["staging"] == "whole" or "generic" in kernel), f
    if name.startswith("nc 11"):
        assert (N + M) * (N + M - 1) // 2 > 64 and f["waves"] >= 2, f
    ck = Checks()
    Y0 = _shape_inputs(N, d, n, R, M)
    obs = C.point_obstacles(8, M, d) if M else None
    veh1_pairs = np.array([1 in p for p in C.all_pairs(N + M)])
    ctx = capi.Context(N, d, n, R, point_obs=obs)
    try:
        full0, dirty0 = _reduced_forms(ck, torch, ctx, Y0, "nothing planted")
        ck.true(not dirty0.any(), "nothing planted: a dirty row")
        for what in NF.PLANTINGS:
            full, dirty = _reduced_forms(ck, torch, ctx, NF.plant(Y0, what, d), what)
            ck.true(not dirty[0].any(), "%s: batch row 0 has a dirty pair" % what)
            ck.same(dirty[1], veh1_pairs, "%s: the dirty pairs of batch row 1 are not the pairs of vehicle 1" % what)
            ck.same(full[0], full0[0], "%s: batch row 0's full rows moved" % what)
            ck.same(full[1][~veh1_pairs], full0[1][~veh1_pairs], "%s: a clean pair's full row moved" % what)
    finally:
        ctx.close()
    if M:
        ctx = capi.Context(N, d, n, R, point_obs=NF.plant_obstacle(obs))
        try:
            full, dirty = _reduced_forms(ck, torch, ctx, Y0, NF.OBSTACLE_PLANTING)
            obs_pairs = np.array([N in p for p in C.all_pairs(N + M)])
            for b in range(B):
                ck.same(dirty[b], obs_pairs, "%s: row %d, the dirty pairs are not the pairs of that obstacle" % (NF.OBSTACLE_PLANTING, b))
            ck.same(full[:, ~obs_pairs], full0[:, ~obs_pairs], "%s: a clean pair's full row moved" % NF.OBSTACLE_PLANTING)
        finally:
            ctx.close()
    ck.done()


@pytest.mark.parametrize("sep_case,staging", NF.STAGED, ids=[s[0] for s in NF.STAGED])
def test_min_and_active_slot_staged_and_tiled(capi, torch, sep_case, staging):
    """The reduced launch with the objects staged by slots / in row-window tiles (plan_temporal_sep): the smallest entries
    of constraint_rows_ref.SEP_CASES whose plan answers so with min_only."""
    name, N, d, n, R, M, kind, _b, rng, _want = [c for c in C.SEP_CASES if c[0] == sep_case][0]
    f = C.sep_form(N + M, d, n, R, B, *(rng or (0, None)), min_only=True)
    assert f["staging"] == staging and f["kernel"].startswith("k_normsq_elev<MINONLY"), f
    ck = Checks()
    Y0 = NF.batch(6000 + n + R, N, d, n)
    pairs = C.all_pairs(N)
    b0, cnt = rng if rng is not None else (0, len(pairs))
    veh1_pairs = np.array([1 in p for p in pairs[b0:b0 + cnt]])
    assert veh1_pairs.any() and not veh1_pairs.all()
    ctx = capi.Context(N, d, n, R)
    try:
        for what in ("nan at a middle control point", "+inf at the last control point", "two control points of +-1e200"):
            full, dirty = _reduced_forms(ck, torch, ctx, NF.plant(Y0, what, d), what, rng=(b0, cnt), ks=(1, 3))
            ck.true(not dirty[0].any(), "%s: batch row 0 has a dirty pair" % what)
            ck.same(dirty[1], veh1_pairs, "%s: the dirty pairs of batch row 1 are not the pairs of vehicle 1" % what)
    finally:
        ctx.close()
    ck.done()


@pytest.mark.parametrize("R", NF.FIX_ROWS["elevs"])
def test_fixture_shape_against_the_reference(capi, fix, R):
    """4 vehicles, 2-D, degree 5 at DEG_ELEV 0 and 6 on the fixture's inputs: temporal_sep_min and the active form's k = 1 are
    NaN where the reference's rows (optimization.py:311-346) have a non-finite element, and within 1e-9 of their minimum elsewhere."""
    f = NF.FIX_ROWS
    ctx = capi.Context(f["n_veh"], f["dim"], f["deg"], R)
    try:
        for i, what in enumerate((None,) + NF.PLANTINGS):
            Yb = NF.fixture_rows_input(what)
            ref = NF.reduced_min(fix["rows_R%d" % R][i])
            assert np.isnan(ref).any() == (what is not None)
            assert_close(ctx.temporal_sep_min(Yb, MS), ref, what="temporal_sep_min, %s" % what)
            assert_close(ctx.temporal_sep_active(Yb, MS, 1), ref, what="temporal_sep_active k = 1, %s" % what)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
#  finite-difference forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NF.FD_SHAPES, ids=["R = %d" % s[3] for s in NF.FD_SHAPES])
def test_fd_min_rows_and_min_inside_a_view(capi, torch, shape):
    """NaN (and the other plantings) in Y0: temporal_sep_min_dev inside fd_view_begin / _end and temporal_sep_fd_min_rows_dev
    against the full rows of the materialised batch."""
    from optimalbeziertrajectorygeneration_amd import synth
    N, d, n, R = shape
    h = 1e-3
    ck = Checks()
    Y0 = NF.fixture_rows_input(None)[1]
    nb = N * d * (n - 1) + 1
    pairs = C.all_pairs(N)
    ctx = capi.Context(N, d, n, R)
    try:
        P = ctx.num_pairs
        L = ctx.len_temporal_sep // P
        for what in (None,) + NF.PLANTINGS:
            Y = Y0 if what is None else NF.plant_rows(Y0, what, d)
            Yb = synth.fd_batch(Y, h=h)
            assert Yb.shape[0] == nb
            full = ctx.temporal_sep(Yb, MS).reshape(nb, P, L)
            want = NF.reduced_min(full)
            ck.same(ctx.temporal_sep_min(Yb, MS), want, "%s: temporal_sep_min of the materialised batch" % what)
            if what is not None:
                ck.same(np.isnan(want), np.tile([1 in p for p in pairs], (nb, 1)), "%s: the dirty pairs are not vehicle 1's in every row" % what)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            try:
                d0 = _cuda(torch, Y)
                inside = _nan_out(torch, (nb, P))
                ctx.fd_view_begin(d0.data_ptr(), 1, h, nb)
                try:
                    ctx.temporal_sep_min_dev(None, nb, MS, inside.data_ptr())
                finally:
                    ctx.fd_view_end()
                comp = _nan_out(torch, (nb - 1, N - 1))
                ctx.temporal_sep_fd_min_rows_dev(d0.data_ptr(), 1, h, 1, nb - 1, MS, comp.data_ptr())
                torch.cuda.synchronize()
            finally:
                ctx.use_own_stream()
            ck.same(inside.cpu().numpy(), want, "%s: temporal_sep_min_dev inside the view" % what)
            comp = comp.cpu().numpy()
            for g in range(1, nb):
                v = ((g - 1) // (n - 1)) // d                     # the vehicle batch row g advances
                mine = [pairs.index((min(v, u), max(v, u))) for u in range(N) if u != v]
                ck.same(comp[g - 1], want[g, mine], "%s: temporal_sep_fd_min_rows_dev row %d" % (what, g))
    finally:
        ctx.close()
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------
#  one curve against K others
# ---------------------------------------------------------------------------------------------------------------------
def _pair_rows(capi, one, many, d, n, R, max_sep):
    """The full rows of the pairs (one_b, many_k), [B][K][2n + R + 1]: obtg_temporal_sep of a context of K + 1 vehicles,
    candidate first, whose first K lexicographic pairs are those."""
    K = many.shape[0]
    ctx = capi.Context(K + 1, d, n, R)
    try:
        Y = np.empty((one.shape[0], (K + 1) * d, n + 1))
        Y[:, :d] = one
        Y[:, d:] = many.reshape(K * d, n + 1)
        L = ctx.len_temporal_sep // ctx.num_pairs
        return ctx.temporal_sep(Y, max_sep).reshape(one.shape[0], ctx.num_pairs, L)[:, :K].copy()
    finally:
        ctx.close()


def _one_many_inputs(d, n, what):
    if (d, n) == (NF.FIX_SEQ["dim"], NF.FIX_SEQ["deg"]):
        return NF.fixture_seq_input(what)
    Yb = C.rows_batch(7400 + n, 3, 6, d, n, "full") * 0.25
    one, many = Yb[:, :d].copy(), Yb[0, d:].reshape(5, d, n + 1).copy()
    if what is not None:
        one = NF.plant(one, what, d, veh=0)
        many[2] = NF.plant_rows(many[2], what, d, veh=0)
    return np.ascontiguousarray(one), many


def _one_many_dev(torch, ctx, one, many, spans=None, no_overlap=None):
    nb, K = one.shape[0], many.shape[0]
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        do, dm = _cuda(torch, one), _cuda(torch, many)
        out = _nan_out(torch, (nb, K))
        if spans is None:
            ctx.one_vs_many_min_dev(do.data_ptr(), nb, dm.data_ptr(), K, MS, out.data_ptr())
        else:
            ctx.one_vs_many_min_spans_dev(do.data_ptr(), spans[0], nb, dm.data_ptr(), spans[1], K, MS, out.data_ptr(), no_overlap)
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    return out.cpu().numpy()


def _cut(row, t0, tf, a, e):
    """bern_kernels.hip SpanCut + restrict_row on one coordinate row (a copy): de Casteljau down to [a, e]"""
    p = np.array(row, dtype=np.float64)
    nc = p.size
    with np.errstate(all="ignore"):
        if t0 < a:
            z = (a - t0) / (tf - t0)
            for lev in range(1, nc):
                for i in range(nc - lev):
                    p[i] = (1.0 - z) * p[i] + z * p[i + 1]
            t0 = a
        if tf > e:
            z = (e - t0) / (tf - t0)
            for lev in range(1, nc):
                for i in range(nc - 1, lev - 1, -1):
                    p[i] = (1.0 - z) * p[i - 1] + z * p[i]
    return p


def _cut_pair_is_dirty(o, so, m, sm):
    """Does the squared distance of the two curves, cut to the overlap of their spans, have a non-finite coefficient?  (Every
    product of two coefficients of the difference enters one with a positive weight.)"""
    a, e = max(so[0], sm[0]), min(so[1], sm[1])
    with np.errstate(all="ignore"):
        dv = np.stack([_cut(o[q], so[0], so[1], a, e) - _cut(m[q], sm[0], sm[1], a, e) for q in range(o.shape[0])])
        return not (np.isfinite(dv).all() and np.isfinite(dv[:, :, None] * dv[:, None, :]).all())


@pytest.mark.parametrize("case", NF.ONE_MANY, ids=["R = %d" % c[2] for c in NF.ONE_MANY])
def test_one_vs_many_min(capi, torch, fix, case):
    """one_vs_many_min[_dev] and, on equal spans, one_vs_many_min_spans[_dev]: NaN in candidate 1 and in many[2].  R = 10 is the
    shape of the fixture: also against the reference's own function (Examples/SequentialSwarm.py:43-70, max_sep 1)."""
    d, n, R, nb, K = case
    ck = Checks()
    ctx = capi.Context(1, d, n, R)
    try:
        for i, what in enumerate((None,) + NF.PLANTINGS):
            one, many = _one_many_inputs(d, n, what)
            assert one.shape == (nb, d, n + 1) and many.shape == (K, d, n + 1)
            want = NF.reduced_min(_pair_rows(capi, one, many, d, n, R, MS))
            planted = np.zeros((nb, K), bool)
            if what is not None:
                planted[1, :] = True
                planted[:, 2] = True
                if "1e200" in what:
                    planted[1, 2] = False                        # the same +-1e200 in both curves: their difference is 0 there
            ck.same(np.isnan(want), planted, "%s: the dirty pairs of the full rows" % what)
            got = ctx.one_vs_many_min(one, many, MS)
            ck.same(got, want, "%s: one_vs_many_min" % what)
            ck.same(_one_many_dev(torch, ctx, one, many), want, "%s: one_vs_many_min_dev" % what)
            so, sm = np.tile([0.5, 4.0], (nb, 1)), np.tile([0.5, 4.0], (K, 1))
            ck.same(ctx.one_vs_many_min_spans(one, so, many, sm, MS, 1e6), want, "%s: one_vs_many_min_spans, equal spans" % what)
            ck.same(_one_many_dev(torch, ctx, one, many, (so, sm), 1e6), want, "%s: one_vs_many_min_spans_dev, equal spans" % what)
            if R == NF.FIX_SEQ["elev"]:
                ref = fix["seq_out"][i]
                got1 = ctx.one_vs_many_min(one, many, NF.FIX_SEQ["max_sep"])
                try:
                    assert_close(got1, ref, what="%s against the reference" % what)
                    ck.true(True, "")
                except AssertionError as e:
                    ck.true(False, str(e))
    finally:
        ctx.close()
    ck.done()


SPAN_CASES = [c[:3] for c in NF.ONE_MANY] + [NF.ONE_MANY_GENERIC[:3]]


@pytest.mark.parametrize("d,n,R", SPAN_CASES, ids=["%d-D deg %d R = %d" % c for c in SPAN_CASES])
def test_one_vs_many_min_spans_cut_and_without_overlap(capi, torch, d, n, R):
    """Spans that cut both curves of every pair, and one pair without overlap whose curve holds the planting: that pair
    returns no_overlap whatever its control points hold (the reference returns None before it looks at them); an overlapping
    pair is NaN exactly when the cut curves' squared distance has a non-finite coefficient, and keeps its unplanted bits
    otherwise.  deg 12: k_generic_one_vs_many_spans."""
    from optimalbeziertrajectorygeneration_amd import _capi as cap
    nb, K = 3, 5
    assert bool(cap.fast_kernels(d, n) & 1) == (n != 12)
    NO = 1e6
    so = np.array([[0.0, 5.0], [1.0, 6.0], [0.5, 4.5]])
    sm = np.array([[2.0, 8.0], [0.25, 3.0], [1.5, 4.0], [0.75, 9.0], [2.5, 7.0]])
    sm_apart = sm.copy()
    sm_apart[2] = [6.0, 7.5]                                      # many[2] (planted) after candidates 0 and 2: no overlap; it touches candidate 1
    ck = Checks()
    ctx = capi.Context(1, d, n, R)
    try:
        one0, many0 = _one_many_inputs(d, n, None)
        base = {}
        for tag, spans in (("cut", (so, sm)), ("apart", (so, sm_apart))):
            base[tag] = ctx.one_vs_many_min_spans(one0, spans[0], many0, spans[1], MS, NO)
            overlap = np.array([[max(a[0], b[0]) < min(a[1], b[1]) for b in spans[1]] for a in spans[0]])
            ck.true(bool(np.isfinite(base[tag]).all()), "%s, nothing planted: a non-finite value" % tag)
            ck.same(base[tag] == NO, ~overlap, "%s, nothing planted: no_overlap" % tag)
        assert (base["apart"][:, 2] == NO).all() and (base["cut"] != NO).all()
        for what in NF.PLANTINGS:
            one, many = _one_many_inputs(d, n, what)
            for tag, spans in (("cut", (so, sm)), ("apart", (so, sm_apart))):
                overlap = base[tag] != NO
                dirty = np.array([[overlap[b, k] and _cut_pair_is_dirty(one[b], spans[0][b], many[k], spans[1][k]) for k in range(K)]
                                  for b in range(nb)])
                touched = np.zeros((nb, K), bool)
                touched[1, :] = True
                touched[:, 2] = True
                ck.same(dirty, touched & overlap, "%s, %s: the pairs with a planted curve that overlap are not the dirty ones" % (what, tag))
                want = np.where(dirty, np.nan, base[tag])
                ck.same(ctx.one_vs_many_min_spans(one, spans[0], many, spans[1], MS, NO), want, "%s, %s: one_vs_many_min_spans" % (what, tag))
                ck.same(_one_many_dev(torch, ctx, one, many, spans, NO), want, "%s, %s: one_vs_many_min_spans_dev" % (what, tag))
    finally:
        ctx.close()
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------
#  the Python layer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["min", "active"])
def test_bezoptimization_rows_and_exact_jacobian_at_a_nan_iterate(capi, rows):
    """An x with one NaN entry (vehicle 1): the closure -- served or direct -- returns NaN for the pairs of vehicle 1 and the
    other pair's bits; temporalSeparationJacobian(method='exact') is NaN in the columns of a NaN row's own vehicles (not the
    finite derivative of the control points the indices happen to name), 0 in the others', and the clean pair's rows are
    those of the unplanted x."""
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization

    def make(**kw):
        return BezOptimization(numVeh=3, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=0.9, tf=6.0,
                               initPoints=[(0, 0), (3, 0), (6, 0.5)], finalPoints=[(6, 6), (0, 6.5), (3, 6)],
                               separationRows=rows, activeRows=3, **kw)
    bo, bo_direct = make(), make(fdBatching=False)
    k = 1 if rows == "min" else 3
    x0 = bo.generateGuess(std=0.3, seed=4)
    cols = 2 * bo._numCols                                          # entries of x per vehicle
    assert x0.size == 3 * cols
    x = x0.copy()
    x[cols + 2] = np.nan
    ck = Checks()
    ctx = capi.Context(3, 2, 5, 0)
    try:
        full, full0 = ctx.temporal_sep(np.stack([bo.reshapeVector(x), bo.reshapeVector(x0)]), 0.9).reshape(2, 3, 11)
    finally:
        ctx.close()
    dirty = np.array([True, False, True])                           # pairs (0,1) (0,2) (1,2)
    ck.same(~NF.clean(full), dirty, "the dirty pairs")
    ck.true(bool(NF.clean(full0).all()), "a dirty pair at the clean x")

    def reduced(r):
        return NF.reduced_min(r) if rows == "min" else NF.reduced_active(r, k)[0].ravel()
    for name, b in (("fdBatching", bo), ("direct", bo_direct)):
        ck.same(b.temporalSeparationConstraints(x), reduced(full), "%s closure, separationRows=%r" % (name, rows))
        ck.same(b.temporalSeparationConstraints(x0), reduced(full0), "%s closure at the clean x" % name)
    J, J0 = bo.temporalSeparationJacobian(x, method='exact'), bo.temporalSeparationJacobian(x0, method='exact')
    ck.true(J.shape == (3 * k, x.size) and bool(np.isfinite(J0).all()), "shape of the exact Jacobian / a non-finite entry at the clean x")
    own = {0: (0, 1), 1: (0, 2), 2: (1, 2)}
    for p in range(3):
        blk = J[p * k:(p + 1) * k]
        if not dirty[p]:
            ck.same(blk, J0[p * k:(p + 1) * k], "pair %d is clean: its rows are those of the unplanted x" % p)
            continue
        for v in range(3):
            part = blk[:, v * cols:(v + 1) * cols]
            if v in own[p]:
                ck.true(bool(np.isnan(part).all()), "pair %d is NaN: a finite derivative in the columns of its vehicle %d" % (p, v))
            else:
                ck.true(bool((part == 0).all()), "pair %d: a non-zero entry in the columns of vehicle %d" % (p, v))
    ck.done()


@pytest.mark.parametrize("deg", [5, 12], ids=["deg 5: one_vs_many_min", "deg 12: the any-degree fallback"])
def test_sequential_planner_constraint_at_nan_trajectories(capi, deg):
    """sequential.temporalSeparationConstraints and new_vs_all (3-D, elev(10)): degree 5 runs obtg_one_vs_many_min, degree 12
    the fallback through temporal_sep_min of a context of K + 1 vehicles; with spans both run obtg_one_vs_many_min_spans."""
    from optimalbeziertrajectorygeneration_amd import sequential as SS
    d, R, K = 3, 10, 5
    ck = Checks()
    for what in (None, "nan at a middle control point", "whole vehicle nan", "+inf at the last control point"):
        one, many = _one_many_inputs(d, deg, what)
        want = NF.reduced_min(_pair_rows(capi, one, many, d, deg, R, MS))
        traj = many.reshape(K * d, deg + 1)
        if what is not None:
            ck.true(bool(np.isnan(want[1]).all() and np.isnan(want[:, 2]).all() and np.isfinite(np.delete(want[[0, 2]], 2, axis=1)).all()),
                    "%s: the dirty pairs" % what)
        ck.same(SS.new_vs_all(one, traj, d, MS, degElev=R), want, "%s: new_vs_all" % what)
        for b in range(one.shape[0]):
            y = np.concatenate([one[b], traj])
            ck.same(SS.temporalSeparationConstraints(y, K + 1, d, MS, degElev=R), want[b], "%s: temporalSeparationConstraints, candidate %d" % (what, b))
        spans = np.tile([0.0, 3.0], (K, 1))
        spans[2] = [4.0, 5.0]                                       # the planted trajectory is not in the air with the new one
        got = SS.new_vs_all(one, traj, d, MS, degElev=R, spans=spans, new_span=(0.0, 3.0))
        want_sp = want.copy()
        want_sp[:, 2] = SS.NO_OVERLAP
        ck.same(got, want_sp, "%s: new_vs_all with spans, trajectory 2 without overlap" % what)
    ck.done()
