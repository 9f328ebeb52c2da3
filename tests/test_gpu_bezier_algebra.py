"""The single-curve Bernstein kernels (obtg_bern_elev / diff / mul / normsq / split / restrict / eval) and the objectives
(obtg_euclidean_obj / accel_obj / jerk_obj) against exact rationals: every assertion is the element-wise forward bound
|device - exact| <= K * 2^-53 * M of tests/bezier_algebra_ref.py (which tests/test_bezier_algebra_ref.py holds honest on the
CPU), through the _capi call and through the matching Bezier method where there is one.  Shapes: past one stride of the
64-lane row loops, at and around it, unequal degrees, split parameters at and outside the ends, all 1001 samples of
Bezier.curve, the launchers' limits.  Each test prints the largest share of the bound the device used (pytest -s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bezier_algebra_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MANY = 130          # rows of the one many-block call per operation: more blocks than one launch wave of a CU


@pytest.fixture(scope="module")
def ctx():
    from optimalbeziertrajectorygeneration_amd import _capi
    return _capi.scratch_context()


@pytest.fixture(scope="module")
def bez():
    from optimalbeziertrajectorygeneration_amd import bezier
    return bezier


class Shares(object):
    """Every comparison of one test: all are made, the largest share of the bound is printed, then the failures raise."""

    def __init__(self, op):
        self.op, self.worst, self.n, self.failed = op, 0.0, 0, []

    def hold(self, cand, ref, what):
        self.n += 1
        try:
            self.worst = max(self.worst, R.assert_within(cand, ref, "%s %s" % (self.op, what)))
        except AssertionError as e:
            self.failed.append(str(e))

    def same(self, got, want, what):
        self.n += 1
        if not np.array_equal(np.asarray(got), np.asarray(want)):
            self.failed.append("%s %s: not bit for bit" % (self.op, what))

    def done(self):
        print("\n%s: largest share of the bound K * 2^-53 * M used by the device %.3f (%d comparisons)" % (self.op, self.worst, self.n))
        assert not self.failed, "%d of %d comparisons failed:\n%s" % (len(self.failed), self.n, "\n".join(self.failed[:20]))


def curve(bez, cpts, t0=0.0, tf=1.0):
    return bez.Bezier(np.array(cpts, dtype=np.float64, ndmin=2), t0=t0, tf=tf)


# ---------------------------------------------------------------------------------------------------------------------
def test_elev(ctx, bez):
    sh = Shares("elev")
    for (n, Rr), rows in [(s, 4) for s in R.ELEV_SHAPES] + [((10, 54), MANY)]:
        a = R.input_rows(100 + n + Rr, n + 1, rows)
        ref = R.elev(a, Rr)
        for how, out in (("capi", ctx.bern_elev(a, Rr)), ("Bezier", curve(bez, a).elev(Rr).cpts)):
            sh.hold(out, ref, "(%d, %d) x %d %s" % (n, Rr, rows, how))
            sh.same(out[:, 0], a[:, 0], "(%d, %d) %s first coefficient" % (n, Rr, how))
            sh.same(out[:, -1], a[:, -1], "(%d, %d) %s last coefficient" % (n, Rr, how))
    sh.done()


def test_mul(ctx, bez):
    sh = Shares("mul")
    for (m, n), rows in [(s, 4) for s in R.MUL_SHAPES] + [((32, 32), MANY)]:
        a, b = R.input_rows(200 + m, m + 1, rows), R.input_rows(300 + n, n + 1, rows)
        ref = R.mul(a, b)
        ab, ba = ctx.bern_mul(a, b), ctx.bern_mul(b, a)
        sh.hold(ab, ref, "(%d, %d) x %d capi" % (m, n, rows))
        sh.hold(ba, ref, "(%d, %d) x %d capi, operands swapped" % (m, n, rows))
        sh.hold(curve(bez, a).mul(curve(bez, b)).cpts, ref, "(%d, %d) x %d Bezier" % (m, n, rows))
        sh.n += 1
        if not R.pair_within(ab, ba, ref):                       # mul(a, b) == mul(b, a) within the two bounds
            sh.failed.append("mul (%d, %d): mul(a, b) and mul(b, a) differ by more than 2 K * 2^-53 * M" % (m, n))
    sh.done()


def test_normsq(ctx, bez):
    sh = Shares("normsq")                                         # (obtg_bern_normsq takes one curve, d rows, per call)
    for d, n in R.NORMSQ_SHAPES:
        for kind in range(4):
            x = R.input_rows(400 + 10 * n + kind, n + 1, 4 * d)[kind::4]      # d rows of one kind
            ref = R.normsq(x)
            sh.hold(ctx.bern_normsq(x), ref, "(%d, %d) kind %d capi" % (d, n, kind))
            sh.hold(curve(bez, x).normSquare().cpts, ref, "(%d, %d) kind %d Bezier" % (d, n, kind))
        x = R.input_rows(450 + n, n + 1, max(d, 4))[:d]                       # rows of different kinds in one curve
        sh.hold(ctx.bern_normsq(x), R.normsq(x), "(%d, %d) mixed kinds capi" % (d, n))
    sh.done()


def test_diff(ctx, bez):
    sh = Shares("diff")
    for n, rows in [(n, 4) for n in R.DIFF_DEGREES] + [(65, MANY)]:
        a = R.input_rows(500 + n, n + 1, rows)
        for T in R.DIFF_T:
            ref = R.diff(a, T)
            sh.hold(ctx.bern_diff(a, T), ref, "n = %d, T = %r x %d capi" % (n, T, rows))
            sh.hold(curve(bez, a, 0.0, T).diff().cpts, ref, "n = %d, T = %r x %d Bezier" % (n, T, rows))
    sh.done()


def test_split(ctx, bez):
    sh = Shares("split")
    for n, rows in [(n, 4) for n in R.SPLIT_DEGREES] + [(64, MANY)]:
        many = rows == MANY
        a = R.input_rows(600 + n, n + 1, rows)
        for z in ([0.3] if many else R.split_z(n)):
            rl, rr = R.split(a, z)
            left, right = ctx.bern_split(a, z)
            sh.hold(left, rl, "n = %d, z = %r x %d left capi" % (n, z, rows))
            sh.hold(right, rr, "n = %d, z = %r x %d right capi" % (n, z, rows))
            c1, c2 = curve(bez, a).split(z)                                   # span [0, 1]: z is tDiv
            sh.hold(c1.cpts, rl, "n = %d, z = %r left Bezier" % (n, z))
            sh.hold(c2.cpts, rr, "n = %d, z = %r right Bezier" % (n, z))
            sh.same([c1.t0, c1.tf, c2.t0, c2.tf], [0.0, z, z, 1.0], "n = %d, z = %r spans of the pieces" % (n, z))
            if z == 0.0:
                sh.same(left, np.repeat(a[:, :1], n + 1, axis=1), "n = %d, z = 0 left" % n)
                sh.same(right, a, "n = %d, z = 0 right" % n)
            if z == 1.0:
                sh.same(left, a, "n = %d, z = 1 left" % n)
                sh.same(right, np.repeat(a[:, -1:], n + 1, axis=1), "n = %d, z = 1 right" % n)
    # a span of its own: Bezier.split forms z = (tDiv - t0) / (tf - t0) and keeps [t0, tDiv], [tDiv, tf]
    a = R.input_rows(690, 66)
    t0, tf, tdiv = 2.5, 9.75, 4.1
    c1, c2 = curve(bez, a, t0, tf).split(tdiv)
    rl, rr = R.split(a, (tdiv - t0) / (tf - t0))
    sh.hold(c1.cpts, rl, "span (2.5, 9.75) left Bezier")
    sh.hold(c2.cpts, rr, "span (2.5, 9.75) right Bezier")
    sh.same([c1.t0, c1.tf, c2.t0, c2.tf], [t0, tdiv, tdiv, tf], "span (2.5, 9.75) spans of the pieces")
    sh.done()


def test_eval(ctx, bez):
    sh = Shares("eval")
    for nc, rows in [(nc, 4) for nc in R.EVAL_NC] + [(65, MANY)]:
        many = rows == MANY
        a = R.input_rows(700 + nc, nc, rows)
        for n_tau in ([65] if many else R.EVAL_NTAU):
            for t0, tf in R.EVAL_SPANS:
                tau = R.eval_tau(n_tau, t0, tf)
                ref = R.eval_curve(a, tau, t0, tf)
                out = ctx.bern_eval(a, tau, t0, tf)
                sh.hold(out, ref, "nc = %d, %d samples on (%r, %r) x %d capi" % (nc, n_tau, t0, tf, rows))
                sh.hold(curve(bez, a, t0, tf)(tau), ref, "nc = %d, %d samples on (%r, %r) Bezier" % (nc, n_tau, t0, tf))
                if n_tau >= 2:                      # tau = t0 and tau = tf give the end control points exactly
                    sh.same(out[:, 0], a[:, 0], "nc = %d, tau = t0" % nc)
                    sh.same(out[:, -1], a[:, -1], "nc = %d, tau = tf" % nc)
    sh.done()


@pytest.mark.parametrize("nc", R.EVAL_NC)
def test_curve_all_1001_samples(bez, nc):
    """Bezier.curve on its default grid, every sample: odd and even nc (the LDS pitch nc | 1) up to the longest row
    obtg_bern_eval takes"""
    sh = Shares("eval (Bezier.curve, nc = %d)" % nc)
    t0, tf = R.EVAL_SPANS[nc % 2]
    a = R.input_rows(750 + nc, nc, 3)
    c = curve(bez, a, t0, tf)
    out = c.curve
    assert out.shape == (3, 1001) and np.array_equal(c.tau, np.linspace(t0, tf, 1001))
    sh.hold(out, R.eval_curve(a, c.tau, t0, tf), "on (%r, %r)" % (t0, tf))
    sh.same(out[:, 0], a[:, 0], "first sample")
    sh.same(out[:, -1], a[:, -1], "last sample")
    sh.done()


def test_eval_limit_is_125_control_points(ctx):
    """126 control points would need 66 032 bytes of LDS: the launcher answers OBTG_ERR_UNSUPPORTED without a launch and the
    context stays usable; 125 ask for 65 000 and work (test_eval, test_curve_all_1001_samples)"""
    from optimalbeziertrajectorygeneration_amd import _capi
    a = R.input_rows(760, 126)
    with pytest.raises(_capi.ObtgError) as e:
        ctx.bern_eval(a, [0.25, 0.5], 0.0, 1.0)
    assert e.value.code == _capi.ERR_UNSUPPORTED == -5
    b = a[:, :125]
    assert R.within(ctx.bern_eval(b, [0.25, 0.5], 0.0, 1.0), R.eval_curve(b, [0.25, 0.5], 0.0, 1.0))


def test_restrict(ctx):
    sh = Shares("restrict")
    for nc, rows in [(nc, 10) for nc in R.RESTRICT_NC] + [(65, MANY)]:
        a = R.input_rows(800 + nc, nc, rows)
        span, target = R.restrict_cases(rows)                    # one target per row: rows of one launch take different branches
        ref = R.restrict(a, span, target)
        out = ctx.bern_restrict(a, span, target)
        sh.hold(out, ref, "nc = %d x %d" % (nc, rows))
        sh.same(out[3::5], a[3::5], "nc = %d: rows that take no cut" % nc)
    sh.done()


def test_bezier_level_elevated_stack_and_alignment(bez):
    sh = Shares("Bezier level")
    curves = [R.input_rows(850 + k, k, 3) for k in (4, 11, 70)]
    out = bez.elevated_stack(curves)
    assert out.shape == (3, 3, 70)
    for i, c in enumerate(curves):
        sh.hold(out[i], R.elev(c, 70 - c.shape[1]), "elevated_stack, length %d" % c.shape[1])
    sh.same(out[2], curves[2], "elevated_stack, the longest curve")
    # _temporalAlignment: unequal degrees (a call per curve) and equal degrees (one call for both)
    for (n1, s1), (n2, s2) in (((5, (0.0, 4.0)), (8, (1.0, 6.0))), ((64, (0.5, 4.0)), (64, (0.0, 3.25))), ((6, (1.0, 2.0)), (6, (1.0, 5.0)))):
        c1, c2 = curve(bez, R.input_rows(860 + n1, n1 + 1, 2), *s1), curve(bez, R.input_rows(870 + n2, n2 + 1, 2), *s2)
        a1, a2 = bez._temporalAlignment(c1, c2)
        t0, tf = max(s1[0], s2[0]), min(s1[1], s2[1])
        for c, a, s in ((c1, a1, s1), (c2, a2, s2)):
            sh.hold(a.cpts, R.restrict(c.cpts, s, (t0, tf)), "_temporalAlignment degrees (%d, %d), span %r" % (n1, n2, s))
            sh.same([a.t0, a.tf], [t0, tf], "_temporalAlignment span")
    sh.done()


# ---------------------------------------------------------------------------------------------------------------------
#  the objectives: a Context per shape
# ---------------------------------------------------------------------------------------------------------------------
def test_euclidean_obj():
    from optimalbeziertrajectorygeneration_amd import _capi
    sh = Shares("euclidean_obj")
    for n_veh, dim, deg in R.EUCLID_SHAPES:
        Y = R.iterates(800 + n_veh, n_veh, dim, deg)
        c = _capi.Context(n_veh, dim, deg, 0)
        try:
            out = c.euclidean_obj(Y)
        finally:
            c.close()
        assert out.shape == (R.ENERGY_B,)
        for b in range(R.ENERGY_B):
            sh.hold(out[b:b + 1], R.euclidean_obj(Y[b], n_veh, dim), "(%d, %d, %d) iterate %d" % (n_veh, dim, deg, b))
    sh.done()


@pytest.mark.parametrize("order,name", [(2, "accel_obj"), (3, "jerk_obj")])
def test_deriv_energy_obj(order, name):
    from optimalbeziertrajectorygeneration_amd import _capi
    sh = Shares(name)
    forms = {}
    by_shape = {}
    for n_veh, dim, deg, Rr in R.ENERGY_SHAPES:
        by_shape.setdefault((n_veh, dim, deg), []).append(Rr)
    for (n_veh, dim, deg), Rs in by_shape.items():
        Y = R.iterates(900 + n_veh + deg, n_veh, dim, deg)
        # launch_deriv_energy_obj ends in launch_speed: a specialised kernel where the shape has one, else the any-degree one
        forms[(n_veh, dim, deg)] = "specialised" if _capi.fast_kernels(dim, deg) & 1 else "generic"
        c = _capi.Context(n_veh, dim, deg, 0)
        try:
            for Rr in Rs:
                c.set_deg_elev(Rr)
                for tf in R.ENERGY_TF:
                    out = c.deriv_energy_obj(Y, tf, order)
                    for b in range(R.ENERGY_B):
                        sh.hold(out[b:b + 1], R.deriv_energy_obj(Y[b], n_veh, dim, Rr, tf, order),
                                "(%d, %d, %d) R = %d, tf = %r, iterate %d" % (n_veh, dim, deg, Rr, tf, b))
        finally:
            c.close()
    print("\n%s: speed kernel form per (n_veh, dim, deg): %s" % (name, ", ".join("%r %s" % kv for kv in sorted(forms.items()))))
    assert set(forms.values()) == {"specialised", "generic"}
    sh.done()


def test_objective_function_of_the_problem_class():
    """BezOptimization(minimizeGoal=...).objectiveFunction against the same reference, on the Y its reshapeVector forms"""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    sh = Shares("objectiveFunction")
    try:
        for goal, Rr in (("Accel", 30), ("Jerk", 0), ("Euclidean", 0)):
            opt.DEG_ELEV = Rr                                    # read at call time
            bo = opt.BezOptimization(numVeh=3, dimension=2, degree=7, minimizeGoal=goal, initPoints=[(0, 0), (1, 5), (9, 2)],
                                     finalPoints=[(10, 1), (8, 8), (0, 7)], tf=7.0)
            x = bo.generateGuess(std=0.4, seed=11)
            Y = bo.reshapeVector(x)
            ref = (R.euclidean_obj(Y, 3, 2) if goal == "Euclidean" else
                   R.deriv_energy_obj(Y, 3, 2, Rr, 7.0, 2 if goal == "Accel" else 3))
            sh.hold([bo.objectiveFunction(x)], ref, "%s, DEG_ELEV = %d" % (goal, Rr))
    finally:
        opt.DEG_ELEV = 0
    sh.done()


# ---------------------------------------------------------------------------------------------------------------------
#  the longest rows the launchers accept: 1024 coefficients, entries in uniform(-1, 1)
# ---------------------------------------------------------------------------------------------------------------------
def _uniform(seed, rows, length):
    return np.random.default_rng(seed).uniform(-1, 1, (rows, length))


def test_longest_elev(ctx):
    sh = Shares("elev(511, 512)")
    a = _uniform(1, 3, 512)
    out = ctx.bern_elev(a, 512)
    assert np.isfinite(out).all()
    sh.hold(out, R.elev(a, 512), "1024 coefficients")
    sh.done()


def test_longest_mul(ctx):
    sh = Shares("mul(511, 512)")
    a, b = _uniform(2, 3, 512), _uniform(3, 3, 513)
    out = ctx.bern_mul(a, b)
    assert np.isfinite(out).all()
    sh.hold(out, R.mul(a, b), "1024 coefficients")
    sh.done()


def test_longest_normsq(ctx):
    sh = Shares("normsq(d = 3, n = 511)")
    x = _uniform(4, 3, 512)
    out = ctx.bern_normsq(x)
    assert np.isfinite(out).all()
    sh.hold(out, R.normsq(x), "1023 coefficients")
    sh.done()


def test_1025_coefficients_are_refused(ctx):
    from optimalbeziertrajectorygeneration_amd import _capi
    calls = (("elev", lambda: ctx.bern_elev(_uniform(5, 3, 512), 513)),
             ("mul", lambda: ctx.bern_mul(_uniform(6, 3, 513), _uniform(7, 3, 513))),
             ("normsq", lambda: ctx.bern_normsq(_uniform(8, 3, 513))),
             ("diff", lambda: ctx.bern_diff(_uniform(9, 3, 1025), 1.0)),
             ("split", lambda: ctx.bern_split(_uniform(10, 3, 1025), 0.5)),
             ("restrict", lambda: ctx.bern_restrict(_uniform(11, 3, 1025), (0.0, 1.0), (0.25, 1.0))))
    for name, call in calls:
        with pytest.raises(_capi.ObtgError) as e:
            call()
        assert e.value.code == -5, name
    a = R.input_rows(12, 6)
    assert R.within(ctx.bern_elev(a, 7), R.elev(a, 7))           # the context is still usable
