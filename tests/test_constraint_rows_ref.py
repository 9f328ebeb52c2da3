"""Holds tests/constraint_rows_ref.py honest, on the CPU: (a) the CPU oracle passes the exact-rational bound at every shape
tests/test_gpu_constraint_rows.py uses, (b) so do the reference's own outputs in tests/golden (constraints.npz, problem.npz,
nearstop.npz with its exact_* arrays), (c) the yardstick agrees with the Fraction restatement of tests/exact_jacobian_ref.py,
(d) the bound rejects wrong answers -- each mutant misses by at least ten times the bound, and the one that moves an element
by 1e-10 of the row's scale PASSES the suite's older bar, assert_close(..., 1e-9) --, (e) the launch-form arithmetic restated
in constraint_rows_ref (sep_form, ang_form) says of every case what the case's table entry claims.
The largest shares of the bound are printed (pytest -s).

Measured here (x86-64, the gcc oracle; the reference's fixtures from NumPy / OpenBLAS), largest share of the bound:
    CPU oracle           separation 0.172   speed 0.098   angular rate (quotient test) 0.463
    reference fixtures   separation 0.179   speed 0.013   angular rate 0.017; nearstop.npz and its exact_* arrays below 0.001
                         (near-stop rows: the quotient test is loose by itself where D is small against MD)
"""
import math
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_rows_ref as C  # noqa: E402
import exact_jacobian_ref as E  # noqa: E402
from util import assert_close  # noqa: E402


class Shares(object):
    def __init__(self, title):
        self.title, self.worst = title, {}

    def hold(self, fam, cand, ref, what):
        fn = C.ang_assert_within if isinstance(ref, C.AngRef) else C.assert_within
        self.worst[fam] = max(self.worst.get(fam, 0.0), fn(cand, ref, "%s %s" % (fam, what)))

    def report(self):
        print("\n%s: largest share of the bound used" % self.title)
        for fam in sorted(self.worst):
            print("  %-28s %.3f" % (fam, self.worst[fam]))
        assert all(v <= 1.0 for v in self.worst.values())


# ------------------------------------------------------------------------------------------------ (a) the CPU oracle
def test_oracle_separation_at_every_device_shape(oracle):
    """(the oracle takes no point obstacles: the vehicles' pairs of a case with obstacles)"""
    sh = Shares("CPU oracle, separation")
    for name, N, d, n, R, M, kind, B, rng, form in C.SEP_CASES:
        Y = C.swarm(11, N, d, n, kind)
        pairs = C.all_pairs(N)
        sel = slice(None) if rng is None else slice(rng[0], rng[0] + rng[1])
        ref = C.temporal_sep(Y, N, d, R, C.SEP_MAX_SEP, None, pairs[sel])
        got = oracle.temporal_sep(Y, N, d, R, C.SEP_MAX_SEP).reshape(len(pairs), -1)[sel]
        sh.hold("generic shapes" if "generic" in form["kernel"] else ("R > 0" if R else "R = 0"), got, ref, name)
    sh.report()


def test_oracle_speed_at_every_device_shape(oracle):
    sh = Shares("CPU oracle, speed")
    for name, N, d, n, R, kind, form in C.SPEED_CASES:
        Y = C.swarm(12, N, d, n, kind)
        for tf in C.SPEED_TF:
            for is_max, bound in ((1, C.SPEED_BOUNDS[0]), (0, C.SPEED_BOUNDS[1])):
                ref = C.speed(Y, N, d, R, tf, bound, is_max)
                sh.hold("R > 0" if R else "R = 0", oracle.speed(Y, N, d, R, tf, bound, is_max).reshape(ref.shape), ref,
                        "%s tf %r is_max %d" % (name, tf, is_max))
    sh.report()


def _ang_inputs():
    for name, N, n, R, order, kind, form in C.ANG_CASES:
        yield name, N, n, R, order, C.swarm(13, N, 2, n, kind)
    for m in (6, 7, 127, 128):
        yield "any-degree m = %d" % m, 2, 6, m - 6, 0, C.swarm(14, 2, 2, 6, "full")


def test_oracle_angular_rate_at_every_device_shape(oracle):
    """The oracle elevates the position first (the reference's order): held to the counts of order 1"""
    sh = Shares("CPU oracle, angular rate (quotient test)")
    for name, N, n, R, order, Y in _ang_inputs():
        if 4 * (n + R) > 1000:
            continue                    # C(4 m, 2 m) of the oracle's product weights is not finite past m = 250
        for tf in C.ANG_TF[:2 if R > 50 else 3]:
            ref = C.ang_rate(Y, N, R, tf, 1.0, 1)
            sh.hold("R > 0" if R else "R = 0", oracle.ang_rate(Y, N, R, tf, 1.0).reshape(ref.shape), ref, "%s tf %r" % (name, tf))
    sh.report()


def test_oracle_batch_entry(oracle):
    B, N, d, n, R = 3, 5, 2, 10, 4
    Yb = C.rows_batch(15, B, N, d, n)
    tf = np.array(C.SPEED_TF)
    o_sep, o_sp, o_an = oracle.eval_batch(Yb, tf, N, d, R, C.SEP_MAX_SEP, 5.0, 1.0)
    sh = Shares("CPU oracle, eval_batch")
    for b in range(B):
        sh.hold("separation", o_sep[b].reshape(-1, 2 * n + R + 1), C.temporal_sep(Yb[b], N, d, R, C.SEP_MAX_SEP), b)
        sh.hold("speed", o_sp[b].reshape(N, -1), C.speed(Yb[b], N, d, R, tf[b], 5.0, 1), b)
        sh.hold("angular rate", o_an[b].reshape(N, -1), C.ang_rate(Yb[b], N, R, tf[b], 1.0, 1), b)
    sh.report()


# ------------------------------------------------------------------------------------------------ (b) the reference's fixtures
def test_reference_fixtures_pass_the_bound(golden_dir):
    sh = Shares("reference fixtures")
    c = np.load(os.path.join(golden_dir, "constraints.npz"))
    for name in c["names"]:
        name = str(name)
        N, dim, n, R, tf, ms, vmax, vmin, wmax = c[name + "_par"]
        N, dim, n, R = int(N), int(dim), int(n), int(R)
        Y = c[name + "_Y"]
        if N <= 40:                                       # (c3 is 2016 pairs of the same kernel arithmetic as c3s)
            sh.hold("separation", c[name + "_tsep"].reshape(-1, 2 * n + R + 1), C.temporal_sep(Y, N, dim, R, ms), name)
        sh.hold("speed", c[name + "_maxspeed"].reshape(N, -1), C.speed(Y, N, dim, R, tf, vmax, 1), name + " max")
        sh.hold("speed", c[name + "_minspeed"].reshape(N, -1), C.speed(Y, N, dim, R, tf, vmin, 0), name + " min")
        if name + "_angrate" in c.files:
            sh.hold("angular rate", c[name + "_angrate"].reshape(N, -1), C.ang_rate(Y, N, R, tf, wmax, 1), name)
    p = np.load(os.path.join(golden_dir, "problem.npz"))
    obs = [[3.0, 2.0], [6.0, 7.0]]
    for R in (0, 30, 100):
        for tag in ("g", "r"):
            x, y = (p["ex1_xguess"], p["ex1_yguess"]) if tag == "g" else (p["ex1_x"], p["ex1_y"])
            pre = "ex1_%s_" % tag
            sh.hold("separation", p[pre + "tsep_class_R%d" % R].reshape(6, -1), C.temporal_sep(y, 2, 2, R, 1.0, obs), pre + "class")
            sh.hold("separation", p[pre + "tsep_example_R%d" % R].reshape(1, -1), C.temporal_sep(y, 2, 2, R, 1.0), pre + "example")
            sh.hold("speed", p[pre + "maxspeed_R%d" % R].reshape(2, -1), C.speed(y, 2, 2, R, x[-1], 5.0, 1), pre + "max")
            sh.hold("speed", p[pre + "minspeed_R%d" % R].reshape(2, -1), C.speed(y, 2, 2, R, x[-1], 0.0, 0), pre + "min")
            if R <= 30:
                sh.hold("angular rate", p[pre + "angrate_R%d" % R].reshape(2, -1), C.ang_rate(y, 2, R, x[-1], 1.0, 1), pre + "ang")
    sh.hold("separation", p["sw_r_tsep"].reshape(630, -1), C.temporal_sep(p["sw_y"], 36, 3, 0, 0.9), "swarm")
    sh.hold("separation", p["fx_tsep"].reshape(3, -1), C.temporal_sep(p["fx_y"], 3, 2, 0, 0.5), "fx")
    sh.hold("angular rate", p["fx_angrate"].reshape(3, -1), C.ang_rate(p["fx_y"], 3, 0, 7.0, 2.0, 1), "fx")
    g = np.load(os.path.join(golden_dir, "nearstop.npz"))
    N, n, R = int(g["par"][0]), int(g["par"][2]), int(g["par"][3])
    for tf in g["tfs"]:
        ref = C.ang_rate(g["Y"], N, R, float(tf), 1.0, 1)
        sh.hold("angular rate, nearstop.npz", g["angrate_tf%g" % tf].reshape(ref.shape), ref, "tf %g" % tf)
        sh.hold("nearstop.npz exact_*", g["exact_tf%g" % tf].reshape(ref.shape), ref, "exact, tf %g" % tf)
        sh.hold("speed", g["maxspeed_tf%g" % tf].reshape(N, -1), C.speed(g["Y"], N, 2, R, float(tf), 5.0, 1), "nearstop")
    sh.report()


# ------------------------------------------------------------------------------------------------ (c) against the Fraction restatement
def test_agrees_with_the_fraction_restatement():
    N, d, n, R = 4, 3, 4, 3
    Y = C.swarm(21, N, d, n, "edges")
    obs = C.point_obstacles(22, 2, d)
    ref = C.temporal_sep(Y, N, d, R, 0.5, obs)           # (bounds whose squares are exact: E squares the bound in exact arithmetic)
    assert [ref.value(i) for i in range(len(ref.num))] == E.temporal_sep(Y, N, d, R, 0.5, obs)
    for is_max in (0, 1):
        ref = C.speed(Y, N, d, R, 0.013, 5.0, is_max)
        assert [ref.value(i) for i in range(len(ref.num))] == E.speed(Y, N, d, R, 0.013, 5.0, is_max)
    Y2 = C.swarm(23, 3, 2, 5)
    Y2[2:4] = [[3.25], [-1.5]]                                        # a vehicle at rest: 0 / 0
    ref = C.ang_rate(Y2, 3, 2, 7.3, 1.5)
    assert [ref.value(i) for i in range(len(ref.N))] == E.ang_rate(Y2, 3, 2, 7.3, 1.5)
    assert all(ref.N[i] == 0 == ref.D[i] for i in range(ref.shape[1], 2 * ref.shape[1]))
    # the majorant dominates the value, the bound is positive wherever the value is not an exact zero of zeros
    s = C.temporal_sep(Y, N, d, R, 0.9, obs)
    assert all(s.majorant(i) >= abs(s.value(i)) for i in range(len(s.num)))


def test_quotient_test_on_zero_denominators():
    Y = C.swarm(24, 3, 2, 5)
    Y[2:4] = [[3.25], [-1.5]]
    ref = C.ang_rate(Y, 3, 0, 2.0, 1.0)
    good = ref.nearest()
    assert np.isnan(good[1]).all() and C.ang_within(good, ref)
    bad = good.copy()
    bad[1, 3] = 0.0                                                   # a finite value where 0 / 0 must be NaN
    assert not C.ang_within(bad, ref)
    bad = good.copy()
    bad[0, 2] = math.inf
    assert not C.ang_within(bad, ref)
    # D = 0 != N: a straight line at constant speed zero only in y, x'' != 0 cannot be: use N, D by hand
    r = C.AngRef([5, -5, 0], [0, 0, 0], [5, 5, 0], [0, 0, 0], 10, 10, 1.0, (1, 3))
    assert C.ang_within(np.array([[-math.inf, math.inf, math.nan]]), r)
    assert not C.ang_within(np.array([[math.inf, math.inf, math.nan]]), r)
    assert not C.ang_within(np.array([[-math.inf, math.inf, 0.0]]), r)


def test_diff_majorant_is_the_sum_of_magnitudes(oracle, golden_dir):
    """Why the speed rows' derivative takes (n/T)(|P_i| + |P_(i+1)|) and not (n/T)|P_(i+1) - P_i|: Bezier.diff() is a matrix
    product, each of its two products rounded at the size of the position.  On a swarm offset by 1e6 the oracle misses the
    difference-majorant's bound by three to four orders of magnitude, and so does the plain NumPy statement of the reference's
    own line (cpts.dot(diffMatrix), bezier.py:514) -- the count was wrong, not the arithmetic."""
    N, d, n, R, tf = 4, 3, 5, 7, 0.013
    Y = C.swarm(1, N, d, n, "offset")
    got = oracle.speed(Y, N, d, R, tf, 5.0, 1).reshape(N, -1)
    tight = C.speed(Y, N, d, R, tf, 5.0, 1, "difference")
    s_or = float(C.shares(got, tight)[0].max())
    # the reference's own statement: derivative by the matrix product, elev(1), normSquare, elev(R), in float64
    Dm = np.zeros((n + 1, n))
    for i in range(n):
        Dm[i, i], Dm[i + 1, i] = -n / tf, n / tf
    rows = []
    for v in range(N):
        dv = [[F(float(x)) for x in (Y[v * d + q] @ Dm)] for q in range(d)]
        c = E.elev(E.normsq([E.elev(r, 1) for r in dv]), R)           # (everything after the matrix product exact)
        rows.append([float(F(5.0) ** 2 - x) for x in c])
    s_np = float(C.shares(np.array(rows), tight)[0].max())
    print("\nspeed rows of a swarm offset by 1e6 against the |P_(i+1) - P_i| majorant: oracle %.3g, cpts.dot(diffMatrix) %.3g times the bound"
          % (s_or, s_np))
    assert s_or > 100 and s_np > 100
    assert C.within(got, C.speed(Y, N, d, R, tf, 5.0, 1)) and C.within(np.array(rows), C.speed(Y, N, d, R, tf, 5.0, 1))
    # the separation's first difference IS one subtraction: the same swarm passes with |v_i - v_j|
    assert C.within(oracle.temporal_sep(Y, N, d, R, 0.75).reshape(6, -1), C.temporal_sep(Y, N, d, R, 0.75))


# ------------------------------------------------------------------------------------------------ (d) mutants
def _w(n, k, j):
    return F(math.comb(n, j) * math.comb(n, k - j), math.comb(2 * n, k))


def _product(dv, n, d, half=True, weight_bump=None, drop_last=False):
    out = []
    for k in range(2 * n + 1):
        js = list(range(max(0, k - n), min(n, k) + 1))
        if drop_last:
            js = js[:-1] if len(js) > 1 else js
        s = F(0)
        for j in js:
            w = _w(n, k, j)
            if weight_bump == (k, j):
                w *= 1 + F(1, 10 ** 12)
            s += w * sum(r[j] * r[k - j] for r in dv)
        out.append(s * (F(d, 2) if half else 1))
    return out


def _elev_moved(c, R, move):
    """elevation by the matrix, entry `move` = (j, k) added into column k + 1 instead of k"""
    N = len(c) - 1
    out = [F(0)] * (N + R + 1)
    for k in range(N + R + 1):
        for j in range(max(0, k - R), min(N, k) + 1):
            out[k + 1 if (j, k) == move else k] += F(math.comb(N, j) * math.comb(R, k - j), math.comb(N + R, k)) * c[j]
    return out


def test_mutants_miss_by_ten_bounds():
    N, d, n, R, ms, tf, bound = 3, 3, 10, 5, 0.9, 7.3, 5.0
    Y = C.swarm(31, N, d, n)
    nc = n + 1
    ref = C.temporal_sep(Y, N, d, R, ms)
    L = 2 * n + R + 1
    ms2 = F(C.square(ms))
    cur = [[E.fr(Y[v * d + q]) for q in range(d)] for v in range(N)]
    pairs = C.all_pairs(N)
    dvs = [[E.add(cur[a][q], cur[b][q], -1) for q in range(d)] for a, b in pairs]

    def rows(fn):
        return np.array([[float(x) for x in fn(dv)] for dv in dvs])

    def worst(cand, r=ref):
        return float(C.shares(cand, r)[0].max())
    right = rows(lambda dv: [x - ms2 for x in E.elev(_product(dv, n, d), R)])
    assert np.array_equal(right, ref.nearest()) and worst(right) <= 0.5
    report = {}
    # one folded weight off by 1e-12 relative: the middle coefficient's largest term
    k = n
    j = max(range(0, n + 1), key=lambda t: abs(sum(r[t] * r[k - t] for r in dvs[0])))
    report["one weight off by 1e-12"] = worst(rows(lambda dv: [x - ms2 for x in E.elev(_product(dv, n, d, weight_bump=(k, j)), R)]))
    report["(d/2) dropped"] = worst(rows(lambda dv: [x - ms2 for x in E.elev(_product(dv, n, d, half=False), R)]))
    report["an elevation entry one column on"] = worst(rows(lambda dv: [x - ms2 for x in _elev_moved(_product(dv, n, d), R, (n, n + 2))]))
    report["last product term dropped"] = worst(rows(lambda dv: [x - ms2 for x in E.elev(_product(dv, n, d, drop_last=True), R)]))
    report["R off by one"] = worst(C.temporal_sep(Y, N, d, R + 1, ms).nearest()[:, :L])
    # speed: diff()'s elev(1) omitted (the derivative's n coefficients taken for n + 1 with a zero behind them); sign and offset swapped
    sref = C.speed(Y, N, d, R, tf, bound, 1)
    b2, T = F(C.square(bound)), F(tf)
    sp_right, sp_noelev, sp_swap = [], [], []
    for v in range(N):
        der = [[F(n) / T * (x[i + 1] - x[i]) for i in range(n)] for x in cur[v]]
        sp_right.append([float(b2 - x) for x in E.elev(_product([E.elev(r, 1) for r in der], n, d), R)])
        sp_noelev.append([float(b2 - x) for x in E.elev(_product([r + [F(0)] for r in der], n, d), R)])
        sp_swap.append([float(b2 * x + (-1)) for x in E.elev(_product([E.elev(r, 1) for r in der], n, d), R)])
    assert np.array_equal(np.array(sp_right), sref.nearest())
    report["diff's elev(1) omitted"] = worst(np.array(sp_noelev), sref)
    report["sign and offset swapped"] = worst(np.array(sp_swap), sref)
    # one element moved by 1e-10 of the row's scale: passes the older bar, misses this one
    moved = ref.nearest().copy()
    moved[1, 7] += 1e-10 * np.abs(moved[1]).max()
    assert_close(moved, ref.nearest(), 1e-9, "the 1e-10 mutant against the 1e-9 bar")
    assert_close(moved, right, 1e-9)
    report["one element moved by 1e-10 of the row's scale"] = worst(moved)
    # the angular rate's quotient test: the same displacement, and a numerator weight off by 1e-12
    aref = C.ang_rate(Y[:4], 2, R, tf, 1.0) if d == 2 else C.ang_rate(C.swarm(32, 2, 2, n), 2, R, tf, 1.0)
    good = aref.nearest()
    assert C.ang_within(good, aref)
    by_element = []
    for k in range(aref.shape[1]):
        am = good.copy()
        am[0, k] += 1e-10 * np.abs(am[0]).max()
        assert_close(am, good, 1e-9)
        by_element.append(float(C.ang_shares(am, aref)[0].max()))
    print("\nangular rate, one element moved by 1e-10 of the row's scale: bounds missed by, over the row's elements: "
          "largest %.3g, median %.3g, smallest %.3g" % (max(by_element), float(np.median(by_element)), min(by_element)))
    report["angular rate: the element moved by 1e-10 where the quotient is best conditioned"] = max(by_element)
    print("\nmutants, in bounds missed by:")
    for kname, v in report.items():
        print("  %-48s %.3g" % (kname, v))
    assert all(v >= 10.0 for v in report.values()), report


# ------------------------------------------------------------------------------------------------ (e) the launch forms
def test_case_tables_name_the_form_the_planner_takes():
    for name, N, d, n, R, M, kind, B, rng, want in C.SEP_CASES:
        f = C.sep_form(N + M, d, n, R, B, *(rng or (0, None)))
        assert all(f[k] == v for k, v in want.items()), (name, f, want)
    kernels = {C.sep_form(c[1] + c[5], c[2], c[3], c[4], c[7], *(c[8] or (0, None)))["kernel"] for c in C.SEP_CASES}
    assert kernels == {"k_normsq_elev", "k_normsq_elev<ELEV>", "k_sep_elev_coop", "k_generic_normsq_elev"}
    forms = {(f["staging"], f["tile_rows"]) for f in (C.sep_form(c[1] + c[5], c[2], c[3], c[4], c[7], *(c[8] or (0, None)))
                                                     for c in C.SEP_CASES if c[4] == 0 and "generic" not in c[9]["kernel"])}
    assert {("whole", 64), ("whole", 32), ("whole", 16), ("slots", 64), ("tiled", 64)} <= forms
    assert {C.speed_form(c[2], c[3], c[4]) for c in C.SPEED_CASES} == {"fast", "fast elevated", "generic"}
    for name, N, n, R, order, kind, form in C.ANG_CASES:
        assert C.ang_form(n, R, order) == form, name
    # k_generic_angrate's two schedule switches always agree: both count floor(m / 2) + 1 tiles, and 2 m + 1 <= 256 is the same
    # m <= 127 as 64 tiles -- so two of the four (balanced, balanced2) combinations exist, and m = 6, 7, 127 | 2, 128, 250 reach them
    assert all(C.angrate_balanced(m) == C.angrate_balanced2(m) for m in range(1, 251))
    assert C.ANG_GENERIC_M == {(True, True): 6, (False, False): 2, (True, False): None, (False, True): None}
    assert [C.angrate_balanced(m) for m in (6, 7, 127, 128, 250)] == [True, True, True, False, False]


def test_finiteness_condition_of_the_generic_rows():
    """include/obtg.h: the any-degree rows are finite while C(2n + R, k) times the majorant of the elevated product stays
    below DBL_MAX for every k.  The longest row (n = 2, R = 1019, 1024 coefficients) scaled to sit just inside."""
    Y, peak = C.longest_row_case()
    assert C.DBL_MAX / 8 <= peak < C.DBL_MAX / 2
    lim = float(np.abs(Y[0:2] - Y[2:4]).max())
    print("\nlongest generic row just inside the finiteness condition: largest |v_i - v_j| coordinate %.3f" % lim)
    assert 1.0 < lim < 100.0
    # the any-degree angular rate at m = 250: tf = 0.013 is outside its condition, a tf of a few units just inside
    Y = C.swarm(950, 2, 2, 6)
    assert C.ang_rate(Y, 2, 244, 0.013, 1.0).peak > C.DBL_MAX
    tf = C.ang_tf_inside(Y, 2, 244, 7.3)
    print("any-degree angular rate, m = 250, positions within +-10: just inside its finiteness condition at tf = %r" % tf)
    assert 0.5 < tf < 64.0
