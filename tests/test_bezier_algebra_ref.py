"""Holds tests/bezier_algebra_ref.py honest, on the CPU: (a) what the reference itself recorded (tests/golden/bezier_ops.npz,
aligned.npz) passes the exact-rational bound, (b) so does the CPU oracle at every shape the device tests use, and (c) the bound
rejects wrong answers -- each mutant built to miss by at least ten times its bound, which the test asserts of its own inputs.
The shares of the bound that (a) and (b) use are printed (pytest -s)."""
import math
import os
import sys
from collections import defaultdict
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bezier_algebra_ref as R  # noqa: E402


class Shares(object):
    def __init__(self, title):
        self.title, self.worst = title, defaultdict(float)

    def hold(self, op, cand, ref, what):
        self.worst[op] = max(self.worst[op], R.assert_within(cand, ref, "%s %s" % (op, what)))

    def report(self):
        print("\n%s: largest share of the bound K * 2^-53 * M used" % self.title)
        for op in sorted(self.worst):
            print("  %-14s %.3f" % (op, self.worst[op]))


# ------------------------------------------------------------------------------------------------ (a) the reference's fixtures
def test_reference_fixtures_pass_the_bound(golden_dir):
    o = np.load(os.path.join(golden_dir, "bezier_ops.npz"))
    sh = Shares("reference fixtures")
    for c in range(int(o["n_cases"])):
        pre = "c%d_" % c
        a, b, tf = o[pre + "a"], o[pre + "b"], float(o[pre + "tf"])
        sh.hold("elev", o[pre + "elev1"], R.elev(a, 1), pre + "elev1")
        sh.hold("elev", o[pre + "elev7"], R.elev(a, 7), pre + "elev7")
        sh.hold("diff", o[pre + "diff"], R.diff(a, tf), pre + "diff")
        sh.hold("diff", o[pre + "diff2"], R.diff(o[pre + "diff"], tf), pre + "diff2")     # (of its own float64 derivative)
        sh.hold("mul", o[pre + "mul"], R.mul(a, b), pre + "mul")
        sh.hold("normsq", o[pre + "normsq"], R.normsq(a), pre + "normsq")
        for q in range(3):
            left, right = R.split(a, float(o[pre + "split%d_t" % q]) / tf)
            sh.hold("split", o[pre + "split%d_l" % q], left, pre + "split%d left" % q)
            sh.hold("split", o[pre + "split%d_r" % q], right, pre + "split%d right" % q)
        sh.hold("call", o[pre + "call_v"], R.eval_curve(a, o[pre + "call_t"], 0.0, tf), pre + "call_v")
        grid = np.linspace(0.0, tf, 1001)
        sh.hold("curve", o[pre + "curve_head"], R.eval_curve(a, grid[:3], 0.0, tf), pre + "curve_head")
        sh.hold("curve", o[pre + "curve_tail"], R.eval_curve(a, grid[-3:], 0.0, tf), pre + "curve_tail")
    fx = np.load(os.path.join(golden_dir, "aligned.npz"))
    for g in fx["groups"]:
        g = str(g)
        over = ~fx[g + "_none"]
        ends = fx[g + "_ends"][over]
        for c, s, a in (("_c1", "_s1", "_a1"), ("_c2", "_s2", "_a2")):
            cp, sp, al = fx[g + c][over], fx[g + s][over], fx[g + a][over]
            dim, nc = cp.shape[1:]
            ref = R.restrict(cp.reshape(-1, nc), np.repeat(sp, dim, axis=0), np.repeat(ends, dim, axis=0))
            sh.hold("restrict", al.reshape(-1, nc), ref, g + a)
    sh.report()


# ------------------------------------------------------------------------------------------------ (b) the CPU oracle
def test_oracle_passes_the_bound_at_every_device_shape(oracle):
    O = oracle
    sh = Shares("CPU oracle")
    for n, Rr in R.ELEV_SHAPES:
        a = R.input_rows(100 + n + Rr, n + 1)
        sh.hold("elev", O.elev(a, Rr), R.elev(a, Rr), (n, Rr))
    for m, n in R.MUL_SHAPES:
        a, b = R.input_rows(200 + m, m + 1), R.input_rows(300 + n, n + 1)
        sh.hold("mul", O.mul(a, b), R.mul(a, b), (m, n))
    for d, n in R.NORMSQ_SHAPES:
        for r in range(4):
            x = R.input_rows(400 + 10 * n + r, n + 1, 4 * d)[r::4]          # d rows of kind r
            sh.hold("normsq", O.normsq(x), R.normsq(x), (d, n, r))
    for n in R.DIFF_DEGREES:
        a = R.input_rows(500 + n, n + 1)
        for T in R.DIFF_T:
            sh.hold("diff", O.diff(a, T), R.diff(a, T), (n, T))
    for n in R.SPLIT_DEGREES:
        a = R.input_rows(600 + n, n + 1)
        for z in R.split_z(n):
            left, right = O.split(a, z)
            rl, rr = R.split(a, z)
            sh.hold("split", left, rl, (n, z, "left"))
            sh.hold("split", right, rr, (n, z, "right"))
    for nc in R.EVAL_NC:
        a = R.input_rows(700 + nc, nc)
        for n_tau in R.EVAL_NTAU:
            for t0, tf in R.EVAL_SPANS:
                tau = R.eval_tau(n_tau, t0, tf)
                sh.hold("eval", O.curve_eval(a, tau, t0, tf), R.eval_curve(a, tau, t0, tf), (nc, n_tau, t0, tf))
    for n_veh, dim, deg in R.EUCLID_SHAPES:
        for b, Y in enumerate(R.iterates(800 + n_veh, n_veh, dim, deg)):
            sh.hold("euclidean_obj", [O.euclidean_obj(Y, n_veh, dim)], R.euclidean_obj(Y, n_veh, dim), (n_veh, dim, deg, b))
    for n_veh, dim, deg, Rr in R.ENERGY_SHAPES:
        for tf in R.ENERGY_TF:
            for b, Y in enumerate(R.iterates(900 + n_veh + deg, n_veh, dim, deg)):
                sh.hold("accel_obj", [O.accel_obj(Y, n_veh, dim, Rr, tf)], R.deriv_energy_obj(Y, n_veh, dim, Rr, tf, 2),
                        (n_veh, dim, deg, Rr, tf, b))
    sh.report()


def test_restrict_reference_is_its_own_two_splits():
    """restrict() against split(): a head cut is the right piece at zh, a tail cut the left piece at zt, and a row that takes
    no cut is the input with K = 0 (equality demanded)"""
    a = R.input_rows(11, 9, 5)
    span, target = R.restrict_cases(5)
    ref = R.restrict(a, span, target)
    nc = a.shape[1]
    head, zh, tail, zt = R.span_cut(span[0], target[0])
    assert head and not tail
    r0 = R.split(a[0], zh)[1]
    assert all(ref.value(j) == r0.value(j) and ref.K[j] == r0.K[j] for j in range(nc))
    head, zh, tail, zt = R.span_cut(span[1], target[1])
    assert tail and not head
    r1 = R.split(a[1], zt)[0]
    assert all(ref.value(nc + j) == r1.value(j) and ref.K[nc + j] == r1.K[j] for j in range(nc))
    assert R.span_cut(span[2], target[2])[0] and R.span_cut(span[2], target[2])[2]
    assert all(ref.value(3 * nc + j) == Fraction(float(a[3, j])) and ref.K[3 * nc + j] == 0 for j in range(nc))
    assert R.within(np.where(np.arange(5)[:, None] == 3, a, ref.nearest()), ref)
    bad = ref.nearest()
    bad[3, 4] = np.nextafter(a[3, 4], np.inf)
    assert not R.within(bad, ref)


# ------------------------------------------------------------------------------------------------ (c) wrong answers are rejected
def reject(mutant, ref, what):
    """the mutant misses by at least ten times its bound (a condition on the inputs, asserted), hence fails it"""
    s = R.share(mutant, ref)
    assert s >= 10.0, "%s: the mutant misses by only %.3g times its bound -- choose other inputs" % (what, s)
    assert not R.within(mutant, ref), what
    return s


def _binom(n):
    return np.array([math.comb(n, k) for k in range(n + 1)], dtype=np.float64)


def test_mutants_are_rejected(oracle):
    O = oracle
    rows = R.input_rows(21, 64)                                   # n = 63
    n, Rr = 63, 40
    ref = R.elev(rows, Rr)
    good = O.elev(rows, Rr)
    assert R.within(good, ref)
    bn, bR, bo = _binom(n), _binom(Rr), _binom(n + Rr)

    # one term dropped from one coefficient's sum
    m = good.copy()
    k, j = 50, 30
    m[2, k] -= rows[2, j] * bn[j] * bR[k - j] / bo[k]
    reject(m, ref, "elev: one term dropped")

    # the divisor taken from the binomial row of n + R - 1
    m = good.copy()
    m[:, :-1] = good[:, :-1] * bo[:-1] / _binom(n + Rr - 1)
    reject(m, ref, "elev: divisor from the row of n + R - 1")

    # coefficient 64 computed from the input row shifted by one
    m = good.copy()
    shifted = np.concatenate([rows[:, 1:], np.zeros((4, 1))], axis=1)
    m[:, 64] = O.elev(shifted, Rr)[:, 64]
    reject(m, ref, "elev: coefficient 64 from the shifted row")
    for r in range(4):                                            # every kind of row on its own, the mixed-magnitude one too
        one = good.copy()
        one[r, 64] = m[r, 64]
        reject(one, ref, "elev: coefficient 64 from the shifted row, row %d" % r)

    # the same three on a product of different degrees
    a, b = R.input_rows(22, 41), R.input_rows(23, 24)
    refm = R.mul(a, b)
    goodm = O.mul(a, b)
    assert R.within(goodm, refm)
    m = goodm.copy()
    m[2, 30] -= a[2, 20] * b[2, 10] * math.comb(40, 20) * math.comb(23, 10) / math.comb(63, 30)
    reject(m, refm, "mul: one term dropped")
    m = goodm.copy()
    m[:, :-1] = goodm[:, :-1] * _binom(63)[:-1] / _binom(62)
    reject(m, refm, "mul: divisor from the row of m + n - 1")

    # w rounded to float32 (split), t rounded to float32 (eval)
    z = 0.3
    refl, refr = R.split(rows, z)
    left, right = O.split(rows, z)
    assert R.within(left, refl) and R.within(right, refr)
    w32 = float(np.float32(1.0 - z))
    cur = rows.copy()
    ml, mr = np.empty_like(rows), np.empty_like(rows)
    for lev in range(n + 1):
        ml[:, lev], mr[:, n - lev] = cur[:, 0], cur[:, -1]
        cur = w32 * cur[:, :-1] + z * cur[:, 1:]
    reject(ml, refl, "split: w in float32, left")
    reject(mr, refr, "split: w in float32, right")
    tau = 2.5 + 7.25 * np.array([0.1, 0.37, 0.77])                # (parameters float32 does not hold)
    refe = R.eval_curve(rows, tau, 2.5, 9.75)
    assert R.within(O.curve_eval(rows, tau, 2.5, 9.75), refe)
    t32 = R.eval_t(tau, 2.5, 9.75).astype(np.float32).astype(np.float64)
    reject(O.curve_eval(rows, t32, 0.0, 1.0), refe, "eval: t in float32")

    # one vehicle's last segment left out of the Euclidean sum
    n_veh, dim, deg = 7, 2, 9
    Y = R.iterates(24, n_veh, dim, deg)[0]
    refu = R.euclidean_obj(Y, n_veh, dim)
    assert R.within([O.euclidean_obj(Y, n_veh, dim)], refu)
    P = Y.reshape(n_veh, dim, deg + 1)
    seg = np.sqrt((np.diff(P, axis=2) ** 2).sum(axis=1))          # [n_veh][deg]
    reject([seg.sum() - seg[4, -1]], refu, "euclidean: one last segment left out")

    # elev skipped before the control-point sum when R > 0
    n_veh, dim, deg, Re, tf = 3, 2, 7, 30, 7.0
    Y = R.iterates(25, n_veh, dim, deg)[0]
    refa = R.deriv_energy_obj(Y, n_veh, dim, Re, tf, 2)
    assert R.within([O.accel_obj(Y, n_veh, dim, Re, tf)], refa)
    reject([O.accel_obj(Y, n_veh, dim, 0, tf)], refa, "accel: elev skipped before the sum")
    # and a jerk that stops one derivative short
    reject([O.accel_obj(Y, n_veh, dim, Re, tf)], R.deriv_energy_obj(Y, n_veh, dim, Re, tf, 3), "jerk: one derivative short")


def test_a_derivative_order_above_the_degree_is_an_exact_zero_with_a_positive_majorant():
    for (n_veh, dim, deg, order) in ((1, 2, 2, 3), (1, 3, 1, 2), (1, 3, 1, 3)):
        Y = R.iterates(26, n_veh, dim, deg)[0]
        ref = R.deriv_energy_obj(Y, n_veh, dim, 0, 7.0, order)
        assert ref.value(0) == 0 and ref.majorant(0) > 0


def test_the_longest_rows_stay_finite_in_float64():
    """By Vandermonde the kernels' unnormalised sums at 1024 coefficients stay below max|a| C(1023, 511) ~ 2.2e306"""
    assert float(math.comb(1023, 511)) < 2.3e306 < sys.float_info.max
    assert 3 * float(math.comb(1022, 511)) < sys.float_info.max
