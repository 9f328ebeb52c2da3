"""Exact rational yardstick for the derivatives of the Bernstein constraint / cost families (fractions.Fraction throughout).

The families are restated from their definitions (optimization.py:311-539 of the reference: normSquare with its (d/2)
factor, diff = derivative then elev(1), elev, mul) and differentiated by stencils that are exact on them:
  - temporal separation, speed rows, accel / jerk objectives are quadratic in every control point: the central difference
    with unit step, (f(y + 1) - f(y - 1)) / 2, is their derivative exactly;
  - the angular rate's numerator (q^2, q linear along one coordinate) and denominator ((|v|^2)^2, quartic along one
    coordinate) have degree <= 4 along any one coordinate: the five-point stencil is exact, then the quotient rule;
  - tf enters the speed and angular-rate rows as tf^-2 (accel / jerk objectives as tf^(-2 order)): d/dtf = -2 f / tf.
Elevation is linear, so the stencils run on the unelevated polynomials and their results are elevated.  Float inputs are
converted exactly (Fraction(float)).  Test infrastructure only; shapes are small (a degree-10, R = 100 pair costs ~1 s).
"""
from fractions import Fraction as F
from functools import lru_cache
from math import comb


def fr(a):
    return [F(float(v)) for v in a]


@lru_cache(maxsize=None)
def _elev_cols(N, R):
    """per output k of the elevation N -> N + R: [(j, weight)]"""
    return tuple(tuple((j, F(comb(N, j) * comb(R, k - j), comb(N + R, k))) for j in range(max(0, k - R), min(N, k) + 1))
                 for k in range(N + R + 1))


def elev(c, R):
    if R == 0:
        return list(c)
    return [sum(w * c[j] for j, w in col) for col in _elev_cols(len(c) - 1, R)]


@lru_cache(maxsize=None)
def _mul_w(m, n):
    return tuple(tuple((j, F(comb(m, j) * comb(n, k - j), comb(m + n, k))) for j in range(max(0, k - n), min(m, k) + 1))
                 for k in range(m + n + 1))


def mul(a, b):
    m, n = len(a) - 1, len(b) - 1
    return [sum(w * a[j] * b[k - j] for j, w in col) for k, col in enumerate(_mul_w(m, n))]


def add(a, b, s=1):
    return [x + s * y for x, y in zip(a, b)]


def normsq(X):
    """bezier.py:869-889: (d/2) sum_c x_c * x_c (the reference's quirk kept)"""
    d = len(X)
    acc = None
    for x in X:
        p = mul(x, x)
        acc = p if acc is None else add(acc, p)
    return [F(d, 2) * v for v in acc]


def diff(x, T):
    """bezier.py:497-519: derivative (n / T) (x_{i+1} - x_i), then elev(1)"""
    n = len(x) - 1
    return elev([F(n) / T * (x[i + 1] - x[i]) for i in range(n)], 1)


def _curves(Y, nveh, dim, obs):
    """vehicles' curves (lists of Fractions per coordinate) then the point obstacles as constant curves"""
    nc = len(Y[0])
    cur = [[fr(Y[v * dim + c]) for c in range(dim)] for v in range(nveh)]
    for o in (obs if obs is not None else []):
        cur.append([[F(float(o[c]))] * nc for c in range(dim)])
    return cur


# ---------------------------------------------------------------------------------------------------- temporal separation
def temporal_sep(Y, nveh, dim, R, max_sep, obs=None):
    """rows of every pair (lexicographic), as obtg_temporal_sep"""
    cur = _curves(Y, nveh, dim, obs)
    out = []
    ms2 = F(float(max_sep)) ** 2
    for a in range(len(cur)):
        for b in range(a + 1, len(cur)):
            dv = [add(cur[a][c], cur[b][c], -1) for c in range(dim)]
            out += [v - ms2 for v in elev(normsq(dv), R)]
    return out


def temporal_sep_jac(Y, nveh, dim, R, obs=None):
    """[P][L][dim][nc]: d rows / d P_a by the unit central difference on P_a (pairs of two obstacles: zeros)"""
    cur = _curves(Y, nveh, dim, obs)
    nc = len(Y[0])
    out = []
    for a in range(len(cur)):
        for b in range(a + 1, len(cur)):
            dv = [add(cur[a][c], cur[b][c], -1) for c in range(dim)]
            L = 2 * (nc - 1) + R + 1
            blk = [[[F(0)] * nc for _ in range(dim)] for _ in range(L)]
            if a < nveh:
                for c in range(dim):
                    for i in range(nc):
                        fp, fm = [list(r) for r in dv], [list(r) for r in dv]
                        fp[c][i] += 1
                        fm[c][i] -= 1
                        g = elev([(p - m) / 2 for p, m in zip(normsq(fp), normsq(fm))], R)
                        for k in range(L):
                            blk[k][c][i] = g[k]
            out.append(blk)
    return out


# ---------------------------------------------------------------------------------------------------- speed
def _speed_raw(X, T):
    return normsq([diff(x, T) for x in X])


def speed(Y, nveh, dim, R, tf, bound, is_max):
    T, b2 = F(float(tf)), F(float(bound)) ** 2
    out = []
    for v in range(nveh):
        r = elev(_speed_raw([fr(Y[v * dim + c]) for c in range(dim)], T), R)
        out += [b2 - x if is_max else x - b2 for x in r]
    return out


def speed_jac(Y, nveh, dim, R, tf, is_max):
    """([N][L][dim][nc], [N][L]) with the sign of the bound applied"""
    T = F(float(tf))
    nc = len(Y[0])
    L = 2 * (nc - 1) + R + 1
    sg = -1 if is_max else 1
    J, Jt = [], []
    for v in range(nveh):
        X = [fr(Y[v * dim + c]) for c in range(dim)]
        blk = [[[F(0)] * nc for _ in range(dim)] for _ in range(L)]
        for c in range(dim):
            for i in range(nc):
                Xp, Xm = [list(r) for r in X], [list(r) for r in X]
                Xp[c][i] += 1
                Xm[c][i] -= 1
                g = elev([(p - m) / 2 for p, m in zip(_speed_raw(Xp, T), _speed_raw(Xm, T))], R)
                for k in range(L):
                    blk[k][c][i] = sg * g[k]
        J.append(blk)
        Jt.append([sg * (-2 * x / T) for x in elev(_speed_raw(X, T), R)])
    return J, Jt


# ---------------------------------------------------------------------------------------------------- angular rate
def _num_den(X, T):
    """numerator q^2 and denominator (|v|^2)^2 at degree 4n (optimization.py:578-611 before the elevation)"""
    d1 = [diff(x, T) for x in X]
    d2 = [diff(x, T) for x in d1]
    q = add(mul(d2[1], d1[0]), mul(d2[0], d1[1]), -1)
    s = add(mul(d1[0], d1[0]), mul(d1[1], d1[1]))
    return mul(q, q), mul(s, s)


def ang_rate(Y, nveh, R, tf, max_rate):
    """rows of obtg_ang_rate (None where the quotient has a zero denominator)"""
    T, m2 = F(float(tf)), F(float(max_rate)) ** 2
    out = []
    for v in range(nveh):
        num, den = _num_den([fr(Y[2 * v]), fr(Y[2 * v + 1])], T)
        num, den = elev(num, 4 * R), elev(den, 4 * R)
        out += [m2 - a / b if b != 0 else None for a, b in zip(num, den)]
    return out


def ang_rate_jac(Y, nveh, R, tf):
    """([N][La][2][nc], [N][La]): five-point stencil on num and den per control point, elevation, quotient rule.  Rows with
    a zero denominator: None."""
    T = F(float(tf))
    nc = len(Y[0])
    La = 4 * (nc - 1 + R) + 1
    J, Jt = [], []
    for v in range(nveh):
        X = [fr(Y[2 * v]), fr(Y[2 * v + 1])]
        num, den = _num_den(X, T)
        num, den = elev(num, 4 * R), elev(den, 4 * R)
        blk = [[[None] * nc for _ in range(2)] for _ in range(La)]
        for c in range(2):
            for i in range(nc):
                ev = {}
                for s in (-2, -1, 1, 2):
                    Xs = [list(r) for r in X]
                    Xs[c][i] += s
                    ev[s] = _num_den(Xs, T)
                dn = elev([(ev[-2][0][k] - 8 * ev[-1][0][k] + 8 * ev[1][0][k] - ev[2][0][k]) / 12 for k in range(len(ev[1][0]))], 4 * R)
                dd = elev([(ev[-2][1][k] - 8 * ev[-1][1][k] + 8 * ev[1][1][k] - ev[2][1][k]) / 12 for k in range(len(ev[1][1]))], 4 * R)
                for k in range(La):
                    if den[k] != 0:
                        blk[k][c][i] = -(dn[k] * den[k] - num[k] * dd[k]) / den[k] ** 2
        J.append(blk)
        Jt.append([2 * (a / b) / T if b != 0 else None for a, b in zip(num, den)])
    return J, Jt


# ---------------------------------------------------------------------------------------------------- objectives
def deriv_energy(Y, nveh, dim, R, tf, order):
    """sum over vehicles of the elevated control points of normSquare(diff^order(P)) (accel: 2, jerk: 3)"""
    T = F(float(tf))
    tot = F(0)
    for v in range(nveh):
        X = [fr(Y[v * dim + c]) for c in range(dim)]
        for _ in range(order - 1):
            X = [diff(x, T) for x in X]
        tot += sum(elev(_speed_raw(X, T), R))
    return tot


def deriv_energy_grad(Y, nveh, dim, R, tf, order):
    """([N*dim][nc], d/dtf): unit central differences (the objective is quadratic in each control point)"""
    nc = len(Y[0])
    T = F(float(tf))
    Yf = [fr(r) for r in Y]

    def f(Yq):
        tot = F(0)
        for v in range(nveh):
            X = Yq[v * dim:(v + 1) * dim]
            for _ in range(order - 1):
                X = [diff(x, T) for x in X]
            tot += sum(elev(_speed_raw(X, T), R))
        return tot
    g = [[F(0)] * nc for _ in range(nveh * dim)]
    for r in range(nveh * dim):
        for i in range(nc):
            Yp, Ym = [list(x) for x in Yf], [list(x) for x in Yf]
            Yp[r][i] += 1
            Ym[r][i] -= 1
            g[r][i] = (f(Yp) - f(Ym)) / 2
    return g, -2 * order * f(Yf) / T
