"""The yardstick of the true angular-rate rows and their envelope Jacobian (obtg_ang_rate_poly, obtg_ang_rate_true_min[_jac]),
in EXACT rationals.  No device, no reference code.

For one planar vehicle with control points x_i, y_i (i <= n) on a time span T, with x' = dx/dtime and x'' its derivative,

    den(t) = x'^2 + y'^2,    num(t) = y'' x' - x'' y',    omega(t) = num / den          (optimization.py:543-574)
    p_sigma(t) = W den(t) - sigma num(t),     sigma = +1 (side 0, left turns), -1 (side 1, right turns):

|omega| <= W on [0, 1] iff min_t p_+ >= 0 and min_t p_- >= 0.  The rows are in units of W * speed^2, not W^2 - omega^2.
With w = B^(n-1)(t), u = B^(n-2)(t), entries out of range 0:

    x'(t)  = (n/T) sum_i w_i (x_(i+1) - x_i),      x''(t) = (n(n-1)/T^2) sum_i u_i (x_(i+2) - 2 x_(i+1) + x_i)
    A_i = (n/T)(w_(i-1) - w_i),                    C_i = (n(n-1)/T^2)(u_(i-2) - 2 u_(i-1) + u_i)
    d p / d x_i = 2 W x' A_i - sigma (y'' A_i - y' C_i)
    d p / d y_i = 2 W y' A_i - sigma (x' C_i - x'' A_i)
    d p / d T   = (-2 W den + 3 sigma num) / T

A float64 is a dyadic rational: `y`, `tf`, `W` and `t` are taken as Fractions and everything below is exact.
test_ang_envelope_ref.py holds the formulas to the oracle's Bernstein algebra (diff, diff, mul)."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envelope_ref as E  # noqa: E402
import extrema_ref as R  # noqa: E402

SIGMA = (1, -1)          # side -> sigma


def _F(x):
    return Fraction(float(x))


def _basis(n, t):
    return E.basis(n, t) if n >= 0 else []


def derivatives(yv, tf, t):
    """(x', y', x'', y'', w, u) at t, exact; yv: the vehicle's [2][n + 1] control points"""
    yv = np.asarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    t, T = _F(t), _F(tf)
    w, u = _basis(n - 1, t), _basis(n - 2, t)
    nT, nnT = Fraction(n) / T, Fraction(n * (n - 1)) / (T * T)
    P = [[_F(v) for v in row] for row in yv]
    d1 = [nT * sum(w[i] * (P[c][i + 1] - P[c][i]) for i in range(n)) for c in range(2)]
    d2 = [nnT * sum(u[i] * (P[c][i + 2] - 2 * P[c][i + 1] + P[c][i]) for i in range(n - 1)) for c in range(2)]
    return d1[0], d1[1], d2[0], d2[1], w, u


def den_num(yv, tf, t):
    xd, yd, xdd, ydd, _, _ = derivatives(yv, tf, t)
    return xd * xd + yd * yd, ydd * xd - xdd * yd


def row(yv, tf, W, side, t):
    """p_sigma(t), exact"""
    den, num = den_num(yv, tf, t)
    return _F(W) * den - SIGMA[side] * num


def omega(yv, tf, t):
    """the angular rate at t, exact (the speed must not vanish there)"""
    den, num = den_num(yv, tf, t)
    return num / den


def envelope_block(yv, tf, W, side, t):
    """([2][n + 1] Fractions: d p_sigma / d (x_i, y_i) at t, Fraction: d p_sigma / d T at t)"""
    yv = np.asarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    T, Wf, sg = _F(tf), _F(W), SIGMA[side]
    xd, yd, xdd, ydd, w, u = derivatives(yv, tf, t)
    nT, nnT = Fraction(n) / T, Fraction(n * (n - 1)) / (T * T)

    def at(b, i):
        return b[i] if 0 <= i < len(b) else Fraction(0)
    A = [nT * (at(w, i - 1) - at(w, i)) for i in range(n + 1)]
    Cc = [nnT * (at(u, i - 2) - 2 * at(u, i - 1) + at(u, i)) for i in range(n + 1)]
    bx = [2 * Wf * xd * A[i] - sg * (ydd * A[i] - yd * Cc[i]) for i in range(n + 1)]
    by = [2 * Wf * yd * A[i] - sg * (xd * Cc[i] - xdd * A[i]) for i in range(n + 1)]
    den, num = xd * xd + yd * yd, ydd * xd - xdd * yd
    return [bx, by], (-2 * Wf * den + 3 * sg * num) / T


def envelope_blocks(Y, tf, W, t_star):
    """float64 ([N][2][2][n + 1], [N][2]): every (vehicle, side)'s block and d/dtf of the row Y[N * 2][n + 1] at its own
    t_star[N][2]"""
    Y = np.asarray(Y, dtype=np.float64)
    t_star = np.asarray(t_star, dtype=np.float64)
    N = Y.shape[0] // 2
    blk, dtf = np.zeros((N, 2, 2, Y.shape[1])), np.zeros((N, 2))
    for v in range(N):
        for side in range(2):
            b, g = envelope_block(Y[2 * v:2 * v + 2], tf, W, side, t_star[v, side])
            blk[v, side] = np.array([[float(x) for x in r] for r in b])
            dtf[v, side] = float(g)
    return blk, dtf


def den_num_coeffs(Y, tf):
    """([N][2n + 1], [N][2n + 1]): the Bernstein coefficients of den and num of every vehicle of the row Y[N * 2][n + 1], from
    the oracle's diff and mul alone -- the chain of the reference's _angularRate: its `weights` and `cpts * weights`"""
    from oracle import oracle as O
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    d1 = O.diff(Y, float(tf))
    d2 = O.diff(d1, float(tf))
    x1, y1, x2, y2 = d1[0::2], d1[1::2], d2[0::2], d2[1::2]
    return O.mul(x1, x1) + O.mul(y1, y1), O.mul(y2, x1) - O.mul(x2, y1)


def ang_coeffs(Y, tf, W):
    """[N][2][2n + 1]: the rows' polynomials W den -+ num of the row Y[N * 2][n + 1]"""
    den, num = den_num_coeffs(Y, tf)
    return np.stack((float(W) * den - num, float(W) * den + num), axis=1)


def true_rows(Y, tf, W, rel=R.REL):
    """[N][2] dicts(L, H, t, nodes, s): the certified minimum over [0, 1] of every (vehicle, side)'s polynomial"""
    co = ang_coeffs(Y, tf, W)
    return [[R.certified_min(co[v, side], rel) for side in range(2)] for v in range(co.shape[0])]


def oracle_row(yv, tf, W, side, t):
    """p_sigma(t) from the oracle's coefficients contracted with the exact B_k^2n(t): a Fraction"""
    yv = np.ascontiguousarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    co = ang_coeffs(yv, tf, W)[0, side]
    w2 = E.basis(2 * n, _F(t))
    return sum(w2[k] * _F(co[k]) for k in range(2 * n + 1))


def oracle_den_num(yv, tf, t):
    """(den(t), num(t)) from the oracle's coefficients contracted with the exact B_k^2n(t): Fractions"""
    yv = np.ascontiguousarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    den, num = den_num_coeffs(yv, tf)
    w2 = E.basis(2 * n, _F(t))
    return sum(w2[k] * _F(den[0, k]) for k in range(2 * n + 1)), sum(w2[k] * _F(num[0, k]) for k in range(2 * n + 1))


def oracle_block(yv, tf, W, side, t, h=0.5):
    """The block of one (vehicle, side) from the ORACLE's coefficients: central differences with a power-of-two step (exact
    because p is at most quadratic in each control point, up to the rounding of the coefficients; y +- h must be exact),
    contracted with the exact B_k^2n(t).  float64 [2][n + 1]."""
    yv = np.ascontiguousarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    w2 = E.basis(2 * n, _F(t))
    out = np.zeros((2, n + 1))
    for c in range(2):
        for i in range(n + 1):
            yp, ym = yv.copy(), yv.copy()
            yp[c, i] += h
            ym[c, i] -= h
            assert yp[c, i] - yv[c, i] == h and yv[c, i] - ym[c, i] == h
            cp, cm = ang_coeffs(yp, tf, W)[0, side], ang_coeffs(ym, tf, W)[0, side]
            out[c, i] = float(sum(w2[k] * (_F(cp[k]) - _F(cm[k])) for k in range(2 * n + 1)) / Fraction(2 * h))
    return out


def scatter(blk, dtf, n_veh, first, num_cols, D=None):
    """Dense [2N][n_veh * 2 * num_cols (+ 1)] from blocks [N][2][2][n + 1], row 2 v + side: the layout speed_envelope_ref.scatter
    gives, once per side"""
    import speed_envelope_ref as S
    sides = [S.scatter(blk[:, side], dtf[:, side], n_veh, 2, first, num_cols, D) for side in range(2)]
    J = np.zeros((2 * n_veh, sides[0].shape[1]))
    J[0::2], J[1::2] = sides[0], sides[1]
    return J
