"""The yardstick of the true speed rows and their envelope Jacobian (obtg_speed_true_min[_jac]), in EXACT rationals.  No
device, no reference code.

For one vehicle with control points P[c][i] (c < d, i <= n) on a time span T the speed row's polynomial is

    q(t) = sign * (d/2) |c'(t)|^2 + offset,      c'_c(t) = (n/T) sum_i B_i^(n-1)(t) (P[c][i+1] - P[c][i]),

(sign, offset) = (-1, +bound^2) for the maximum-speed rows, (+1, -bound^2) for the minimum-speed rows (normSquare's (d/2)
factor).  Its partial derivatives at a parameter t, with w = B^(n-1)(t) and w_(-1) = w_n = 0:

    d q / d P[c][i] = sign * d * c'_c(t) * (n/T) * (w_(i-1) - w_i)
    d q / d T       = -2 (q(t) - offset) / T

A float64 is a dyadic rational: `y`, `tf` and `t` are taken as Fractions and everything below is exact.
test_speed_envelope_ref.py holds the formulas to the oracle's speed coefficients."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envelope_ref as E  # noqa: E402
import extrema_ref as R  # noqa: E402


def transform(bound, is_max):
    """(sign, offset) of a speed row, exact (bound ** 2 as Python forms it, then taken as the rational it is)"""
    b2 = Fraction(float(bound) ** 2)
    return (Fraction(-1), b2) if is_max else (Fraction(1), -b2)


def velocity(yv, tf, t):
    """([c'_c(t)] for c < d, w = B^(n-1)(t)), exact; yv: the vehicle's [d][n + 1] control points"""
    yv = np.asarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    w = E.basis(n - 1, Fraction(float(t)))
    nT = Fraction(n) / Fraction(float(tf))
    vel = [nT * sum(w[i] * (Fraction(float(yv[c, i + 1])) - Fraction(float(yv[c, i]))) for i in range(n)) for c in range(yv.shape[0])]
    return vel, w


def row_minus_offset(yv, tf, is_max, t):
    """q(t) - offset = sign (d/2) |c'(t)|^2, exact"""
    vel, _ = velocity(yv, tf, t)
    sign = -1 if is_max else 1
    return sign * Fraction(len(vel), 2) * sum(v * v for v in vel)


def envelope_block(yv, tf, is_max, t):
    """([d][n + 1] Fractions: d q / d P[c][i] at t, Fraction: d q / d T at t)"""
    yv = np.asarray(yv, dtype=np.float64)
    d, n = yv.shape[0], yv.shape[1] - 1
    vel, w = velocity(yv, tf, t)
    sign = -1 if is_max else 1
    nT = Fraction(n) / Fraction(float(tf))
    wl = [Fraction(0)] + list(w) + [Fraction(0)]          # wl[i] = w_(i-1)
    blk = [[sign * d * vel[c] * nT * (wl[i] - wl[i + 1]) for i in range(n + 1)] for c in range(d)]
    dtf = -2 * (sign * Fraction(d, 2) * sum(v * v for v in vel)) / Fraction(float(tf))
    return blk, dtf


def envelope_blocks(Y, dim, tf, is_max, t_star):
    """float64 ([N][dim][n + 1], [N]): every vehicle's block and d/dtf of the row Y[N * dim][n + 1] at its own t_star[N]"""
    Y = np.asarray(Y, dtype=np.float64)
    N = Y.shape[0] // dim
    blk, dtf = np.zeros((N, dim, Y.shape[1])), np.zeros(N)
    for v in range(N):
        b, g = envelope_block(Y[v * dim:(v + 1) * dim], tf, is_max, t_star[v])
        blk[v] = np.array([[float(x) for x in row] for row in b])
        dtf[v] = float(g)
    return blk, dtf


def speed_coeffs(Y, dim, tf, bound, is_max):
    """The speed rows' polynomials of one evaluation row Y[N * dim][n + 1]: oracle.speed at R = 0, [N][2n + 1]"""
    from oracle import oracle as O
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n = Y.shape[1] - 1
    return O.speed(Y, Y.shape[0] // dim, dim, 0, float(tf), float(bound), bool(is_max)).reshape(-1, 2 * n + 1)


def true_rows(Y, dim, tf, bound, is_max, rel=R.REL):
    """[N] dicts(L, H, t, nodes, s): the certified minimum over [0, 1] of every vehicle's row polynomial"""
    co = speed_coeffs(Y, dim, tf, bound, is_max)
    return [R.certified_min(co[v], rel) for v in range(co.shape[0])]


def oracle_block(yv, tf, bound, is_max, t, h=0.5):
    """The block of one vehicle from the ORACLE's coefficients: central differences with a power-of-two step (exact for a
    quadratic up to the rounding of the coefficients; y +- h must be exact), contracted with the exact B_k^2n(t).
    float64 [d][n + 1]."""
    yv = np.ascontiguousarray(yv, dtype=np.float64)
    d, n = yv.shape[0], yv.shape[1] - 1
    w2 = E.basis(2 * n, Fraction(float(t)))
    out = np.zeros((d, n + 1))
    for c in range(d):
        for i in range(n + 1):
            yp, ym = yv.copy(), yv.copy()
            yp[c, i] += h
            ym[c, i] -= h
            assert yp[c, i] - yv[c, i] == h and yv[c, i] - ym[c, i] == h
            cp, cm = speed_coeffs(yp, d, tf, bound, is_max)[0], speed_coeffs(ym, d, tf, bound, is_max)[0]
            out[c, i] = float(sum(w2[k] * (Fraction(float(cp[k])) - Fraction(float(cm[k]))) for k in range(2 * n + 1)) / Fraction(2 * h))
    return out


def oracle_row_minus_offset(yv, tf, bound, is_max, t):
    """q(t) - offset from the oracle's coefficients, contracted with the exact B_k^2n(t): a Fraction"""
    yv = np.ascontiguousarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    co = speed_coeffs(yv, yv.shape[0], tf, bound, is_max)[0]
    w2 = E.basis(2 * n, Fraction(float(t)))
    return sum(w2[k] * Fraction(float(co[k])) for k in range(2 * n + 1)) - transform(bound, is_max)[1]


def scatter(blk, dtf, n_veh, dim, first, num_cols, D=None):
    """Dense [N][n_veh * dim * num_cols (+ 1)] from blocks [N][dim][n + 1]: the free columns first .. first + num_cols of the
    vehicle's own block -- the layout of BezOptimization's x.  D[N * dim][n + 1] (time-optimal problems): dY/dtf; the last
    column is then dtf + the block along D."""
    J = np.zeros((n_veh, n_veh * dim * num_cols))
    for v in range(n_veh):
        J[v, v * dim * num_cols:(v + 1) * dim * num_cols] = blk[v][:, first:first + num_cols].reshape(-1)
    if D is None:
        return J
    D = np.asarray(D, dtype=np.float64).reshape(n_veh, dim, -1)
    col = np.array([dtf[v] + float((blk[v] * D[v]).sum()) for v in range(n_veh)])
    return np.hstack((J, col[:, None]))
