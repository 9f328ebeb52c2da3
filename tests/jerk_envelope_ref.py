"""The yardstick of the true jerk rows and their envelope Jacobian (obtg_jerk_true_min[_jac]), in EXACT rationals.  No
device, no reference code.

For one vehicle with control points P[c][i] (c < d, i <= n) on a time span T the jerk row's polynomial is

    q(t) = bound^2 - (d/2) |c'''(t)|^2,
    c'''_c(t) = (n (n-1) (n-2) / T^3) sum_{i <= n-3} B_i^(n-3)(t) (P[c][i+3] - 3 P[c][i+2] + 3 P[c][i+1] - P[c][i]),

(normSquare's (d/2) factor; bound^2 as Python forms it).  Its partial derivatives at a parameter t, with
u = B^(n-3)(t) and entries out of range 0:

    C_i = (n (n-1) (n-2) / T^3) (u_(i-3) - 3 u_(i-2) + 3 u_(i-1) - u_i)
    d q / d P[c][i] = -d * c'''_c(t) * C_i
    d q / d T       = -6 (q(t) - bound^2) / T

A float64 is a dyadic rational: `y`, `tf` and `t` are taken as Fractions and everything below is exact.
test_jerk_envelope_ref.py holds the formulas to the oracle's jerk coefficients."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envelope_ref as E  # noqa: E402
import extrema_ref as R  # noqa: E402


def offset(bound):
    """bound ** 2 as Python forms it, then taken as the rational it is"""
    return Fraction(float(bound) ** 2)


def jerk(yv, tf, t):
    """([c'''_c(t)] for c < d, u = B^(n-3)(t) -- empty for n <= 2), exact; yv: the vehicle's [d][n + 1] control points"""
    yv = np.asarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    u = E.basis(n - 3, Fraction(float(t))) if n >= 3 else []
    T = Fraction(float(tf))
    nnT = Fraction(n * (n - 1) * (n - 2)) / (T * T * T)
    P = [[Fraction(float(x)) for x in row] for row in yv]
    jk = [nnT * sum(u[i] * (P[c][i + 3] - 3 * P[c][i + 2] + 3 * P[c][i + 1] - P[c][i]) for i in range(n - 2)) for c in range(yv.shape[0])]
    return jk, u


def row_minus_offset(yv, tf, t):
    """q(t) - bound^2 = -(d/2) |c'''(t)|^2, exact"""
    jk, _ = jerk(yv, tf, t)
    return -Fraction(len(jk), 2) * sum(a * a for a in jk)


def envelope_block(yv, tf, t):
    """([d][n + 1] Fractions: d q / d P[c][i] at t, Fraction: d q / d T at t)"""
    yv = np.asarray(yv, dtype=np.float64)
    d, n = yv.shape[0], yv.shape[1] - 1
    jk, u = jerk(yv, tf, t)
    T = Fraction(float(tf))
    nnT = Fraction(n * (n - 1) * (n - 2)) / (T * T * T)
    ul = [Fraction(0)] * 3 + list(u) + [Fraction(0)] * 3                            # ul[i + 3] = u_i
    Ci = [nnT * (ul[i] - 3 * ul[i + 1] + 3 * ul[i + 2] - ul[i + 3]) for i in range(n + 1)]
    blk = [[-d * jk[c] * Ci[i] for i in range(n + 1)] for c in range(d)]
    dtf = -6 * (-Fraction(d, 2) * sum(a * a for a in jk)) / T
    return blk, dtf


def envelope_blocks(Y, dim, tf, t_star):
    """float64 ([N][dim][n + 1], [N]): every vehicle's block and d/dtf of the row Y[N * dim][n + 1] at its own t_star[N]"""
    Y = np.asarray(Y, dtype=np.float64)
    N = Y.shape[0] // dim
    blk, dtf = np.zeros((N, dim, Y.shape[1])), np.zeros(N)
    for v in range(N):
        b, g = envelope_block(Y[v * dim:(v + 1) * dim], tf, t_star[v])
        blk[v] = np.array([[float(x) for x in row] for row in b])
        dtf[v] = float(g)
    return blk, dtf


def jerk_coeffs(Y, dim, tf, bound):
    """The jerk rows' polynomials of one evaluation row Y[N * dim][n + 1]: the oracle's maximum-speed rows of the
    second derivative's control points at R = 0, [N][2n + 1]"""
    from oracle import oracle as O
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n = Y.shape[1] - 1
    return O.speed(O.diff(O.diff(Y, float(tf)), float(tf)), Y.shape[0] // dim, dim, 0, float(tf), float(bound), True).reshape(-1, 2 * n + 1)


def true_rows(Y, dim, tf, bound, rel=R.REL):
    """[N] dicts(L, H, t, nodes, s): the certified minimum over [0, 1] of every vehicle's row polynomial"""
    co = jerk_coeffs(Y, dim, tf, bound)
    return [R.certified_min(co[v], rel) for v in range(co.shape[0])]


def oracle_block(yv, tf, bound, t, h=0.5):
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
            cp, cm = jerk_coeffs(yp, d, tf, bound)[0], jerk_coeffs(ym, d, tf, bound)[0]
            out[c, i] = float(sum(w2[k] * (Fraction(float(cp[k])) - Fraction(float(cm[k]))) for k in range(2 * n + 1)) / Fraction(2 * h))
    return out


def oracle_row_minus_offset(yv, tf, bound, t):
    """q(t) - bound^2 from the oracle's coefficients, contracted with the exact B_k^2n(t): a Fraction"""
    yv = np.ascontiguousarray(yv, dtype=np.float64)
    n = yv.shape[1] - 1
    co = jerk_coeffs(yv, yv.shape[0], tf, bound)[0]
    w2 = E.basis(2 * n, Fraction(float(t)))
    return sum(w2[k] * Fraction(float(co[k])) for k in range(2 * n + 1)) - offset(bound)


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
