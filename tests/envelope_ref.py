"""The yardstick of the envelope-Jacobian tests, in EXACT rationals.  No device, no reference code.

For a pair (a, b) of one evaluation row the squared-separation polynomial is p(t) = (d/2) |Delta(t)|^2, Delta = v_a - v_b
(normSquare's factor), so its partial derivative with respect to a's control point (c, i) at a parameter t is

    KAPPA * B_i^n(t) * Delta_c(t),        KAPPA = d.

A float64 is a dyadic rational: `y` and `t` are taken as Fractions and everything below is exact.  test_envelope_ref.py
holds KAPPA to the oracle (central differences of its coefficients, which are exact for a quadratic)."""
import os
import sys
from fractions import Fraction
from math import comb

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extrema_ref as R  # noqa: E402


def kappa(dim):
    return dim


def basis(n, t):
    """[B_0^n(t) .. B_n^n(t)], exact"""
    t = Fraction(t)
    s = 1 - t
    return [comb(n, i) * t ** i * s ** (n - i) for i in range(n + 1)]


def full_row(Y, obs):
    """one evaluation row with the point obstacles as constant curves behind the vehicles: [n_obj * dim][n + 1]"""
    Y = np.asarray(Y, dtype=np.float64)
    if obs is None or len(obs) == 0:
        return Y
    return np.vstack([Y, np.repeat(np.asarray(obs, dtype=np.float64).reshape(-1, 1), Y.shape[1], axis=1)])


def pairs(n_obj):
    return [(a, b) for a in range(n_obj - 1) for b in range(a + 1, n_obj)]


def envelope_block(y, dim, n_veh, a, b, t):
    """[dim][n + 1] Fractions: d p / d y[a * dim + c][i] at t for the pair (a, b) of the row y[n_obj * dim][n + 1]; all zeros
    when a is a point obstacle (a >= n_veh: no variable on either side)."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[1] - 1
    if a >= n_veh:
        return [[Fraction(0)] * (n + 1) for _ in range(dim)]
    w = basis(n, Fraction(float(t)))
    out = []
    for c in range(dim):
        dl = sum(w[i] * (Fraction(float(y[a * dim + c, i])) - Fraction(float(y[b * dim + c, i]))) for i in range(n + 1))
        out.append([kappa(dim) * w[i] * dl for i in range(n + 1)])
    return out


def envelope_blocks(y, dim, n_veh, n_obj, t_star):
    """float64 [P][dim][n + 1]: every pair's block at its own t_star[P]"""
    y = np.asarray(y, dtype=np.float64)
    out = np.zeros((n_obj * (n_obj - 1) // 2, dim, y.shape[1]))
    for p, (a, b) in enumerate(pairs(n_obj)):
        out[p] = np.array([[float(v) for v in row] for row in envelope_block(y, dim, n_veh, a, b, t_star[p])])
    return out


def oracle_block(y, n_obj, dim, a, b, t, h=0.5):
    """The same block from the ORACLE's coefficients: central differences with a power-of-two step (exact for a quadratic up
    to the rounding of the coefficients; y +- h must be exact), contracted with the exact B_k^2n(t).  float64 [dim][n + 1]."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    n = y.shape[1] - 1
    p = pairs(n_obj).index((a, b))
    w2 = basis(2 * n, Fraction(float(t)))
    out = np.zeros((dim, n + 1))
    for c in range(dim):
        for i in range(n + 1):
            yp, ym = y.copy(), y.copy()
            yp[a * dim + c, i] += h
            ym[a * dim + c, i] -= h
            assert yp[a * dim + c, i] - y[a * dim + c, i] == h and y[a * dim + c, i] - ym[a * dim + c, i] == h
            cp, cm = R.separation_coeffs(yp, n_obj, dim, 1.0)[p], R.separation_coeffs(ym, n_obj, dim, 1.0)[p]
            out[c, i] = float(sum(w2[k] * (Fraction(float(cp[k])) - Fraction(float(cm[k]))) for k in range(2 * n + 1)) / Fraction(2 * h))
    return out


def scatter(blk, n_veh, n_obj, dim, first, num_cols):
    """Dense [P][n_veh * dim * num_cols] from blocks [P][dim][n + 1]: the free columns first .. first + num_cols of the pair's
    first object, negated for its second (a point obstacle has no variable) -- the layout of BezOptimization's x."""
    J = np.zeros((blk.shape[0], n_veh * dim * num_cols))
    for p, (a, b) in enumerate(pairs(n_obj)):
        for own, sg in ((a, 1.0), (b, -1.0)):
            if own < n_veh:
                J[p, own * dim * num_cols:(own + 1) * dim * num_cols] += sg * blk[p][:, first:first + num_cols].reshape(-1)
    return J
