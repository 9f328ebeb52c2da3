"""The yardstick of the keep-out rows against obstacles that MOVE (obtg_keep_out_moving_true_min[_jac],
obtg_bern_keep_out_moving).  No device, no reference code.  Beside tests/keep_out_ref.py, which it builds on.

Obstacle o keeps its faces H = (a_f, b_f) and is translated by a Bezier offset q(time), control points Q[d][m + 1] on the
absolute span [0, T].  A vehicle with control points P[d][n + 1] (m <= n) lives on [0, tf].  With s in [0, 1], r = tf / T:

    E(s) = q(s tf)         q restricted to [0, r] of its own parameter, raised to degree n
    D_i  = P_i - E_i       the relative control points
    row  = min_s max_f (a_f . D(s) - b_f) - margin:  the static row (keep_out_ref) of the curve D.

(1) EXACT rationals (a float64 is a dyadic rational): r = tf / T as a rational, the restriction by the blossom -- point j of
the piece over [0, r] is sum_i B_i^j(r) Q_i --, the elevation E_i = sum_j C(m, j) C(n - m, i - j) / C(n, i) Q_j, the difference.
(2) The explicit derivative with respect to tf at a given (t, f1, f2, lam):

    d row / d tf = -(a^ . E'(t)) t / tf,    a^ = lam a_f1 + (1 - lam) a_f2,    E'(t) = n sum_i (E_(i+1) - E_i) B_i^(n-1)(t)

because dE(s) / d tf = s q'(s tf) = s E'(s) / tf and D = P - E.

Rounding allowance of the device's relative points (rel_allowance), per coordinate c, for 0 < r <= 1, in the convention of
keep_out_ref.value_allowance (one rounding is at most 2^-53 of the largest magnitude it acts on; first order).  The device's
arithmetic is fixed in include/obtg.h; with Mq = max_j |Q[c][j]| (every intermediate value is a convex combination of the
Q[c][j], so Mq bounds it) and Mp = max_i |P[c][i]|:
  ratio        r = fl(tf / T): one rounding, |dr| <= 2^-53 r <= 2^-53.  Point j of the restricted piece moves by at most
               j |blossom difference| |dr| <= 2 m Mq 2^-53                                                    2 m   on Mq
  restriction  at most m levels on the way to a point; a level is fma(r, up, fl(1 - r) * b): the rounding of 1 - r (the two
               weights then sum to 1 within 2^-53), the rounding of the product and the rounding of the fma       3 m   on Mq
  elevation    n - m steps; a step is fma(w, prev, fl(1 - w) * cur) with w = fl(i / (k + 1)): the roundings of w and of
               1 - w, of the product and of the fma                                                          4 (n - m) on Mq
  difference   one subtraction                                                                                  1 on Mp + Mq
Later levels and steps are convex combinations and do not amplify what earlier ones left.  So
    |rel[c][i] - exact| <= K 2^-53 M,    K = 5 m + 4 (n - m) + 1,    M = Mp + Mq.
No bound is claimed for r > 1 (de Casteljau outside [0, 1] is not a convex combination)."""
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import keep_out_ref as K  # noqa: E402

fr = K.fr


# ---------------------------------------------------------------------------------------------------------------------
#  (1) exact rationals
# ---------------------------------------------------------------------------------------------------------------------
def ratio(tf, T):
    return fr(tf) / fr(T)


def restrict(q, r):
    """[m + 1] Fractions: the control points of q over [0, r] of its parameter, by the blossom"""
    m = len(q) - 1
    r = fr(r)
    return [sum(w * fr(x) for w, x in zip(K.basis(j, r), q[:j + 1])) for j in range(m + 1)]


def elevate(e, n):
    """[n + 1] Fractions: the degree-m control points e at degree n >= m"""
    m = len(e) - 1
    return [sum(Fraction(math.comb(m, j) * math.comb(n - m, i - j), math.comb(n, i)) * e[j]
                for j in range(max(0, i - (n - m)), min(m, i) + 1)) for i in range(n + 1)]


def motion_points(Q, r, n):
    """E[d][n + 1] Fractions of the motion Q[d][m + 1] at the ratio r"""
    return [elevate(restrict(list(row), r), n) for row in np.asarray(Q, dtype=np.float64)]


def relative(P, Q, r):
    """D[d][n + 1] Fractions: P - E"""
    P = np.asarray(P, dtype=np.float64)
    E = motion_points(Q, r, P.shape[1] - 1)
    return [[fr(P[c, i]) - E[c][i] for i in range(P.shape[1])] for c in range(P.shape[0])]


def rounded(D):
    """the exact points rounded once to float64"""
    return np.array([[float(x) for x in row] for row in D])


def bezier_at(cp, t):
    """sum_i B_i(t) cp_i in exact rationals"""
    return sum(w * fr(x) for w, x in zip(K.basis(len(cp) - 1, t), cp))


def relative_at(P, Q, r, s):
    """[d] Fractions: c(s) - q(s r), evaluated directly"""
    return [bezier_at(list(p), s) - bezier_at(list(q), fr(s) * fr(r)) for p, q in zip(np.asarray(P, dtype=np.float64),
                                                                                      np.asarray(Q, dtype=np.float64))]


def rel_allowance(P, Q):
    """[d] floats: K 2^-53 M per coordinate (module docstring): K = 5 m + 4 (n - m) + 1, M = max |P[c]| + max |Q[c]|"""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    n, m = P.shape[1] - 1, Q.shape[1] - 1
    return (5 * m + 4 * (n - m) + 1) * 2.0 ** -53 * (np.abs(P).max(axis=1) + np.abs(Q).max(axis=1))


# ---------------------------------------------------------------------------------------------------------------------
#  (2) the explicit d row / d tf
# ---------------------------------------------------------------------------------------------------------------------
def deriv_at(cp, t):
    """the derivative with respect to the parameter of the curve with control points cp (Fractions), at t"""
    n = len(cp) - 1
    if n == 0:
        return Fraction(0)
    return n * sum((cp[i + 1] - cp[i]) * w for i, w in enumerate(K.basis(n - 1, t)))


def a_hat(H, f1, f2, lam):
    H = np.asarray(H, dtype=np.float64)
    d = H.shape[1] - 1
    lam = fr(lam)
    return [fr(H[f1, c]) if f2 < 0 else lam * fr(H[f1, c]) + (1 - lam) * fr(H[f2, c]) for c in range(d)]


def jac_tf(E, H, t, f1, f2, lam, tf):
    """-(a^ . E'(t)) t / tf in exact rationals; E[d][n + 1] Fractions (motion_points)"""
    a = a_hat(H, f1, f2, lam)
    return -sum(ac * deriv_at(Ec, t) for ac, Ec in zip(a, E)) * fr(t) / fr(tf)


def jac_tf_scale(E, H, f1, f2, lam, tf):
    """|a^| max |E'| / tf: the scale jac_tf is held on (E' bounded by n times the largest difference of its control points)"""
    a = a_hat(H, f1, f2, lam)
    n = len(E[0]) - 1
    dE = max([abs(Ec[i + 1] - Ec[i]) for Ec in E for i in range(n)] or [Fraction(0)]) * n
    return float(math.sqrt(float(sum(x * x for x in a))) * float(dE) / float(tf))


def searched_row(P, Q, T, tf, H, eps_rel=1e-12):
    """keep_out_ref.search on the correctly rounded relative points"""
    return K.search(rounded(relative(P, Q, ratio(tf, T))), H, eps_rel)


def forward_difference_tf(P, Q, T, tf, H, h=1e-6, eps_rel=1e-12):
    """(row(tf + h) - row(tf)) / ((tf + h) - tf): the difference quotient in tf of the yardstick's own searched row"""
    t1 = tf + h
    return (searched_row(P, Q, T, t1, H, eps_rel)["val"] - searched_row(P, Q, T, tf, H, eps_rel)["val"]) / (t1 - tf)


def row(P, Q, T, tf, H, eps_rel=1e-12):
    """dict(val, t, f1, f2, lam, jac_tf, D): the row of the rounded relative points, its active faces by the exact rule at the
    search's t, and the exact d/dtf there, rounded once"""
    r = ratio(tf, T)
    D = rounded(relative(P, Q, r))
    sr = K.search(D, H, eps_rel)
    f1, f2, lam = K.active(D, H, sr["t"], sr["tol"])
    E = motion_points(Q, r, D.shape[1] - 1)
    return dict(val=sr["val"], t=sr["t"], f1=f1, f2=f2, lam=float(lam), D=D, jac_tf=float(jac_tf(E, H, sr["t"], f1, f2, lam, tf)))


# ---------------------------------------------------------------------------------------------------------------------
#  inputs the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
def motions(dim, m, seed, O=2):
    """[O] arrays [dim][m + 1]: offsets that start near 0 and wander by about one unit -- the batch of keep_out_ref.batch still
    passes by, grazes and crosses the translated obstacles"""
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-1.0, 1.0, size=(O, dim, m + 1))
    Q[..., 0] *= 0.25
    return [np.ascontiguousarray(q) for q in Q]


def motion_tables(Qs):
    """(Q, q_off) as obtg_ctx_set_keep_out_motion takes them; None: an obstacle that stands still"""
    blocks = [np.asarray(q, dtype=np.float64).reshape(-1) for q in Qs if q is not None]
    counts = [0 if q is None else np.asarray(q).shape[1] for q in Qs]
    return (np.concatenate(blocks) if blocks else np.zeros(0)), np.cumsum([0] + counts).astype(np.int32)


def spans(r, B=5, tf0=2.0):
    """(tf[B], T): the rows' spans, all different, the longest first, and the motion's span with tf[0] / T == r"""
    tf = tf0 * (1.0 - 0.0625 * np.arange(B))
    return tf, tf0 / r
