"""The yardstick of the keep-in rows, their true margins and their envelope Jacobian (obtg_keep_in,
obtg_keep_in_true_min[_jac]), in EXACT rationals.  No device, no reference code.

A region is F half-spaces a_f . p <= b_f, H[F][d + 1] = (a_f, b_f); an item is a (vehicle, face) pair of VF[P][2].  For
vehicle v with control points P[c][i] (c < d, i <= n)

    g(t) = b_f - a_f . c_v(t),    Bernstein coefficient i:  g_i = b_f - sum_c a_f[c] P[c][i],

a polynomial of the curve's own degree.  Its partial derivative with respect to the vehicle's control point (c, i) at a
parameter t is -a_f[c] B_i^n(t); no time span enters.

A float64 is a dyadic rational: Y, H and t are taken as Fractions and everything below is exact.  The forward-error bounds
follow tests/bezier_algebra_ref.py: a candidate passes when |candidate - value| <= K * 2^-53 * M, M the same formula on
absolute values, K the rounded operations on the element's longest chain in the device's kernel
(csrc/bern_device.h keep_in_coeff: d fused multiply-adds, one rounding each -> K = d; the output transform fma(1, g, 0) is
exact).  Elevated rows (R > 0) are k_bern_elev's arithmetic on the rounded coefficients: its T_k + 10 on top, on the elevation
of the majorants (its weights are positive, and |g_i| <= M_i)."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bezier_algebra_ref as A  # noqa: E402
import envelope_ref as E  # noqa: E402
import extrema_ref as R  # noqa: E402


def _fr(x):
    return Fraction(float(x))


def coeffs(Y, dim, H, VF):
    """(g, M): [P][n + 1] Fractions each -- the exact coefficients of every item of the row Y[N * dim][n + 1] and their
    majorants |b| + sum_c |a[c]| |P[c][i]|"""
    Y, H = np.asarray(Y, dtype=np.float64), np.asarray(H, dtype=np.float64)
    nc = Y.shape[1]
    g, M = [], []
    for v, f in np.asarray(VF).reshape(-1, 2).tolist():
        a, b = [_fr(x) for x in H[f, :dim]], _fr(H[f, dim])
        P = [[_fr(x) for x in Y[v * dim + c]] for c in range(dim)]
        g.append([b - sum(a[c] * P[c][i] for c in range(dim)) for i in range(nc)])
        M.append([abs(b) + sum(abs(a[c]) * abs(P[c][i]) for c in range(dim)) for i in range(nc)])
    return g, M


def rows_ref(Y, dim, H, VF, R_=0):
    """bezier_algebra_ref.Ref of obtg_keep_in's rows of the row Y at elevation R_: shape (P, n + R_ + 1), K = d (+ T_k + 10)"""
    g, M = coeffs(Y, dim, H, VF)
    P, nc = len(g), len(g[0])
    n = nc - 1
    if R_ == 0:
        return A.Ref.from_fractions([x for r in g for x in r], [x for r in M for x in r], [dim] * (P * nc), (P, nc))
    bn, bR, bo = A._binrow(n), A._binrow(R_), A._binrow(n + R_)
    val, maj, K = [], [], []
    for r, m in zip(g, M):
        for k in range(nc + R_):
            js = range(max(0, k - R_), min(n, k) + 1)
            val.append(sum(r[j] * bn[j] * bR[k - j] for j in js) / bo[k])
            maj.append(sum(m[j] * bn[j] * bR[k - j] for j in js) / bo[k])
            K.append(dim + A._terms(nc, R_ + 1, k) + 10)
    return A.Ref.from_fractions(val, maj, K, (P, nc + R_))


def float_coeffs(Y, dim, H, VF):
    """float64 [P][n + 1]: the exact coefficients, each rounded once (what certified_min is given)"""
    return np.array([[float(x) for x in r] for r in coeffs(Y, dim, H, VF)[0]])


def true_rows(Y, dim, H, VF, rel=R.REL):
    """[P] dicts(L, H, t, nodes, s): the certified minimum over [0, 1] of every item's polynomial"""
    return [R.certified_min(c, rel) for c in float_coeffs(Y, dim, H, VF)]


def envelope_block(h, dim, n, t):
    """[dim][n + 1] Fractions: d g / d P[c][i] at t for the face h = (a, b)"""
    w = E.basis(n, _fr(t))
    return [[-_fr(h[c]) * w[i] for i in range(n + 1)] for c in range(dim)]


def envelope_blocks(dim, n, H, VF, t_star):
    """float64 [P][dim][n + 1]: every item's block at its own t_star[P]"""
    VF = np.asarray(VF).reshape(-1, 2)
    out = np.zeros((VF.shape[0], dim, n + 1))
    for p, (_, f) in enumerate(VF.tolist()):
        out[p] = np.array([[float(x) for x in row] for row in envelope_block(np.asarray(H)[f], dim, n, t_star[p])])
    return out


def scatter(blk, VF, n_veh, dim, first, num_cols, D=None):
    """Dense [P][n_veh * dim * num_cols (+ 1)] from blocks [P][dim][n + 1]: the free columns first .. first + num_cols of the
    block, in the columns of the item's own vehicle -- the layout of BezOptimization's x.  D[N * dim][n + 1] (time-optimal
    problems): dY/dtf; the last column is then the block along D (the rows have no explicit d/dtf)."""
    VF = np.asarray(VF).reshape(-1, 2)
    J = np.zeros((VF.shape[0], n_veh * dim * num_cols))
    for p, (v, _) in enumerate(VF.tolist()):
        J[p, v * dim * num_cols:(v + 1) * dim * num_cols] = blk[p][:, first:first + num_cols].reshape(-1)
    if D is None:
        return J
    D = np.asarray(D, dtype=np.float64).reshape(n_veh, dim, -1)
    col = np.array([float((blk[p] * D[v]).sum()) for p, (v, _) in enumerate(VF.tolist())])
    return np.hstack((J, col[:, None]))


# ---------------------------------------------------------------------------------------------------------------------
#  the inputs the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
def vehicles(deg, dim, seed, n_veh=3):
    """Y[n_veh * dim][deg + 1]: synth.swarm_control_points, seeded"""
    from optimalbeziertrajectorygeneration_amd import synth
    return np.ascontiguousarray(synth.swarm_control_points(n_veh, dim, deg, seed=seed), dtype=np.float64)


def _place(ends, cps):
    """b of a face a . p <= b from the values a . p at the vehicle's two end points and at all its control points: between
    the extreme end point and the extreme control point, a quarter of the way out, so that the end points are inside and the
    extreme control point is not (a quarter, not half: the curve itself then leaves through some faces); where an end point
    IS the extreme control point, 0.25 beyond it (a face the curve cannot reach)."""
    e, c = max(ends), max(cps)
    return e + 0.25 * (c - e) if c > e else e + 0.25


def region(Y, dim):
    """(keepIn, H, VF) for the vehicles of Y[N * dim][n + 1]: per vehicle 2 dim axis faces (+e_0, -e_0, +e_1, ...) and one
    oblique face, each placed by _place; keepIn is the per-vehicle list BezOptimization takes, (H, VF) the tables it comes to."""
    Y = np.asarray(Y, dtype=np.float64)
    N = Y.shape[0] // dim
    oblique = np.array([1.0, 0.5, -0.25])[:dim]
    keep, Hs, VF = [], [], []
    for v in range(N):
        Pv = Y[v * dim:(v + 1) * dim]
        normals = [s * np.eye(dim)[c] for c in range(dim) for s in (1.0, -1.0)] + [oblique]
        Av = np.array(normals)
        vals = Av @ Pv                                              # [faces][n + 1]
        bv = np.array([_place(vals[f, [0, -1]], vals[f]) for f in range(Av.shape[0])])
        keep.append((Av, bv))
        VF += [(v, len(Hs) + f) for f in range(Av.shape[0])]
        Hs += list(np.hstack((Av, bv[:, None])))
    return keep, np.array(Hs), np.array(VF, dtype=np.int32)
