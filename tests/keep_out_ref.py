"""The yardstick of the keep-out rows and their envelope Jacobian (obtg_keep_out_true_min[_jac], obtg_bern_keep_out).  No
device, no reference code.

An obstacle is a convex set {p : a_f . p <= b_f}, H[F][d + 1] = (a_f, b_f).  For a curve with control points P[c][i]
(c < d, i <= n)

    g_f(t) = a_f . c(t) - b_f        Bernstein coefficient i:  a_f . P_i - b_f       (the curve's own degree)
    G(t)   = max_f g_f(t)            (> 0 outside, minus the penetration depth inside)
    row    = min over t in [0, 1] of G(t)  -  margin.

Two things live here.  (1) The quantity in EXACT rationals (a float64 is a dyadic rational): g_f(t), g_f'(t), B_i^n(t), the
co-activity rule and the block formula at a given (t, f1, f2).  (2) A float64 branch and bound of its own (`search`,
best-first on a heap -- not the device's depth-first order), written from the definition above.

The envelope block at the minimiser t*, f1 = argmax_f g_f(t*):  one face at an end or a smooth interior minimum,
jac[c][i] = a_f1[c] B_i(t*);  at a kink, where a second face f2 is co-active,
    lam1 = g_f2' / (g_f2' - g_f1'),  lam2 = 1 - lam1,   jac[c][i] = (lam1 a_f1[c] + lam2 a_f2[c]) B_i(t*).
Co-activity: f != f1 is co-active iff g_f'(t*) and g_f1'(t*) have opposite signs and
g_f1(t*) - g_f(t*) <= 2 tol (1 + |g_f'| / |g_f1'|); among several the largest g_f(t*); g_f1'(t*) == 0 is smooth.

Rounding allowance of a device value (value_allowance): the device's value at t* = k / 2^D is a face coefficient of a
control point that went through D de Casteljau splits of at most n levels each -- one rounding per level, each at most
2^-53 of the largest |coordinate| -- and then the coefficient's d fused multiply-adds, one rounding each: K = d + n D on
M = |b| + sum_c |a[c]| max_i |P[c][i]|, the convention of tests/constraint_rows_ref.py."""
import heapq
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

U53 = Fraction(1, 2 ** 53)


def fr(x):
    return x if isinstance(x, Fraction) else Fraction(float(x))


# ---------------------------------------------------------------------------------------------------------------------
#  (1) exact rationals
# ---------------------------------------------------------------------------------------------------------------------
def basis(n, t):
    """[n + 1] Fractions: B_i^n(t)"""
    t = fr(t)
    return [math.comb(n, i) * t ** i * (1 - t) ** (n - i) for i in range(n + 1)]


def face_coeffs(P, h):
    """[n + 1] Fractions: the Bernstein coefficients a . P_i - b of g_f for the face h = (a, b)"""
    P = np.asarray(P, dtype=np.float64)
    d = P.shape[0]
    return [sum(fr(h[c]) * fr(P[c, i]) for c in range(d)) - fr(h[d]) for i in range(P.shape[1])]


def g_at(P, h, t):
    c = face_coeffs(P, h)
    return sum(ci * w for ci, w in zip(c, basis(len(c) - 1, t)))


def dg_at(P, h, t):
    c = face_coeffs(P, h)
    n = len(c) - 1
    if n == 0:
        return Fraction(0)
    return n * sum((c[i + 1] - c[i]) * w for i, w in enumerate(basis(n - 1, t)))


def G_at(P, H, t):
    """(G(t), argmax face -- the first of equals)"""
    vals = [g_at(P, h, t) for h in np.asarray(H)]
    m = max(vals)
    return m, vals.index(m)


def active(P, H, t, tol):
    """(f1, f2, lam1) by the co-activity rule at t, everything exact; f2 = -1 and lam1 = 1 without a second face"""
    H = np.asarray(H, dtype=np.float64)
    t = fr(t)
    g = [g_at(P, h, t) for h in H]
    s = [dg_at(P, h, t) for h in H]
    f1 = g.index(max(g))
    if t == 0 or t == 1 or s[f1] == 0:
        return f1, -1, Fraction(1)
    best = None
    for f in range(len(g)):
        if f == f1 or s[f] * s[f1] >= 0:
            continue
        if g[f1] - g[f] <= 2 * fr(tol) * (1 + abs(s[f]) / abs(s[f1])) and (best is None or g[f] > g[best]):
            best = f
    if best is None:
        return f1, -1, Fraction(1)
    return f1, best, s[best] / (s[best] - s[f1])


def lam_at(P, H, t, f1, f2):
    """the exact weight of f1 at t for the pair (f1, f2); 1 without a second face"""
    if f2 < 0:
        return Fraction(1)
    H = np.asarray(H, dtype=np.float64)
    s1, s2 = dg_at(P, H[f1], t), dg_at(P, H[f2], t)
    return s2 / (s2 - s1)


def block(H, n, t, f1, f2, lam1):
    """[d][n + 1] Fractions: (lam1 a_f1[c] + (1 - lam1) a_f2[c]) B_i^n(t); f2 < 0: a_f1[c] B_i^n(t)"""
    H = np.asarray(H, dtype=np.float64)
    d = H.shape[1] - 1
    w = basis(n, t)
    lam1 = fr(lam1)
    a = [fr(H[f1, c]) if f2 < 0 else lam1 * fr(H[f1, c]) + (1 - lam1) * fr(H[f2, c]) for c in range(d)]
    return [[a[c] * w[i] for i in range(n + 1)] for c in range(d)]


def block_float(H, n, t, f1, f2, lam1):
    return np.array([[float(x) for x in r] for r in block(H, n, t, f1, f2, lam1)])


def majorant(P, H):
    """max over the faces of |b| + sum_c |a[c]| max_i |P[c][i]|"""
    P, H = np.abs(np.asarray(P, dtype=np.float64)), np.abs(np.asarray(H, dtype=np.float64))
    return float((H[:, -1] + H[:, :-1] @ P.max(axis=1)).max())


def depth_of(t):
    """D with t = k / 2^D, k odd (0 for t in {0, 1})"""
    q = fr(t).denominator
    return q.bit_length() - 1


def value_allowance(P, H, t):
    """K 2^-53 M of a device value at the dyadic t (module docstring): K = d + n D"""
    P = np.asarray(P)
    return (P.shape[0] + (P.shape[1] - 1) * depth_of(t)) * 2.0 ** -53 * majorant(P, H)


# ---------------------------------------------------------------------------------------------------------------------
#  (2) a float64 branch and bound, best-first
# ---------------------------------------------------------------------------------------------------------------------
def _split(Q):
    """de Casteljau at 1/2 of the rows of Q[d][K]: (left, right)"""
    K = Q.shape[1]
    L, R = np.empty_like(Q), np.empty_like(Q)
    w = Q.copy()
    for r in range(K):
        L[:, r] = w[:, 0]
        R[:, K - 1 - r] = w[:, K - 1 - r]
        w = 0.5 * w[:, :-1] + 0.5 * w[:, 1:]
    return L, R


def search(P, H, eps_rel=1e-12, max_nodes=100000):
    """dict(val, t, bound, nodes, s, tol, ok): the least of G over [0, 1] within tol = eps_rel s, s = max |g_f,i| of the root:
    bound <= min G <= val, val - bound <= tol when ok.  A non-finite input: NaNs."""
    P, H = np.asarray(P, dtype=np.float64), np.asarray(H, dtype=np.float64)
    A, b = H[:, :-1], H[:, -1]

    def coef(Q):
        return A @ Q - b[:, None]

    with np.errstate(all="ignore"):
        g = coef(P)
    if not np.isfinite(g).all():
        return dict(val=np.nan, t=np.nan, bound=np.nan, nodes=0, s=np.nan, tol=np.nan, ok=True)
    s = float(np.abs(g).max())
    tol = eps_rel * s
    G = g.max(axis=0)
    val, t = (float(G[0]), 0.0) if G[0] <= G[-1] else (float(G[-1]), 1.0)
    heap = [(float(g.min(axis=1).max()), 0.0, 1.0, 0, P)]
    nodes, tick, bound, ok = 1, 0, math.inf, True
    while heap:
        lb, t0, w, _, Q = heapq.heappop(heap)
        if val - lb <= tol:                       # the smallest bound left: everything else closes too
            bound = lb
            break
        if nodes + 2 > max_nodes:
            bound, ok = lb, False
            break
        L, R = _split(Q)
        nodes += 2
        tm = t0 + 0.5 * w
        gm = float(coef(L[:, -1:]).max())
        if gm < val:
            val, t = gm, tm
        for C, c0 in ((L, t0), (R, tm)):
            tick += 1
            heapq.heappush(heap, (float(coef(C).min(axis=1).max()), c0, 0.5 * w, tick, C))
    return dict(val=val, t=t, bound=min(bound, val), nodes=nodes, s=s, tol=tol, ok=ok)


def row(P, H, eps_rel=1e-12, margin=0.0):
    """dict(val, t, f1, f2, lam, jac[d][n + 1], s, tol): the row, its active faces by the exact rule at the search's t, and
    the exact block rounded once"""
    P = np.asarray(P, dtype=np.float64)
    r = search(P, H, eps_rel)
    f1, f2, lam = active(P, H, r["t"], r["tol"])
    return dict(val=r["val"] - margin, t=r["t"], f1=f1, f2=f2, lam=float(lam), s=r["s"], tol=r["tol"],
                jac=block_float(H, P.shape[1] - 1, r["t"], f1, f2, lam))


def G_samples(P, H, m=2001):
    """(t[m], G[m]) in float64: G on a uniform grid, by the Bernstein basis"""
    P, H = np.asarray(P, dtype=np.float64), np.asarray(H, dtype=np.float64)
    n = P.shape[1] - 1
    t = np.linspace(0.0, 1.0, m)
    Bm = np.array([math.comb(n, i) * t ** i * (1 - t) ** (n - i) for i in range(n + 1)])      # [n + 1][m]
    return t, ((H[:, :-1] @ P - H[:, -1:]) @ Bm).max(axis=0)


def report(P, H, eps_rel=1e-12, m=2001):
    """dict(kind, generic, why): kind of the item's minimiser -- 'end', 'kink' or 'smooth' -- with `penetrating` (val < 0);
    generic: False when the envelope derivative is not defined well enough to be compared -- a second local minimum of G
    within 1e-3 of the first, three faces within 1e-6 of G at t*, or a kink with a slope below 1e-6."""
    r = row(P, H, eps_rel)
    H = np.asarray(H, dtype=np.float64)
    kind = "end" if r["t"] in (0.0, 1.0) else ("kink" if r["f2"] >= 0 else "smooth")
    why = []
    t, G = G_samples(P, H, m)
    pad = np.concatenate(([np.inf], G, [np.inf]))
    loc = np.sort(G[(pad[1:-1] <= pad[:-2]) & (pad[1:-1] <= pad[2:])])
    if loc.size > 1 and loc[1] - loc[0] <= 1e-3:
        why.append("second local minimum")
    gt = [float(g_at(P, h, r["t"])) for h in H]
    if sum(1 for x in gt if max(gt) - x <= 1e-6) >= 3:
        why.append("three faces")
    if kind == "kink" and min(abs(float(dg_at(P, H[f], r["t"]))) for f in (r["f1"], r["f2"])) < 1e-6:
        why.append("flat kink")
    return dict(kind=kind, penetrating=r["val"] < 0.0, generic=not why, why=why, row=r)


def forward_difference(P, H, h=1e-6, eps_rel=1e-12):
    """[d][n + 1]: (row(P + h e_ci) - row(P)) / ((P_ci + h) - P_ci), the difference quotient of the searched value"""
    P = np.asarray(P, dtype=np.float64)
    v0 = search(P, H, eps_rel)["val"]
    out = np.zeros_like(P)
    for c in range(P.shape[0]):
        for i in range(P.shape[1]):
            Q = P.copy()
            Q[c, i] += h
            out[c, i] = (search(Q, H, eps_rel)["val"] - v0) / (Q[c, i] - P[c, i])
    return out


# ---------------------------------------------------------------------------------------------------------------------
#  obstacles and inputs the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
def unit_square():
    """|x|, |y| <= 1: faces x <= 1, y <= 1, -x <= 1, -y <= 1"""
    return np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]]), np.ones(4)


def oblique_triangle():
    """the triangle (2, -1), (4, 0.5), (2.5, 2), unit normals"""
    from optimalbeziertrajectorygeneration_amd.bezier import halfspacesOfPolygon
    return halfspacesOfPolygon([(2.0, -1.0), (4.0, 0.5), (2.5, 2.0)])


def box3():
    """|x| <= 1, |y| <= 0.75, |z| <= 0.5"""
    A = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    return A, np.array([1.0, 1.0, 0.75, 0.75, 0.5, 0.5])


def tetrahedron():
    """the tetrahedron (2, 0, 0), (4, 0, 0), (3, 2, 0), (3, 0.5, 2), unit outward normals"""
    V = np.array([(2.0, 0.0, 0.0), (4.0, 0.0, 0.0), (3.0, 2.0, 0.0), (3.0, 0.5, 2.0)])
    cen = V.mean(axis=0)
    A, b = [], []
    for k in range(4):
        q = np.delete(V, k, axis=0)
        nrm = np.cross(q[1] - q[0], q[2] - q[0])
        nrm /= np.linalg.norm(nrm)
        if nrm @ (cen - q[0]) > 0:
            nrm = -nrm
        A.append(nrm)
        b.append(nrm @ q[0])
    return np.array(A), np.array(b)


def obstacles(dim):
    return [unit_square(), oblique_triangle()] if dim == 2 else [box3(), tetrahedron()]


def tables(obs, n_veh):
    """(H, obs_off, VO): the tables BezOptimization makes of the list `obs` -- every vehicle against every obstacle,
    vehicle-major"""
    H = np.vstack([np.hstack((np.asarray(A, dtype=float), np.asarray(b, dtype=float)[:, None])) for A, b in obs])
    off = np.cumsum([0] + [len(b) for _, b in obs]).astype(np.int32)
    O = len(obs)
    VO = np.stack((np.repeat(np.arange(n_veh), O), np.tile(np.arange(O), n_veh)), axis=1).astype(np.int32)
    return H, off, VO


def batch(deg, dim, seed, n_veh=3, B=5):
    """Y[B][n_veh * dim][deg + 1]: random control points in a box around the two obstacles -- first and last point drawn
    wider than the inner ones, so that curves pass by, graze and cross the obstacles -- and, in the last row, the last
    vehicle moved 40 away (the far item)."""
    rng = np.random.default_rng(seed)
    Y = rng.uniform(-1.5, 3.5, size=(B, n_veh, dim, deg + 1))
    Y[..., 0] = rng.uniform(-3.0, 5.0, size=(B, n_veh, dim))
    Y[..., -1] = rng.uniform(-3.0, 5.0, size=(B, n_veh, dim))
    Y[B - 1, n_veh - 1] += 40.0
    return np.ascontiguousarray(Y.reshape(B, n_veh * dim, deg + 1))
