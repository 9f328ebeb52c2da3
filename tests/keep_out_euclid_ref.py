"""The yardstick of the Euclidean keep-out rows and their envelope Jacobian (obtg_keep_out_euclid_true_min[_jac],
obtg_bern_keep_out_euclid, obtg_keep_out_features).  No device, no reference code.

An obstacle is a convex set {p : a_f . p <= b_f}.  The rows work on NORMALISED faces a^ = a / |a|, b^ = b / |a| (`normalise`),
taken from there on as the float64 values they are.  With g_f(p) = a^_f . p - b^_f the signed distance is

    D(p) = max_f g_f(p)                                 when that is <= 0           (inside: minus the depth)
    D(p) = max over S of sqrt(g_S^T Gram_S^-1 g_S)      otherwise,

S running over the single faces (value g_f) and over the obstacle's FEATURES whose multipliers mu = Gram_S^-1 g_S are all >= 0
(Gram_S = A^_S A^_S^T, lambda = mu / value).  Every such (S, lambda) is dual feasible, so every candidate is a lower bound of
the distance and the largest is the distance.  Features (`features`): d = 2, a pair of non-parallel faces whose intersection
point satisfies every other face; d = 3, an edge -- a pair of non-parallel faces whose common line, clipped by the other
faces, is not empty -- or a vertex -- a triple with a non-singular Gram matrix whose point satisfies every other face.  The
tests are tolerant, <= 1e-9 (1 + |b^|), so they include rather than exclude; pairs first, then triples, each lexicographic.

Four things live here.  (1) The features by those rules.  (2) D^2, the multipliers and the unit direction at a point in EXACT
rationals (a float64 is a dyadic rational), the square root by `decimal` at 60 digits; `D_exact_subsets` is the same maximum
over ALL subsets of up to d faces.  (3) A float64 branch and bound of its own (`search`, best-first on a heap -- not the
device's depth-first order) with the bound of a sub-curve

    max( max_f min_i g_f,i ,  min_i (u . P_i - beta) ),

(u, beta) = (A^T lambda, lambda . b^) the maximiser at the point the sub-curve was split off at (both ends for the root):
D(p) >= u . p - beta for every p and every dual-feasible pair.  (4) The block jac[c][i] = dir[c] B_i^n(t*): dir the unit
vector from the projection to c(t*) outside, and what the faces rule (tests/keep_out_ref.py `active`) gives inside.

Rounding allowance of a device value at t* = k / 2^D (`value_allowance`), K 2^-53 M with M the faces' majorant
|b^| + sum_c |a^[c]| max_i |P[c][i]|.  Count the operations:
  * the control point went through D de Casteljau splits of at most n levels each, one rounding per level, and a face
    coefficient adds d fused multiply-adds: every g_f carries at most e_g = (d + n D) 2^-53 M  (tests/keep_out_ref.py);
  * Gram^-1 g: m <= 3 roundings per multiplier, each at most 2^-53 c max|g| with c = max(1, the largest sum of |entries| of
    a feature's Gram^-1), so a multiplier carries c e_g + m 2^-53 c M;
  * the dot product q = g . mu: m more roundings, and both factors' errors: dq <= 2 m c M (e_g + m 2^-53 M);
  * the root: D = sqrt(q) >= max|g| / sqrt(m) (Gram's largest eigenvalue is at most m), so dD = dq / (2 D) <= sqrt(3) m c
    (e_g + m 2^-53 M) <= 5.2 c (d + n D + 3) 2^-53 M, and the root's own rounding, at most 2^-53 sqrt(m c) M;
  * the table: Gram^-1 itself comes from the host with a relative error of a few 2^-53 times its conditioning (the features
    test holds it to 16 c 2^-53): dq <= m M^2 16 c^2 2^-53, i.e. dD <= 24 c^2 2^-53 M.
Together K = 6 c (d + n D + 4) + 24 c^2.  A direction is ill-conditioned as 1 / D: its allowance is the value's divided by D."""
import heapq
import itertools
import math
import os
import sys
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_out_ref as faces_ref  # noqa: E402

getcontext().prec = 60
TOL_FACE, DET_MIN, MAX_FEATURES = 1e-9, 1e-12, 128


def fr(x):
    return x if isinstance(x, Fraction) else Fraction(float(x))


# ---------------------------------------------------------------------------------------------------------------------
#  (1) normalised faces and features
# ---------------------------------------------------------------------------------------------------------------------
def normalise(H):
    """Hn[F][d + 1] = (a / |a|, b / |a|); |a| = 1 leaves the face bit for bit, |a| = 0 gives NaN"""
    H = np.asarray(H, dtype=np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt((H[:, :-1] ** 2).sum(axis=1))
        return H / n[:, None]


def _admits(Hn, p, skip):
    return all(Hn[m, :-1] @ p - Hn[m, -1] <= TOL_FACE * (1.0 + abs(Hn[m, -1])) for m in range(len(Hn)) if m not in skip)


def features(Hn):
    """[(faces tuple, Gram^-1 as an m x m float64 array)] by the module docstring's rules, in table order"""
    Hn = np.asarray(Hn, dtype=np.float64)
    F, d = Hn.shape[0], Hn.shape[1] - 1
    if not np.isfinite(Hn).all():
        return []
    out = []
    for S in itertools.combinations(range(F), 2):
        A, b = Hn[list(S), :-1], Hn[list(S), -1]
        G = A @ A.T
        if not np.linalg.det(G) > DET_MIN:
            continue
        Gi = np.linalg.inv(G)
        p = A.T @ (Gi @ b)
        if d == 2:
            ok = _admits(Hn, p, S)
        else:
            v = np.cross(A[0], A[1])
            lo, hi, ok = -math.inf, math.inf, True
            for m in range(F):
                if m in S:
                    continue
                s = Hn[m, :-1] @ v
                r = TOL_FACE * (1.0 + abs(Hn[m, -1])) - (Hn[m, :-1] @ p - Hn[m, -1])
                if abs(s) <= DET_MIN:
                    ok = ok and r >= 0.0
                elif s > 0:
                    hi = min(hi, r / s)
                else:
                    lo = max(lo, r / s)
            ok = ok and lo <= hi
        if ok:
            out.append((S, Gi))
    if d == 3:
        for S in itertools.combinations(range(F), 3):
            A, b = Hn[list(S), :-1], Hn[list(S), -1]
            G = A @ A.T
            if not np.linalg.det(G) > DET_MIN:
                continue
            Gi = np.linalg.inv(G)
            if _admits(Hn, A.T @ (Gi @ b), S):
                out.append((S, Gi))
    return out


def gram_inverse_exact(Hn, S):
    """Gram_S^-1 of the float64 faces in exact rationals: an m x m list of Fractions"""
    key = (np.asarray(Hn, dtype=np.float64)[list(S), :-1].tobytes(), len(S))
    if key not in _gram_cache:
        A = [[fr(x) for x in Hn[f][:-1]] for f in S]
        m = len(S)
        _gram_cache[key] = _inverse([[sum(x * y for x, y in zip(A[i], A[j])) for j in range(m)] for i in range(m)])
    return _gram_cache[key]


_gram_cache = {}


def _inverse(G):
    m = len(G)
    M = [list(r) + [Fraction(int(i == j)) for j in range(m)] for i, r in enumerate(G)]
    for i in range(m):
        piv = next(r for r in range(i, m) if M[r][i] != 0)
        M[i], M[piv] = M[piv], M[i]
        M[i] = [x / M[i][i] for x in M[i]]
        for r in range(m):
            if r != i and M[r][i] != 0:
                M[r] = [x - M[r][i] * y for x, y in zip(M[r], M[i])]
    return [r[m:] for r in M]


def conditioning(feats):
    """c of the module docstring: max(1, the largest sum of |entries| of a feature's Gram^-1)"""
    return max([1.0] + [float(np.abs(Gi).sum()) for _, Gi in feats])


# ---------------------------------------------------------------------------------------------------------------------
#  (2) the signed distance in exact rationals
# ---------------------------------------------------------------------------------------------------------------------
def _sqrt(q):
    """sqrt of a non-negative Fraction as a Decimal at the context's 60 digits"""
    return (Decimal(q.numerator) / Decimal(q.denominator)).sqrt()


def _candidate(Hn, S, g):
    """(q, mu) of the set S at the face values g, or None when a multiplier is negative"""
    if len(S) == 1:
        return (g[S[0]] ** 2, [g[S[0]]]) if g[S[0]] > 0 else None
    try:
        Gi = gram_inverse_exact(Hn, S)
    except StopIteration:
        return None
    mu = [sum(Gi[i][j] * g[S[j]] for j in range(len(S))) for i in range(len(S))]
    if min(mu) < 0:
        return None
    return sum(m * g[f] for m, f in zip(mu, S)), mu


def D_exact(Hn, p, sets=None):
    """dict(D -- float, the exact value rounded once --, D2 -- Fraction, None inside --, S, mu, dir[d] float, inside): the
    signed distance at p on the float64 faces Hn; sets: the features' face tuples (default: `features(Hn)`)"""
    Hn = np.asarray(Hn, dtype=np.float64)
    d = Hn.shape[1] - 1
    pf = [fr(x) for x in p]
    g = [sum(fr(Hn[f, c]) * pf[c] for c in range(d)) - fr(Hn[f, d]) for f in range(len(Hn))]
    gmax = max(g)
    if gmax <= 0:
        f1 = g.index(gmax)
        return dict(D=float(gmax), D2=None, S=(f1,), mu=[Fraction(1)], dir=np.array(Hn[f1, :-1]), inside=True)
    if sets is None:
        sets = [S for S, _ in features(Hn)]
    best = None
    for S in [(f,) for f in range(len(Hn))] + list(sets):
        r = _candidate(Hn, S, g)
        if r is not None and (best is None or r[0] > best[0]):
            best = (r[0], S, r[1])
    q, S, mu = best
    root = _sqrt(q)
    u = [sum(m * fr(Hn[f, c]) for m, f in zip(mu, S)) for c in range(d)]
    dirv = np.array([float(Decimal(x.numerator) / Decimal(x.denominator) / root) for x in u])
    return dict(D=float(root), D2=q, S=tuple(S), mu=mu, dir=dirv, inside=False)


def D_exact_subsets(Hn, p):
    """the same maximum over ALL subsets of up to d faces (dual feasibility needs no feature test)"""
    Hn = np.asarray(Hn, dtype=np.float64)
    d = Hn.shape[1] - 1
    sets = [S for m in range(2, d + 1) for S in itertools.combinations(range(len(Hn)), m)]
    return D_exact(Hn, p, sets)


def curve_point(P, t):
    """c(t) in exact rationals: [d] Fractions"""
    P = np.asarray(P, dtype=np.float64)
    w = faces_ref.basis(P.shape[1] - 1, t)
    return [sum(fr(P[c, i]) * w[i] for i in range(P.shape[1])) for c in range(P.shape[0])]


def curve_tangent(P, t):
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[1] - 1
    w = faces_ref.basis(n - 1, t) if n else []
    return [n * sum((fr(P[c, i + 1]) - fr(P[c, i])) * w[i] for i in range(n)) for c in range(P.shape[0])]


# ---------------------------------------------------------------------------------------------------------------------
#  (3) float64: the distance at a point with its dual pair, and a best-first branch and bound
# ---------------------------------------------------------------------------------------------------------------------
class _Packed:
    """the features of one table grouped by size, for D_float: faces [k][m], Gram^-1 [k][m][m], position in the table [k]"""

    def __init__(self, feats):
        self.groups = []
        for m in (2, 3):
            sel = [k for k, (S, _) in enumerate(feats) if len(S) == m]
            if sel:
                self.groups.append((np.array([feats[k][0] for k in sel]), np.array([feats[k][1] for k in sel]), np.array(sel)))


_packed = {}


def D_float(Hn, feats, p):
    """(D, u[d], beta, S) in float64, candidates in table order, the first of equals; inside: the first largest face"""
    g = Hn[:, :-1] @ p - Hn[:, -1]
    f1 = int(np.argmax(g))
    best = (float(g[f1]), Hn[f1, :-1], float(Hn[f1, -1]), (f1,))
    if g[f1] <= 0.0 or not feats:
        return best
    pk = _packed.get(id(feats))
    if pk is None or pk[0] is not feats:
        pk = _packed[id(feats)] = (feats, _Packed(feats))
    top = None
    for idx, Gi, pos in pk[1].groups:
        gs = g[idx]                                        # [k][m]
        mu = np.einsum("kij,kj->ki", Gi, gs)
        q = (gs * mu).sum(axis=1)
        v = np.where((mu >= 0.0).all(axis=1) & (q > 0.0), np.sqrt(np.maximum(q, 0.0)), -np.inf)
        k = int(np.argmax(v))
        if v[k] > best[0] and (top is None or v[k] > top[0] or (v[k] == top[0] and pos[k] < top[1])):
            top = (float(v[k]), int(pos[k]), mu[k])
    if top is not None:
        S = feats[top[1]][0]
        lam = top[2] / top[0]
        best = (top[0], lam @ Hn[list(S), :-1], float(lam @ Hn[list(S), -1]), tuple(S))
    return best


def search(P, Hn, feats=None, eps_rel=1e-12, max_nodes=100000):
    """dict(val, t, bound, nodes, s, tol, ok): the least of D(c(t)) over [0, 1] within tol = eps_rel s, s = max |g_f,i| of the
    root: bound <= min D <= val, val - bound <= tol when ok.  A non-finite input: NaNs."""
    P, Hn = np.asarray(P, dtype=np.float64), np.asarray(Hn, dtype=np.float64)
    if feats is None:
        feats = features(Hn)
    A, b = Hn[:, :-1], Hn[:, -1]

    def lower(Q, duals):
        lb = float((A @ Q - b[:, None]).min(axis=1).max())
        for u, beta in duals:
            lb = max(lb, float((u @ Q - beta).min()))
        return lb

    with np.errstate(all="ignore"):
        g = A @ P - b[:, None]
    if not np.isfinite(g).all():
        return dict(val=np.nan, t=np.nan, bound=np.nan, nodes=0, s=np.nan, tol=np.nan, ok=True)
    s = float(np.abs(g).max())
    tol = eps_rel * s
    e0, e1 = D_float(Hn, feats, P[:, 0]), D_float(Hn, feats, P[:, -1])
    val, t = (e0[0], 0.0) if e0[0] <= e1[0] else (e1[0], 1.0)
    heap = [(lower(P, [e0[1:3], e1[1:3]]), 0.0, 1.0, 0, P)]
    nodes, tick, bound, ok = 1, 0, math.inf, True
    while heap:
        lb, t0, w, _, Q = heapq.heappop(heap)
        if val - lb <= tol:
            bound = lb
            break
        if nodes + 2 > max_nodes:
            bound, ok = lb, False
            break
        L, R = faces_ref._split(Q)
        nodes += 2
        tm = t0 + 0.5 * w
        em = D_float(Hn, feats, L[:, -1])
        if em[0] < val:
            val, t = em[0], tm
        for C, c0 in ((L, t0), (R, tm)):
            tick += 1
            heapq.heappush(heap, (lower(C, [em[1:3]]), c0, 0.5 * w, tick, C))
    return dict(val=val, t=t, bound=min(bound, val), nodes=nodes, s=s, tol=tol, ok=ok)


def faces_search(P, Hn, eps_rel=1e-12):
    """the faces metric's row on the same (normalised) faces: tests/keep_out_ref.py search"""
    return faces_ref.search(P, Hn, eps_rel)


def D_samples(P, Hn, feats, m=2001):
    """(t[m], D[m]) in float64 on a uniform grid"""
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[1] - 1
    t = np.linspace(0.0, 1.0, m)
    Bm = np.array([math.comb(n, i) * t ** i * (1 - t) ** (n - i) for i in range(n + 1)])
    pts = P @ Bm
    return t, np.array([D_float(Hn, feats, pts[:, k])[0] for k in range(m)])


# ---------------------------------------------------------------------------------------------------------------------
#  (4) the block
# ---------------------------------------------------------------------------------------------------------------------
def direction(P, Hn, t, tol, sets=None):
    """(dir[d] float, faces tuple): outside, the exact unit gradient of D at c(t); inside, the faces rule's
    lam1 a^_f1 + lam2 a^_f2 (tests/keep_out_ref.py active) on the normalised faces"""
    Hn = np.asarray(Hn, dtype=np.float64)
    r = D_exact(Hn, curve_point(P, t), sets)
    if not r["inside"]:
        return r["dir"], r["S"]
    f1, f2, lam = faces_ref.active(P, Hn, t, tol)
    d = Hn.shape[1] - 1
    a = [fr(Hn[f1, c]) if f2 < 0 else lam * fr(Hn[f1, c]) + (1 - lam) * fr(Hn[f2, c]) for c in range(d)]
    return np.array([float(x) for x in a]), (f1,) if f2 < 0 else (f1, f2)


def block(P, Hn, t, tol, sets=None):
    """[d][n + 1] float64: dir[c] B_i^n(t)"""
    n = np.asarray(P).shape[1] - 1
    dirv, _ = direction(P, Hn, t, tol, sets)
    w = np.array([float(x) for x in faces_ref.basis(n, t)])
    return dirv[:, None] * w[None, :]


def forward_difference(P, Hn, feats, h=1e-6, eps_rel=1e-12):
    """[d][n + 1]: the difference quotient of the searched row"""
    P = np.asarray(P, dtype=np.float64)
    v0 = search(P, Hn, feats, eps_rel)["val"]
    out = np.zeros_like(P)
    for c in range(P.shape[0]):
        for i in range(P.shape[1]):
            Q = P.copy()
            Q[c, i] += h
            out[c, i] = (search(Q, Hn, feats, eps_rel)["val"] - v0) / (Q[c, i] - P[c, i])
    return out


def value_allowance(P, Hn, t, feats=None):
    """K 2^-53 M of a device value at the dyadic t (module docstring): K = 6 c (d + n D + 4) + 24 c^2"""
    P = np.asarray(P)
    if feats is None:
        feats = features(Hn)
    c = conditioning(feats)
    K = 6.0 * c * (P.shape[0] + (P.shape[1] - 1) * faces_ref.depth_of(t) + 4) + 24.0 * c * c
    return K * 2.0 ** -53 * faces_ref.majorant(P, Hn)


# ---------------------------------------------------------------------------------------------------------------------
#  obstacles (unit inradius) and curves the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
def _regular(k, phase):
    th = phase + 2.0 * math.pi * np.arange(k) / k
    return np.column_stack((np.cos(th), np.sin(th), np.ones(k)))


def square():
    return np.array([[1.0, 0, 1], [0, 1.0, 1], [-1.0, 0, 1], [0, -1.0, 1]])


def triangle():
    return _regular(3, 0.3)          # irrational normals


def hexagon():
    return _regular(6, 0.2)


def slab():
    return np.array([[0.0, 1.0, 1.0], [0.0, -1.0, 1.0]])


def half_space(d=2):
    return np.array([[1.0] + [0.0] * (d - 1) + [1.0]])


def box():
    return np.array([[1.0, 0, 0, 1], [-1.0, 0, 0, 1], [0, 1.0, 0, 1], [0, -1.0, 0, 1], [0, 0, 1.0, 1], [0, 0, -1.0, 1]])


def tetrahedron():
    A = np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / math.sqrt(3.0)
    return np.column_stack((A, np.ones(4)))


def octahedron():
    A = np.array([[sx, sy, sz] for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]) / math.sqrt(3.0)
    return np.column_stack((A, np.ones(8)))


def wedge():
    """x +- y <= 0 in 3-D: one edge (the z axis), no vertex"""
    return np.array([[1.0, 1.0, 0.0, 0.0], [1.0, -1.0, 0.0, 0.0]])


def scaled_square():
    return square() * np.array([2.0, 0.5, 3.0, 7.0])[:, None]


OBSTACLES = dict(square=square, triangle=triangle, hexagon=hexagon, slab=slab, half_space=half_space, box=box,
                 tetrahedron=tetrahedron, octahedron=octahedron, wedge=wedge, scaled_square=scaled_square)
CORNERED = ("square", "hexagon", "triangle", "box", "octahedron", "tetrahedron")
FEATURE_COUNTS = dict(square=4, slab=0, box=20, octahedron=48, tetrahedron=10, wedge=1)


def curves(deg, dim, seed, M=30):
    """c[M][dim][deg + 1]: control point i at angle th0 + span i / n in a random plane through the origin (2-D: the plane
    itself), th0 uniform in [0, 2 pi), span in [0.6, 3.5], the radius in [1.5, 3.2]"""
    rng = np.random.default_rng(seed)
    out = np.empty((M, dim, deg + 1))
    for m in range(M):
        th0, span, rad = rng.uniform(0.0, 2.0 * math.pi), rng.uniform(0.6, 3.5), rng.uniform(1.5, 3.2)
        th = th0 + span * np.arange(deg + 1) / deg
        if dim == 2:
            e1, e2 = np.array([1.0, 0.0]), np.array([0.0, 1.0])
        else:
            q, _ = np.linalg.qr(rng.normal(size=(3, 2)))
            e1, e2 = q[:, 0], q[:, 1]
        out[m] = rad * (np.outer(e1, np.cos(th)) + np.outer(e2, np.sin(th)))
    return out
