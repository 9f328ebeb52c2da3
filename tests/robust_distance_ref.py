"""Exact-rational yardsticks for the robust distance searches (obtg_gjk_true_pairs, obtg_min_dist_robust,
obtg_min_dist2poly_robust).  Everything is fractions.Fraction on the float inputs converted exactly; nothing here shares code
with the kernels or with csrc/gjk_true.h.

  hull_dist_sq(P, Q)                 exact squared distance of two convex hulls, with closest points and weights
  curve_dist_sq_bracket(A, B, ...)   lo <= min |A(s) - B(t)|^2 <= hi by subdivision of the tensor-Bernstein form
  curve_poly_dist_sq_bracket(...)    the same for a curve against the hull of a few points, for the certified kinds of case
  eval_curve(A, t)                   exact de Casteljau
  sqrt_up / sqrt_dn, within          helpers for comparisons made on squares
"""
import heapq
import itertools
from fractions import Fraction as Fr
from math import comb, isqrt


def frac_points(P):
    """rows of points -> tuples of Fractions (floats convert exactly)"""
    return [tuple(Fr(x) for x in p) for p in P]


def frac_curve(A):
    """A[dim][K] -> list of K points"""
    return [tuple(Fr(A[q][i]) for q in range(len(A))) for i in range(len(A[0]))]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _solve(M, r):
    """M u = r by Gaussian elimination in rationals; None when M is singular"""
    n = len(M)
    M = [list(row) + [r[i]] for i, row in enumerate(M)]
    for c in range(n):
        piv = next((i for i in range(c, n) if M[i][c] != 0), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        inv = 1 / M[c][c]
        M[c] = [x * inv for x in M[c]]
        for i in range(n):
            if i != c and M[i][c] != 0:
                f = M[i][c]
                M[i] = [x - f * y for x, y in zip(M[i], M[c])]
    return [M[i][n] for i in range(n)]


def hull_dist_sq(P, Q):
    """(d2, c1, c2, w1, w2): the exact squared distance between conv(P) and conv(Q), a closest pair of points and their
    barycentric weights over P and Q.  For every pair of sub-simplices S1 of P, S2 of Q with |S1| + |S2| <= dim + 2 whose
    joint system is regular, the least distance of the two AFFINE hulls is found from the normal equations; a solution with
    all weights >= 0 is a distance between hull points, and an optimal pair of weight vectors that is a vertex of the optimal
    set has at most dim + 2 non-zeros with independent columns (Caratheodory), so the optimum is among the kept values."""
    P, Q = frac_points(P), frac_points(Q)
    dim = len(P[0])
    best = None
    for k1 in range(1, min(len(P), dim + 1) + 1):
        for k2 in range(1, min(len(Q), dim + 2 - k1) + 1):
            for S1 in itertools.combinations(range(len(P)), k1):
                cols1 = [_sub(P[i], P[S1[0]]) for i in S1[1:]]
                for S2 in itertools.combinations(range(len(Q)), k2):
                    cols = cols1 + [_sub(Q[S2[0]], Q[j]) for j in S2[1:]]
                    r0 = _sub(P[S1[0]], Q[S2[0]])
                    if cols:
                        u = _solve([[_dot(a, b) for b in cols] for a in cols], [-_dot(a, r0) for a in cols])
                        if u is None:
                            continue
                    else:
                        u = []
                    a = [1 - sum(u[:k1 - 1])] + u[:k1 - 1]
                    b = [1 - sum(u[k1 - 1:])] + u[k1 - 1:]
                    if min(a) < 0 or min(b) < 0:
                        continue
                    v = tuple(r0[q] + sum(u[c] * cols[c][q] for c in range(len(cols))) for q in range(dim))
                    d2 = _dot(v, v)
                    if best is None or d2 < best[0]:
                        best = (d2, S1, a, S2, b)
    d2, S1, a, S2, b = best
    w1, w2 = [Fr(0)] * len(P), [Fr(0)] * len(Q)
    for i, w in zip(S1, a):
        w1[i] = w
    for j, w in zip(S2, b):
        w2[j] = w
    c1 = tuple(sum(w1[i] * P[i][q] for i in range(len(P))) for q in range(dim))
    c2 = tuple(sum(w2[j] * Q[j][q] for j in range(len(Q))) for q in range(dim))
    return d2, c1, c2, w1, w2


def eval_curve(A, t):
    """A[dim][K] at the float (or Fraction) t, exactly"""
    t = Fr(t)
    out = []
    for row in A:
        b = [Fr(x) for x in row]
        while len(b) > 1:
            b = [(1 - t) * x + t * y for x, y in zip(b, b[1:])]
        out.append(b[0])
    return tuple(out)


def dist_sq_at(A, s, B, t):
    d = _sub(eval_curve(A, s), eval_curve(B, t))
    return _dot(d, d)


def _elev_matrix(n):
    """(2n + 1) x (n + 1): Bernstein degree n -> 2n"""
    return [[Fr(comb(n, i) * comb(n, k - i), comb(2 * n, k)) if 0 <= k - i <= n else Fr(0) for i in range(n + 1)]
            for k in range(2 * n + 1)]


def _square_coeffs(pts):
    """Bernstein coefficients (degree 2n) of |C(t)|^2 for the control points pts"""
    n = len(pts) - 1
    out = []
    for k in range(2 * n + 1):
        s = Fr(0)
        for i in range(max(0, k - n), min(n, k) + 1):
            s += comb(n, i) * comb(n, k - i) * _dot(pts[i], pts[k - i])
        out.append(s / comb(2 * n, k))
    return out


def dist_sq_tensor(A, B):
    """D[k][l], bidegree (2n, 2m): |A(s) - B(t)|^2 = |A|^2 + |B|^2 - 2 A . B in the tensor-Bernstein basis"""
    a, b = frac_curve(A), frac_curve(B)
    n, m = len(a) - 1, len(b) - 1
    na, nb = _square_coeffs(a), _square_coeffs(b)
    X = [[_dot(p, q) for q in b] for p in a]
    En, Em = _elev_matrix(n), _elev_matrix(m)
    XE = [[sum(En[k][i] * X[i][j] for i in range(n + 1) if En[k][i] != 0) for j in range(m + 1)] for k in range(2 * n + 1)]
    return [[na[k] + nb[l] - 2 * sum(Em[l][j] * XE[k][j] for j in range(m + 1) if Em[l][j] != 0) for l in range(2 * m + 1)]
            for k in range(2 * n + 1)]


def _halve(c):
    """de Casteljau at 1/2 of one coefficient list: (left, right)"""
    left, right = [c[0]], [c[-1]]
    while len(c) > 1:
        c = [(x + y) / 2 for x, y in zip(c, c[1:])]
        left.append(c[0])
        right.append(c[-1])
    return left, right[::-1]


def _quarter(D):
    """the children of a box: four, or two where one of the curves is a single point (one row or one column)"""
    if len(D[0]) == 1:
        left, right = _halve([r[0] for r in D])
        return [(0, 0, [[x] for x in left]), (1, 0, [[x] for x in right])]
    if len(D) == 1:
        left, right = _halve(D[0])
        return [(0, 0, [left]), (0, 1, [right])]
    rows = [_halve(r) for r in D]
    out = []
    for h in (0, 1):                       # t half
        cols = [_halve([rows[k][h][l] for k in range(len(D))]) for l in range(len(D[0]))]
        for g in (0, 1):                   # s half
            out.append((g, h, [[cols[l][g][k] for l in range(len(D[0]))] for k in range(len(D))]))
    return out


def _corners(D, s0, t0, w):
    return ((D[0][0], s0, t0), (D[0][-1], s0, t0 + w), (D[-1][0], s0 + w, t0), (D[-1][-1], s0 + w, t0 + w))


def curve_dist_sq_bracket(A, B, rel=Fr(1, 10 ** 12), floor=Fr(0), max_nodes=4000):
    """dict(lo, hi, at=(s, t), nodes) with lo <= min over [0, 1]^2 of |A(s) - B(t)|^2 <= hi = the value at `at`.  Best-first
    subdivision at mid-points: a box's lower bound is its least coefficient (convex hull property), the upper bound the least
    corner value met.  Ends when hi - lo <= rel * hi or hi <= floor."""
    A, B = [[list(C[q][:1]) for q in range(len(C))] if all(len(set(r)) == 1 for r in C) else C for C in (A, B)]   # a point-curve
    D = dist_sq_tensor(A, B)
    hi, at = min((v, (s, t)) for v, s, t in _corners(D, Fr(0), Fr(0), Fr(1)))
    heap = [(min(min(r) for r in D), hi, 0, Fr(0), Fr(0), Fr(1), D)]
    tick, nodes = 1, 1
    while True:
        lo = max(min(heap[0][0], hi), Fr(0)) if heap else hi       # (a squared distance is not negative: bounds below 0 count as 0)
        if hi - lo <= rel * hi or hi <= floor:
            return dict(lo=lo, hi=hi, at=at, nodes=nodes)
        if nodes > max_nodes:
            raise RuntimeError("curve_dist_sq_bracket: %d nodes without closing (hi %g, lo %g)" % (nodes, hi, lo))
        _, _, _, s0, t0, w, Dn = heapq.heappop(heap)
        h = w / 2
        for g, hh, Dc in _quarter(Dn):
            sc, tc = s0 + g * h, t0 + hh * h
            nodes += 1
            v, s, t = min(_corners(Dc, sc, tc, h))
            if v < hi:
                hi, at = v, (s, t)
            lb = min(min(r) for r in Dc)
            if lb < hi:
                heapq.heappush(heap, (max(lb, Fr(0)), v, tick, sc, tc, h, Dc))    # among equal bounds, the least corner first
                tick += 1
        if heap and heap[0][0] >= hi:                   # the least of them: no box left can hold a smaller value
            heap = []


def curve_poly_dist_sq_bracket(A, poly, kind, at=None, rel=Fr(1, 10 ** 12), floor=Fr(1, 10 ** 30)):
    """dict(lo, hi[, at]) for min_t dist(A(t), conv(poly))^2, for the three kinds of case the tests use, each certified here:
      'outside'  the curve does not meet the hull.  Its distance is then the distance to the hull's boundary, and the boundary
                 is among the segments between vertex pairs, all of which lie in the hull: the least bracket over those
                 segments (each a degree-1 curve).  Certificate: A(at) is outside, and lo > 0, so the curve never reaches
                 the boundary and cannot get in.  (A hull without interior in the curve's space, a point or a segment or
                 a planar polygon against a curve off its plane, needs no more than lo > 0.)
      'inside'   A(at) is in the hull (hull_dist_sq == 0): the answer is exactly 0.
      'above'    poly lies in z = 0, every z of the curve is the same h, and every control point's projection is in the
                 hull, hence the whole projected curve: the answer is exactly h^2."""
    poly = frac_points(poly)
    if kind == "inside":
        assert hull_dist_sq([eval_curve(A, at)], poly)[0] == 0
        return dict(lo=Fr(0), hi=Fr(0))
    if kind == "above":
        h = Fr(A[2][0])
        assert all(Fr(z) == h for z in A[2]) and all(p[2] == 0 for p in poly)
        assert all(hull_dist_sq([(c[0], c[1], Fr(0))], poly)[0] == 0 for c in frac_curve(A))
        return dict(lo=h * h, hi=h * h)
    assert kind == "outside" and hull_dist_sq([eval_curve(A, at)], poly)[0] > 0
    segs = list(itertools.combinations(range(len(poly)), 2)) or [(0, 0)]
    rooted = []
    for i, j in segs:
        E = [[poly[i][q], poly[j][q]] if i != j else [poly[i][q]] for q in range(3)]
        rooted.append((min(min(r) for r in dist_sq_tensor(A, E)), i, j, E))
    rooted.sort(key=lambda x: x[0])
    lo = hi = at_best = None
    for lb, i, j, E in rooted:
        if hi is not None and lb >= hi:
            continue                                    # this segment cannot hold the minimum: its own lo would be >= hi
        r = curve_dist_sq_bracket(A, E, rel=rel, floor=floor)          # (a curve that reaches a segment ends at the floor, lo 0)
        lo = r["lo"] if lo is None else min(lo, r["lo"])
        if hi is None or r["hi"] < hi:
            hi, at_best = r["hi"], r["at"][0]
    assert lo > 0
    return dict(lo=lo, hi=hi, at=at_best)


# ---- comparisons on squares
def sqrt_dn(x, bits=256):
    """a rational r with r <= sqrt(x) < r + 2^-bits-ish (relative), x >= 0"""
    x = Fr(x)
    if x <= 0:
        return Fr(0)
    sh = max(0, bits - (x.numerator.bit_length() - x.denominator.bit_length()) // 2)
    return Fr(isqrt((x.numerator << (2 * sh)) // x.denominator), 1 << sh)


def le_sqrt(x, h):
    """x <= sqrt(h) for rationals, h >= 0"""
    return x <= 0 or x * x <= h


def ge_sqrt(x, h):
    """x >= sqrt(h) for rationals"""
    return h <= 0 or (x >= 0 and x * x >= h)


def within(x, h, allow):
    """|x - sqrt(h)| <= allow"""
    return le_sqrt(x - allow, h) and ge_sqrt(x + allow, h)


def is_dyadic_unit(t):
    t = Fr(t)
    return 0 <= t <= 1 and (t.denominator & (t.denominator - 1)) == 0
