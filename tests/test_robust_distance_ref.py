"""The exact-rational yardsticks of tests/robust_distance_ref.py against closed forms, and the case lists that
tests/test_gpu_robust_distance.py and tests/test_true_gjk_host.py hold the robust searches to: built once in shared(...), and
shown here, without a device, to contain every kind of case they are meant to.  No device."""
import os
import sys
from fractions import Fraction as Fr
from math import lcm

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_distance_ref as R  # noqa: E402

U53 = Fr(1, 2 ** 53)
# control-point counts: any-count kernel / register kernels of obtg_min_dist_robust; obtg_min_dist2poly_robust
MDR_K = (2, 3, 5, 7, 4, 6, 11)
MD2R_K = (4, 5, 6)
# kinds of curve pair per K: crossing and touching pairs up to degree 5, four degree-10 pairs (the rational bracket's cost)
_ALL = ("generic3d", "c00", "c01", "c10", "c11", "edge_s0", "edge_t0", "crossing", "touch", "self", "parallel", "point", "far")
_NO_ZERO = tuple(k for k in _ALL if k not in ("crossing", "touch"))
MDR_KINDS = {2: _ALL, 3: _ALL, 4: _ALL, 5: _ALL, 6: _ALL, 7: _NO_ZERO, 11: ("generic3d", "c01", "edge_s0", "far")}
MD2R_CURVES = ("vertex", "edge", "end_inside", "middle_inside", "graze", "outside3d", "above")
MD2R_POLYS = ("poly3", "poly4", "poly5", "poly6", "one", "two", "two3d", "collinear")

# The rounding allowance between a reported distance and the exact value at the reported points, as a multiple of
# 2^-53 * scale (scale = the pair's largest absolute coordinate): four times the largest multiple measured on an MI355X over
# every case of the lists below, per kernel and control-point count (tests/test_gpu_robust_distance.py has the figures).
# Every one must stay below 1e-3 * eps * scale at eps = 1e-9, which is 9007 x 2^-53 scale.
MEASURED = {"gjk": 0.8431, "mdr": {2: 1.3928, 3: 1.5432, 5: 1.7567, 7: 2.2099, 4: 2.1003, 6: 2.0755, 11: 5.3325},
            "md2r": {4: 2.2620, 5: 1.6307, 6: 2.2668}}
ALLOW = {"gjk": 4 * Fr(MEASURED["gjk"]), "mdr": {K: 4 * Fr(v) for K, v in MEASURED["mdr"].items()},
         "md2r": {K: 4 * Fr(v) for K, v in MEASURED["md2r"].items()}}
ALLOW_CEILING = Fr(1, 10 ** 12) / U53

_shared = {}


# ------------------------------------------------------------------ (a) point sets
def _gjk_cases():
    rng = np.random.default_rng(41)
    out = []

    def add(kind, P, Q):
        out.append(dict(kind=kind, P=np.array(P, float).reshape(-1, 3), Q=np.array(Q, float).reshape(-1, 3)))

    def cloud(k, dim, shift=0.0):
        p = np.zeros((k, 3))
        p[:, :dim] = rng.uniform(-1, 1, (k, dim))
        p[:, 0] += shift
        return p
    sizes = [(1, 4), (2, 2), (3, 5), (4, 4), (6, 6), (5, 2)]
    for dim in (2, 3):
        for k1, k2 in sizes:
            add("separated%dd" % dim, cloud(k1, dim), cloud(k2, dim, 2.5))
        for k1, k2 in ((4, 3), (4, 6), (6, 5)):           # a vertex of Q well inside a simplex of P
            P, Q = cloud(k1, dim), cloud(k2, dim, 0.25)
            Q[0] = P[:dim + 1].mean(axis=0)
            add("overlapping%dd" % dim, P, Q)
    add("shared_vertex", [[0, 0, 0], [-1, 0.5, 0], [-1, -0.5, 0]], [[0, 0, 0], [1, 0.5, 0], [1, -0.75, 0]])
    add("shared_vertex", [[0, 0, 0], [-1, 0.5, 0.25], [-1, -0.5, 0], [-0.5, 0, 1]], [[0, 0, 0], [1, 0.5, 0], [1, -0.75, 0.5], [2, 0, -1]])
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], float)
    add("gap_2^-30", sq, sq + [1 + 2.0 ** -30, 0.25, 0])
    add("gap_2^-30", sq / 8, sq / 8 + [0.125 + 2.0 ** -30, 0.03125, 0])
    add("gap_2^-30", sq / 8 + [0, 0, 0.0625], np.array([[0.0625, 0.0625, 0.0625 + 2.0 ** -30], [0.0625, 0.03125, 0.125], [0, 0, 0.25], [0.125, 0.125, 0.25]]))
    add("points", [[0.25, -0.5, 0]], [[1.25, 0.25, 0]])
    add("points", [[0.25, -0.5, 0.125]], [[0.25, -0.5, 0.125]])
    add("points", [[0.5, 0.5, 2.0]], sq)
    add("points", cloud(5, 3), [[3.0, 0.1, -0.2]])
    add("collinear", [[0, 0, 0], [0.5, 0.5, 0], [1, 1, 0], [0.25, 0.25, 0]], [[2, 0, 0], [1.5, 0.5, 0], [1.75, 0.25, 0]])
    add("collinear", [[0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1]], cloud(4, 3, 2.5))
    add("collinear", [[0, 0, 0], [1, 1, 0], [2, 2, 0]], [[0, 2, 0], [1, 1, 0], [2, 0, 0]])              # two segments that cross
    add("coplanar", sq + [0, 0, 0.5], [[0.5, 0.5, 1.5], [0.25, 0.75, 2], [0.5, 0.25, 1.75]])
    add("coplanar", [[0, 0, 0], [1, 0, 1], [1, 1, 1], [0, 1, 0], [0.5, 0.5, 0.5]], cloud(4, 3, 3.0))
    add("coplanar", sq, sq * 0.5 + [0.25, 0.25, 0.25])                                                    # parallel faces
    add("duplicates", [[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0]], [[2, 2, 0], [2, 2, 0], [3, 2, 0]])
    add("duplicates", np.repeat(cloud(2, 3), 3, axis=0), np.repeat(cloud(3, 3, 2.5), 2, axis=0))
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    add("interior_points", np.vstack((sq, [[0.5, 0.5, 0], [0.25, 0.5, 0]])), np.vstack((sq + [1.5, 0.5, 0], [[2.0, 1.0, 0]])))
    add("interior_points", np.vstack((tet, [[0.125, 0.25, 0.125]])), np.vstack((tet + [1, 1, 1], [[1.25, 1.125, 1.25]])))
    add("interior_points", [[0.2, 0.2, 0.2]], tet)
    for c in out:
        assert 1 <= len(c["P"]) <= 6 and 1 <= len(c["Q"]) <= 6
        c["exact"] = R.hull_dist_sq(c["P"], c["Q"])[0]
        c["scale"] = Fr(max(np.abs(c["P"]).max(), np.abs(c["Q"]).max()))
    return out


def excess(x, h):
    """x - sqrt(h) for rationals, to 2^-256 relative (for the printed figures only: the assertions compare squares)"""
    return x - R.sqrt_dn(h)


def check_gjk(case, r, eps, mult):
    """The assertions on one result of the true hull distance (device or host build): r = dict(flag, dist, lower, c1, c2,
    status) for the point sets of `case`, allowance = mult * 2^-53 * scale.  c1 / c2 are defined for flag 1 only
    (include/obtg.h).  Returns, as multiples of 2^-53 * scale, dict(dist = | dist - |c1 - c2| |, the measured figure; hull =
    how far c1 / c2 are from their hulls; bound = by how much lower exceeds, or dist falls short of, the exact distance)."""
    exact, scale = case["exact"], case["scale"]
    unit = U53 * scale
    allow = mult * unit
    tol = Fr(eps) * scale
    dist, lower = Fr(float(r["dist"])), Fr(float(r["lower"]))
    assert r["status"] in (0, 2), case["kind"]
    if exact > tol * tol:
        assert r["flag"] == 1, case["kind"]
    if exact == 0:
        assert r["flag"] == 0, case["kind"]
    if r["flag"] == 0:
        # "touching": the simplex point came within eps * scale of the origin, or the origin is inside a tetrahedron
        assert dist == 0 and exact <= (tol + allow) ** 2, case["kind"]
        return dict(dist=Fr(0), hull=Fr(0), bound=Fr(0))
    c1, c2 = [Fr(float(x)) for x in r["c1"]], [Fr(float(x)) for x in r["c2"]]
    gap2 = sum((a - b) ** 2 for a, b in zip(c1, c2))
    h1, h2 = R.hull_dist_sq([c1], case["P"])[0], R.hull_dist_sq([c2], case["Q"])[0]
    m = dict(dist=abs(excess(dist, gap2)) / unit, hull=R.sqrt_dn(max(h1, h2)) / unit,
             bound=max(excess(lower, exact), -excess(dist, exact), Fr(0)) / unit)
    assert R.le_sqrt(lower - allow, exact) and R.ge_sqrt(dist + allow, exact), (case["kind"], float(dist), float(lower), float(exact))
    if r["status"] == 0:
        assert dist - lower <= Fr(eps) * dist, case["kind"]
    assert R.within(dist, gap2, allow), (case["kind"], float(m["dist"]))
    assert h1 <= allow * allow and h2 <= allow * allow, (case["kind"], float(m["hull"]))
    return m


def worst(ms):
    """the largest of each figure over a list of check_* results, as floats"""
    return {k: float(max(m[k] for m in ms)) for k in ms[0]} if ms else {}


# ------------------------------------------------------------------ (b) curve pairs
def _jit(rng, K, amp):
    j = rng.uniform(-amp, amp, K)
    j[0] = j[-1] = 0.0
    return j


def _ray(rng, K, start, sign):
    """leaves `start` along sign * x: its point nearest to anything on the other side of `start` is its first"""
    c = np.zeros((3, K))
    c[0] = start[0] + sign * 0.5 * np.arange(K) + _jit(rng, K, 0.05)
    c[1] = start[1] + _jit(rng, K, 0.1)
    c[2] = start[2] + _jit(rng, K, 0.1)
    return c


def _touch_curve(K):
    """(n s / 8, L (s - 3/8)^2, 0) with L the odd part of the elevated coefficients' denominators: every coefficient a float"""
    n = K - 1
    y = [Fr(9, 64), Fr(-15, 64), Fr(25, 64)]
    for m in range(3, n + 1):
        y = [y[0]] + [Fr(i, m) * y[i - 1] + (1 - Fr(i, m)) * y[i] for i in range(1, m)] + [y[-1]]
    L = 1
    for c in y:
        d = c.denominator
        while d % 2 == 0:
            d //= 2
        L = lcm(L, d)
    p = 1
    while p < L:
        p *= 2
    yy = [float(c * L / p) for c in y]
    assert all(Fr(v) == c * L / p for v, c in zip(yy, y))
    return np.array([np.arange(K) / 8.0, yy, np.zeros(K)])


def _curve_cases(K):
    rng = np.random.default_rng(100 + K)
    n = K - 1
    u = np.arange(K) / n
    curves, pa, pb, kinds = [], [], [], []

    def add(kind, A, B=None):
        if kind not in MDR_KINDS[K]:
            return
        curves.append(np.array(A, float))
        pa.append(len(curves) - 1)
        if B is not None:
            curves.append(np.array(B, float))
        pb.append(len(curves) - 1)
        kinds.append(kind)
    if K == 2:      # skew lines
        gA = np.array([[-1.0, 1.0], [0.0, 0.25], [0.0, 0.125]])
        gB = np.array([[0.125, 0.375], [-1.0, 1.0], [1.0, 1.25]])
    else:           # two arcs that bulge towards each other
        b = 3.2 * u * (1 - u)
        gA = np.array([-1 + b + _jit(rng, K, 0.05), -1 + 2 * u, _jit(rng, K, 0.1)])
        gB = np.array([1.5 - b + _jit(rng, K, 0.05), -0.75 + 2 * u, 0.25 + _jit(rng, K, 0.1)])
    add("generic3d", gA, gB)
    rA, rB = _ray(rng, K, (-0.5, 0.0, 0.0), -1), _ray(rng, K, (0.5, 0.25, 0.125), +1)
    add("c00", rA, rB)
    add("c01", rA, rB[:, ::-1])
    add("c10", rA[:, ::-1], rB)
    add("c11", rA[:, ::-1], rB[:, ::-1])
    wall = np.array([_jit(rng, K, 0.05), -1 + 2 * u, _jit(rng, K, 0.05)])
    away = _ray(rng, K, (0.5, 0.125, 0.0), +1)
    add("edge_s0", away, wall)
    add("edge_t0", wall, away)
    x = -1 + 2 * u
    add("crossing", [x, x + _jit(rng, K, 0.3), np.zeros(K)], [x, -x + _jit(rng, K, 0.3), np.zeros(K)])
    ground = np.array([(-5 * n + 16 * np.arange(K)) / 64.0, np.zeros(K), np.zeros(K)])       # (3 n / 64, 0) at t = 0.5
    if K == 2:
        add("touch", [[0.046875, 0.5], [0.0, 1.0], [0.0, 0.0]], ground)              # an end point on the other segment
    else:
        add("touch", _touch_curve(K), ground)
    add("self", gB)
    i = np.arange(K)
    add("parallel", [i / 8.0, np.zeros(K), np.zeros(K)], [i / 8.0 + n / 16.0, np.ones(K), np.zeros(K)])
    add("point", np.repeat([[0.3], [-2.0], [0.4]], K, axis=1), gA)
    far = np.array([[2.0 ** 20], [0.0], [0.0]])
    add("far", gA + far, gB + far)
    curves = np.array(curves)
    br = []
    for kind, a, b in zip(kinds, pa, pb):
        if kind == "parallel":      # a line of minimisers, which no subdivision closes: y is 0 on one and 1 on the other, so the
            br.append(dict(lo=Fr(1), hi=R.dist_sq_at(curves[a], 0.5, curves[b], 0.0), at=(Fr(1, 2), Fr(0))))     # distance is >= 1
        else:
            br.append(R.curve_dist_sq_bracket(curves[a], curves[b], floor=Fr(1, 10 ** 20)))
    scale = [Fr(max(np.abs(curves[a]).max(), np.abs(curves[b]).max())) for a, b in zip(pa, pb)]
    return dict(curves=curves, pa=np.array(pa, np.int32), pb=np.array(pb, np.int32), kinds=kinds, bracket=br, scale=scale)


# ------------------------------------------------------------------ (e) curves against polygons
def _polygon(rng, nv):
    """nv vertices on a jittered circle, in angular order; the returned table is shuffled and holds one interior point more"""
    ang = np.sort((np.arange(nv) + rng.uniform(-0.2, 0.2, nv)) * 2 * np.pi / nv)
    V = np.array([np.cos(ang), np.sin(ang), np.zeros(nv)]).T * rng.uniform(0.9, 1.1, (nv, 1))
    table = np.vstack((V, [[0.0625, 0.03125, 0.0]]))
    return V, table[rng.permutation(nv + 1)]


def _poly_cases(K):
    rng = np.random.default_rng(200 + K)
    n = K - 1
    tau = 2 * np.arange(K) / n - 1                                  # -1 .. 1
    curves, polys, pc, pp, ckind, pkind, args = [], [], [], [], [], [], []

    def add(ck, A, pi, kind, at=None):
        curves.append(np.array(A, float))
        pc.append(len(curves) - 1)
        pp.append(pi)
        ckind.append(ck)
        args.append((kind, at))
    for nv in (3, 4, 5, 6):
        V, table = _polygon(rng, nv)
        polys.append(table)
        pkind.append("poly%d" % nv)
        pi = len(polys) - 1
        v = V[nv // 2]
        uo = v / np.linalg.norm(v)
        pe = np.array([-uo[1], uo[0], 0.0])
        add("vertex", (v + uo * 0.5)[:, None] + np.outer(uo, 0.6 * tau ** 2 + _jit(rng, K, 0.02)) + np.outer(pe, 0.4 * tau), pi,
            "outside", 0.0)
        a, b = V[0], V[1]
        m, tg = 0.5 * (a + b), b - a
        nr = np.array([tg[1], -tg[0], 0.0]) / np.linalg.norm(tg)     # outward: the vertices run counter-clockwise
        arc = m[:, None] + np.outer(nr, 0.25 + 0.5 * tau ** 2 + _jit(rng, K, 0.02)) + np.outer(tg, 0.3 * tau)
        add("edge", arc, pi, "outside", 0.0)
        add("end_inside", np.array([0.03125 + 1.5 * (tau + 1), -0.0625 + 0.25 * (tau + 1) + _jit(rng, K, 0.1), 0 * tau]), pi, "inside", 0.0)
        add("middle_inside", np.array([2 * tau, 0.0625 * tau + _jit(rng, K, 0.02) * (np.abs(tau) > 0.5), 0 * tau]), pi, "inside", 0.5)
        add("graze", (v + uo * 2.0 ** -20)[:, None] + np.outer(pe, 0.75 * tau), pi, "outside", 0.0)
        lift = arc.copy()
        lift[2] = 0.25 + 0.125 * tau + _jit(rng, K, 0.05)
        add("outside3d", lift, pi, "outside3d", 0.0)
        add("above", np.array([0.125 * tau, 0.0625 * tau ** 2 + _jit(rng, K, 0.05), 0.375 + 0 * tau]), pi, "above")
    g = np.array([-1 + 0.5 * tau + _jit(rng, K, 0.1), 1.5 * tau, 0.5 + 0.25 * tau ** 2 + _jit(rng, K, 0.1)])
    for kind, P in (("one", [[0.5, 0.25, 0.0]]), ("two", [[0.5, -1.0, 0.0], [1.0, 1.0, 0.0]]), ("two3d", [[0.5, -1.0, 0.0], [1.0, 1.0, 1.0]]),
                    ("collinear", [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 0.0, 0.0], [0.25, 0.0, 0.0]])):
        polys.append(np.array(P, float))
        pkind.append(kind)
        add("generic3d", g, len(polys) - 1, "outside", 0.0)
        if kind == "two":
            add("planar", g * [[1], [1], [0]], len(polys) - 1, "outside", 0.0)
    curves = np.array(curves)
    br = []
    for c, p, (kind, at) in zip(pc, pp, args):
        if kind == "outside3d":                         # the projection stays outside; then the boundary decides in 3-D too
            R.curve_poly_dist_sq_bracket(curves[c] * [[1], [1], [0]], polys[p], "outside", at, rel=Fr(1, 100))
            kind = "outside"
        br.append(R.curve_poly_dist_sq_bracket(curves[c], polys[p], kind, at))
    off = np.concatenate(([0], np.cumsum([len(p) for p in polys]))).astype(np.int32)
    scale = [Fr(max(np.abs(curves[c]).max(), np.abs(polys[p]).max())) for c, p in zip(pc, pp)]
    return dict(curves=curves, polys=polys, pts=np.vstack(polys), off=off, pc=np.array(pc, np.int32), pp=np.array(pp, np.int32),
                ckind=ckind, pkind=pkind, bracket=br, scale=scale)


def shared(what, K=None):
    """The case lists, computed once: "gjk" -> list of dict(kind, P, Q, exact, scale); ("curves", K) -> dict(curves[n][3][K],
    pa, pb, kinds, bracket, scale); ("poly", K) -> dict(curves, polys, pts, off, pc, pp, ckind, pkind, bracket, scale)."""
    key = (what, K)
    if key not in _shared:
        _shared[key] = {"gjk": _gjk_cases, "curves": lambda: _curve_cases(K), "poly": lambda: _poly_cases(K)}[what]()
    return _shared[key]


# ------------------------------------------------------------------ the yardsticks against closed forms
def test_hull_dist_sq_closed_forms():
    H = R.hull_dist_sq
    assert H([[0, 0, 0]], [[3, 4, 0]])[0] == 25
    d2, c1, c2, w1, w2 = H([[0.5, 2, 0]], [[0, 0, 0], [2, 0, 0]])                       # point above a segment's interior
    assert d2 == 4 and c2 == (Fr(1, 2), 0, 0) and w2 == [Fr(3, 4), Fr(1, 4)] and w1 == [1]
    assert H([[3, 1, 0]], [[0, 0, 0], [2, 0, 0]])[0] == 2                                 # beyond its end
    assert H([[0, 0, 0], [1, 0, 0]], [[0, 1, 1], [1, 1, 1]])[0] == 2                      # parallel segments
    d2, c1, c2, _, _ = H([[-1, 0, 0], [1, 0, 0]], [[0, -1, 0.75], [0, 1, 0.75]])          # skew segments
    assert d2 == Fr(9, 16) and c1 == (0, 0, 0) and c2 == (0, 0, Fr(3, 4))
    assert H([[0, 0, 0], [2, 2, 0]], [[0, 2, 0], [2, 0, 0]])[0] == 0                      # crossing segments
    assert H([[0, 0], [1, 0]], [[0.5, 0.25], [3, 1]])[0] == Fr(1, 16)                     # 2-D input
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], float)                  # test_true_gjk_known_cases
    assert H(sq, sq + [3, 0, 0])[0] == 4 and H(sq, sq + [2, 2, 0])[0] == 2 and H(sq, sq + [0.5, 0.5, 0])[0] == 0
    d2, _, c2, _, _ = H([[0.5, 0.5, 2.0]], sq)
    assert d2 == 4 and c2 == (Fr(1, 2), Fr(1, 2), 0)
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    assert H([[0.25, 0.25, 0.25]], tet)[0] == 0 and H([[1.0, 1.0, 1.0]], tet)[0] == Fr(4, 3)
    p1 = np.array([(4, 11, 0), (4, 5, 0), (9, 9, 0)], float)                              # dyn4j's demo pair: distance to an edge
    p2 = np.array([(8, 6, 0), (10, 2, 0), (13, 1, 0), (15, 6, 0)], float)
    d2, c1, c2, w1, w2 = H(p1, p2)
    assert d2 == Fr(121, 41) and c2 == (8, 6, 0) and sum(w1) == 1 and sum(w2) == 1
    rng = np.random.default_rng(3)
    for _ in range(10):                                                                    # weights, points and value agree
        P, Q = rng.normal(size=(4, 3)), rng.normal(size=(5, 3)) + [2, 0, 0]
        d2, c1, c2, w1, w2 = H(P, Q)
        assert min(w1) >= 0 and min(w2) >= 0 and sum(w1) == 1 and sum(w2) == 1
        assert c1 == tuple(sum(w * Fr(x) for w, x in zip(w1, P[:, q])) for q in range(3))
        assert d2 == sum((a - b) ** 2 for a, b in zip(c1, c2))
        assert all(d2 <= sum((Fr(a) - Fr(b)) ** 2 for a, b in zip(p, q)) for p in P for q in Q)
        assert H(Q, P)[0] == d2


def test_eval_curve_and_tensor_form():
    A = np.array([[0.0, 1.0, 3.0], [0.0, 2.0, 0.0], [1.0, 1.0, 1.0]])
    assert R.eval_curve(A, 0.5) == (Fr(5, 4), 1, 1) and R.eval_curve(A, 0.0) == (0, 0, 1) and R.eval_curve(A, 1.0) == (3, 0, 1)
    rng = np.random.default_rng(5)
    A, B = rng.normal(size=(3, 4)), rng.normal(size=(3, 2))
    D = R.dist_sq_tensor(A, B)
    assert len(D) == 7 and len(D[0]) == 3
    assert D[0][0] == R.dist_sq_at(A, 0, B, 0) and D[-1][0] == R.dist_sq_at(A, 1, B, 0) and D[0][-1] == R.dist_sq_at(A, 0, B, 1)
    for s, t in ((0.25, 0.75), (0.5, 0.5), (0.8125, 0.125)):                               # the form IS the squared distance
        rows = [R.eval_curve([[x for x in r]], t)[0] for r in D]
        assert R.eval_curve([rows], s)[0] == R.dist_sq_at(A, s, B, t)


def test_curve_bracket_closed_forms():
    seg = lambda a, b: np.array([a, b], float).T                                           # noqa: E731
    r = R.curve_dist_sq_bracket(seg((0, 0, 0), (2, 0, 0)), seg((0.5, 1, 0), (0.5, 3, 0)))
    assert r["lo"] <= 1 <= r["hi"] and r["hi"] - r["lo"] <= r["hi"] / 10 ** 12
    r = R.curve_dist_sq_bracket(seg((-1, 0, 0), (1, 0, 0)), seg((0, -1, 0.75), (0, 1, 0.75)))
    assert r["hi"] == Fr(9, 16) and r["at"] == (Fr(1, 2), Fr(1, 2)) and r["lo"] <= r["hi"] <= r["lo"] * (1 + Fr(2, 10 ** 12))
    r = R.curve_dist_sq_bracket(seg((0, 0, 0), (2, 2, 0)), seg((0, 2, 0), (2, 0, 0)))
    assert r["hi"] == 0 and r["lo"] == 0
    r = R.curve_dist_sq_bracket(seg((0, 0, 0), (3, 0, 0)), seg((0, 3, 0), (2, 1, 0)))    # the second one's end
    assert r["lo"] <= 1 <= r["hi"] and r["hi"] - r["lo"] <= r["hi"] / 10 ** 12 and r["at"][1] == 1
    par = np.array([[0.0, 0.5, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])                    # y = 2 s (1 - s), top (0.5, 0.5)
    r = R.curve_dist_sq_bracket(par, seg((-1, 1, 0), (2, 1, 0)))                           # the line y = 1 above it
    assert r["hi"] == Fr(1, 4) and r["lo"] <= Fr(1, 4) and r["hi"] - r["lo"] <= r["hi"] / 10 ** 12
    rng = np.random.default_rng(9)
    for K in (3, 6):
        A = rng.uniform(-1, 1, (3, K))
        r = R.curve_dist_sq_bracket(A, A)                                                   # a curve against itself
        assert r["lo"] == r["hi"] == 0 and r["nodes"] == 1
        A[2] = 0.0                                                                          # planar, and lifted by h: exactly h
        B = A.copy()
        B[2] = 0.375
        r = R.curve_dist_sq_bracket(A, B, rel=Fr(1, 100))                                   # (a diagonal of minimisers)
        assert r["hi"] == Fr(9, 64) and r["hi"] * Fr(99, 100) <= r["lo"] <= r["hi"]
        B = rng.uniform(-1, 1, (3, K)) + [[2.5], [0], [0]]
        r = R.curve_dist_sq_bracket(A, B)
        assert 0 < r["lo"] <= r["hi"] and r["hi"] - r["lo"] <= r["hi"] / 10 ** 12
        assert r["hi"] == R.dist_sq_at(A, r["at"][0], B, r["at"][1])
        ts = np.linspace(0, 1, 41)
        assert all(R.dist_sq_at(A, s, B, t) >= r["lo"] for s in ts[::4] for t in ts[::4])


def test_curve_poly_bracket_closed_forms():
    sq = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 0]]
    line = lambda a, b: np.array([a, b], float).T                                          # noqa: E731
    r = R.curve_poly_dist_sq_bracket([[0, 0.5, 1], [2, 1, 2], [0, 0, 0]], sq, "outside", 0.0)      # lowest at (0.5, 1.5)
    assert r["lo"] <= Fr(1, 4) == r["hi"] and r["hi"] - r["lo"] <= r["hi"] / 10 ** 12 and r["at"] == Fr(1, 2)
    r = R.curve_poly_dist_sq_bracket(line((2, 3, 0), (3, 2, 0)), sq, "outside", 0.0)      # nearest the corner (1, 1)
    assert r["lo"] <= Fr(9, 2) <= r["hi"]
    assert R.curve_poly_dist_sq_bracket(line((-1, 0.5, 0), (2, 0.5, 0)), sq, "inside", 0.5) == dict(lo=0, hi=0)
    assert R.curve_poly_dist_sq_bracket(line((0.25, 0.25, 0.75), (0.75, 0.5, 0.75)), sq, "above") == dict(lo=Fr(9, 16), hi=Fr(9, 16))
    with pytest.raises(AssertionError):
        R.curve_poly_dist_sq_bracket(line((-1, 0.25, 0), (2, 0.75, 0)), sq, "outside", 0.0)  # it goes through: lo is 0
    with pytest.raises(AssertionError):
        R.curve_poly_dist_sq_bracket(line((0.25, 0.25, 0.75), (1.75, 0.5, 0.75)), sq, "above")


def test_comparisons_on_squares():
    assert R.le_sqrt(Fr(3, 2), Fr(9, 4)) and not R.le_sqrt(Fr(3, 2) + Fr(1, 10 ** 30), Fr(9, 4)) and R.le_sqrt(Fr(-1), Fr(0))
    assert R.ge_sqrt(Fr(3, 2), Fr(9, 4)) and not R.ge_sqrt(Fr(3, 2) - Fr(1, 10 ** 30), Fr(9, 4)) and not R.ge_sqrt(Fr(-2), Fr(1))
    assert R.within(Fr(1), Fr(2), Fr(1, 2)) and not R.within(Fr(1), Fr(2), Fr(2, 5))
    s = R.sqrt_dn(Fr(2))
    assert s * s <= 2 < (s + Fr(1, 2 ** 200)) ** 2
    assert R.is_dyadic_unit(0.0) and R.is_dyadic_unit(0.625) and not R.is_dyadic_unit(-1.0) and not R.is_dyadic_unit(Fr(1, 3))


# ------------------------------------------------------------------ the lists hold what they are meant to
def test_gjk_list_holds_every_kind():
    cases = shared("gjk")
    kinds = {c["kind"] for c in cases}
    assert kinds == {"separated2d", "separated3d", "overlapping2d", "overlapping3d", "shared_vertex", "gap_2^-30", "points",
                     "collinear", "coplanar", "duplicates", "interior_points"}
    for c in cases:
        k = c["kind"]
        if k.startswith("separated"):
            assert c["exact"] > 0
        if k.startswith("overlapping") or k == "shared_vertex":
            assert c["exact"] == 0
        if k.endswith("2d"):
            assert not c["P"][:, 2].any() and not c["Q"][:, 2].any()
        if k == "gap_2^-30":
            assert c["exact"] == Fr(1, 2 ** 60)
    assert {len(c["P"]) for c in cases} | {len(c["Q"]) for c in cases} == {1, 2, 3, 4, 5, 6}
    assert any(c["exact"] > (Fr(1, 10 ** 9) * c["scale"]) ** 2 for c in cases if c["kind"] == "gap_2^-30")


@pytest.mark.parametrize("K", MDR_K)
def test_curve_list_holds_every_kind(K):
    s = shared("curves", K)
    assert tuple(s["kinds"]) == MDR_KINDS[K] and s["curves"].shape[1:] == (3, K)
    assert K < 11 or len(s["kinds"]) <= 4
    inside = lambda x: 0 < x < 1                                                            # noqa: E731
    for kind, br, a, b in zip(s["kinds"], s["bracket"], s["pa"], s["pb"]):
        at, A, B = br["at"], s["curves"][a], s["curves"][b]
        assert br["lo"] <= br["hi"] == R.dist_sq_at(A, at[0], B, at[1])
        if kind in ("generic3d", "far"):
            assert inside(at[0]) and inside(at[1]) and br["lo"] > 0 and A[2].any()
        if kind in ("c00", "c01", "c10", "c11"):
            assert at == (int(kind[1]), int(kind[2])) and br["lo"] > 0
        if kind == "edge_s0":
            assert at[0] == 0 and inside(at[1])
        if kind == "edge_t0":
            assert inside(at[0]) and at[1] == 0
        if kind in ("crossing", "touch"):
            assert br["hi"] <= Fr(1, 10 ** 20) and not A[2].any() and not B[2].any() and K <= 6
        if kind == "touch":                                             # above the other curve's line except at one point
            s0 = 0.375 if K > 2 else 0.0
            assert (B[1] == 0).all() and br["hi"] == 0 and br["at"] == (s0, 0.5) and (A[1, 0] > 0 or K == 2)
            assert all(R.eval_curve(A, t)[1] > 0 for t in (0.25, 0.3125, 0.4375, 0.5, 1.0))
        if kind == "crossing":                                          # each end of one on another side of the other
            assert (A[0] == B[0]).all() and A[1, 0] < B[1, 0] and A[1, -1] > B[1, -1]
        if kind == "self":
            assert a == b and br["hi"] == 0
        if kind == "parallel":
            assert br["hi"] == br["lo"] == 1 and (A[1] == 0).all() and (B[1] == 1).all()
            assert all(np.array_equal(np.diff(C, axis=1), np.repeat([[0.125], [0], [0]], K - 1, axis=1)) for C in (A, B))
        if kind == "point":
            assert (A == A[:, :1]).all()
        if kind == "far":
            assert min(A[0].min(), B[0].min()) >= 2.0 ** 20 - 2


@pytest.mark.parametrize("K", MD2R_K)
def test_poly_list_holds_every_kind(K):
    s = shared("poly", K)
    assert tuple(s["pkind"]) == MD2R_POLYS and [len(p) for p in s["polys"]] == [4, 5, 6, 7, 1, 2, 2, 4]
    seen = set()
    for ck, c, p, br in zip(s["ckind"], s["pc"], s["pp"], s["bracket"]):
        seen.add((ck, s["pkind"][p]))
        A, poly = s["curves"][c], s["polys"][p]
        if ck in ("vertex", "edge", "graze"):
            assert not A[2].any() and br["lo"] > 0
        if ck in ("vertex", "edge"):                                     # the hull's feature nearest the curve's nearest point
            w = R.hull_dist_sq([R.eval_curve(A, br["at"])], poly)[4]
            assert 0 < br["at"] < 1 and sum(1 for x in w if x != 0) == (1 if ck == "vertex" else 2), (ck, float(br["at"]))
        if ck in ("end_inside", "middle_inside"):
            assert br == dict(lo=0, hi=0)
            ends = [R.hull_dist_sq([R.eval_curve(A, t)], poly)[0] for t in (0.0, 1.0)]
            assert (ends[0] == 0 and ends[1] > 0) if ck == "end_inside" else (ends[0] > 0 and ends[1] > 0)
        if ck == "graze":
            assert Fr(1, 2 ** 42) <= br["lo"] <= br["hi"] <= Fr(1, 2 ** 38)
        if ck == "above":
            assert br["lo"] == br["hi"] == Fr(9, 64)
        if ck == "outside3d":
            assert A[2].min() > 0 and br["lo"] > 0
    for pk in ("poly3", "poly4", "poly5", "poly6"):
        assert {(ck, pk) for ck in MD2R_CURVES} <= seen
    assert {("generic3d", pk) for pk in ("one", "two", "two3d", "collinear")} <= seen and ("planar", "two") in seen
