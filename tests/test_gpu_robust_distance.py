"""The robust distance searches -- obtg_gjk_true_pairs, obtg_min_dist_robust (the any-count kernel and the register kernels),
obtg_min_dist2poly_robust -- against exact rationals (tests/robust_distance_ref.py) on the case lists that
tests/test_robust_distance_ref.py builds and shows to hold every kind of case.  Every comparison is made in rationals on
squares (x <= sqrt(h) is written x <= 0 or x^2 <= h).  `scale` is the largest absolute coordinate of a pair, as in the kernels.

Non-finite input (include/obtg.h): a pair with a NaN or an inf anywhere in its curves or polygon returns dist = NaN,
parameters -1 (and a NaN polygon point), nodes = 0, status OBTG_MD_OK, and no other pair of the call changes.

The rounding allowance between a reported dist and the exact distance at the reported parameters / points, MEASURED on an
MI355X as the largest multiple of 2^-53 * scale over every case of (a), (b) and (e) at eps 1e-6 and 1e-9, and the bound used,
four times the measured multiple (test_robust_distance_ref.MEASURED / ALLOW; the tests print the figures again):
    kernel                            measured   bound
    k_gjk_true_pairs                    0.8431    3.37    (c1 / c2 off their hulls: 0.62; lower above / dist below exact: 0.70)
    k_min_dist_robust<0>   K = 2        1.3928    5.57
                           K = 3        1.5432    6.17
                           K = 5        1.7567    7.03
                           K = 7        2.2099    8.84
    k_min_dist_robust<K>   K = 4        2.1003    8.40
                           K = 6        2.0755    8.30
                           K = 11       5.3325   21.33
    k_min_dist2poly_robust K = 4        2.2620    9.05    (polygon point off the hull: 0.38)
                           K = 5        1.6307    6.52    (0.42)
                           K = 6        2.2668    9.07    (0.48)
Every bound is far below 1e-3 * eps * scale at eps = 1e-9, which is 9007 x 2^-53 * scale.

eps = 1e-12, run once on the (b) and (e) lists: every pair that ends OK meets the contract above (with these allowances); the
curve search ends OK on all pairs but the K = 2 pair shifted by 2^20 (NODE_CAP after 1853 nodes: eps * dist is below the
rounding of coordinates of that size, 2^-53 * 2^20), the polygon search on all but the four curves in a plane above the
polygon (a stretch of equal minimisers; NODE_CAP).  A search that cannot close says so; no eps is refused.

Two defects these tests found on finite input, fixed in the kernels: a point-curve (all control points equal) against a curve
filled the frontier (NODE_CAP at every K), since every parameter of the point-curve is a minimiser -- its side of a node is
no longer cut; and obtg_min_dist2poly_robust reported dist = 0 for a curve 2^-20 away from a vertex at eps = 1e-6 (its
end-point distances were zeroed inside eps * scale), below the true minimum -- dist is now always the distance between the
curve's point and the returned polygon point.
"""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_distance_ref as R  # noqa: E402
import test_robust_distance_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = (1e-6, 1e-9)
U53 = T.U53


@pytest.fixture(scope="module")
def capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    assert _capi.device_count() > 0, "these tests need the GPU"
    return _capi


@pytest.fixture
def ctx(capi):
    c = capi.Context(1, 2, 1, 0, device=capi.default_device())
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(r, q, keys, i=slice(None), j=slice(None)):
    return all(np.array_equal(_bits(r[k][i]) if r[k].dtype == np.float64 else r[k][i],
                              _bits(q[k][j]) if q[k].dtype == np.float64 else q[k][j]) for k in keys)


MDR_KEYS = ("res", "nodes", "levels", "frontier", "status")
GJK_KEYS = ("flag", "c1", "c2", "dist", "lower", "iters", "status")


def test_allowances_are_far_below_the_tolerance():
    """the condition of the contract: every allowance stays below 1e-3 * eps * scale at eps = 1e-9"""
    assert T.ALLOW["gjk"] < T.ALLOW_CEILING
    assert all(v < T.ALLOW_CEILING for v in T.ALLOW["mdr"].values()) and all(v < T.ALLOW_CEILING for v in T.ALLOW["md2r"].values())


# ------------------------------------------------------------------ (a) the true hull distance
def _gjk_tables():
    cases = T.shared("gjk")
    sets = [c["P"] for c in cases] + [c["Q"] for c in cases]
    off = np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int32)
    n = len(cases)
    return cases, np.vstack(sets), off, np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)


def gjk_against_exact(ctx, eps, mult):
    cases, pts, off, pa, pb = _gjk_tables()
    r = ctx.gjk_true_pairs(pts, off, pa, pb, eps=eps)
    ms = [T.check_gjk(c, {k: r[k][i] for k in GJK_KEYS}, eps, mult) for i, c in enumerate(cases)]
    return r, T.worst(ms)


@pytest.mark.parametrize("eps", EPS)
def test_gjk_true_pairs_against_exact_hull_distances(ctx, eps):
    """flag == (exact > 0) unless exact <= (eps scale)^2; lower^2 <= exact <= dist^2; dist - lower <= eps dist at status 0;
    |c1 - c2| = dist; c1, c2 in their hulls -- each up to the allowance.  Then the list repeated to 1, 255, 256 and 257 pairs
    (one lane per pair in blocks of 256): every copy carries the bits of the first call."""
    r, w = gjk_against_exact(ctx, eps, T.ALLOW["gjk"])
    print("gjk_true_pairs eps %g: multiples of 2^-53 scale %s" % (eps, w))
    cases, pts, off, pa, pb = _gjk_tables()
    n = len(cases)
    for n_pairs in (1, 255, 256, 257):
        idx = np.arange(n_pairs) % n
        q = ctx.gjk_true_pairs(pts, off, pa[idx], pb[idx], eps=eps)
        assert _same(q, r, GJK_KEYS, slice(None), idx), n_pairs


# ------------------------------------------------------------------ (b) curve against curve
def check_mdr(s, i, res, eps, mult, lower_only=False):
    """one pair's (dist, t1, t2) against its bracket; returns dict(dist = | dist - |A(t1) - B(t2)| | in 2^-53 scale)"""
    A, B = s["curves"][s["pa"][i]], s["curves"][s["pb"][i]]
    br, scale, kind = s["bracket"][i], s["scale"][i], s["kinds"][i]
    unit = U53 * scale
    allow = mult * unit
    dist, t1, t2 = (Fr(float(x)) for x in res)
    assert R.is_dyadic_unit(t1) and R.is_dyadic_unit(t2), (kind, float(t1), float(t2))
    e2 = R.dist_sq_at(A, t1, B, t2)
    m = dict(dist=abs(T.excess(dist, e2)) / unit)
    assert R.within(dist, e2, allow), (kind, float(dist), float(m["dist"]))
    assert R.ge_sqrt(dist + allow, br["lo"]), (kind, float(dist), float(br["lo"]) ** 0.5)
    if not lower_only:
        assert R.le_sqrt(dist * (1 - Fr(eps)) - allow, br["hi"]) or dist <= Fr(eps) * scale, (kind, float(dist), float(br["hi"]) ** 0.5)
    return m


def mdr_against_bracket(ctx, capi, K, eps, mult):
    s = T.shared("curves", K)
    r = ctx.min_dist_robust(s["curves"], s["pa"], s["pb"], eps=eps)
    assert (r["status"] == capi.MD_OK).all(), [(k, st) for k, st in zip(s["kinds"], r["status"]) if st != capi.MD_OK]
    ms = [check_mdr(s, i, r["res"][i], eps, mult) for i in range(len(s["kinds"]))]
    return r, T.worst(ms)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("K", T.MDR_K)
def test_min_dist_robust_against_the_bracket(ctx, capi, K, eps):
    """every pair ends OK; t1, t2 are dyadic in [0, 1]; |A(t1) - B(t2)| evaluated exactly is dist within the allowance;
    dist + allowance >= sqrt(lo); dist (1 - eps) - allowance <= sqrt(hi), or else dist <= eps * scale"""
    r, w = mdr_against_bracket(ctx, capi, K, eps, T.ALLOW["mdr"][K])
    print("min_dist_robust K %d eps %g: multiples of 2^-53 scale %s; nodes %s" % (K, eps, w, r["nodes"].tolist()))


# ------------------------------------------------------------------ (c) caps return a true upper bound
def _arc(K, seed):
    rng = np.random.default_rng(seed)
    u = np.arange(K) / (K - 1)
    return np.array([2 * u, 1.5 * u * (1 - u) + T._jit(rng, K, 0.2), np.zeros(K)])


@pytest.mark.parametrize("K", (4, 6))
def test_caps_return_a_true_upper_bound(ctx, capi, K):
    """A planar curve against its translate along z by 0.5: every (t, t) is a minimiser, the distance is exactly 0.5
    (|A(s) - A(t)|^2 + 0.25 >= 0.25).  Whether the frontier of 1024 nodes fills is not required (it does not: the mid points
    of the root's two curves differ by the offset itself, and the projection on it prunes the root): with OK or NODE_CAP
    alike dist is the exact distance at the reported parameters, and not below the offset; `info` is consistent.  The same
    on a pair of parallel segments, and with a budget of 5 nodes on the generic pairs."""
    A = _arc(K, 300 + K)
    B = A.copy()
    B[2] = 0.5
    s = dict(curves=np.array([A, B]), pa=[0], pb=[1], kinds=["translate"], scale=[Fr(2)], bracket=[dict(lo=Fr(1, 4), hi=Fr(1, 4))])
    for eps in EPS:
        r = ctx.min_dist_robust(s["curves"], [0], [1], eps=eps, max_nodes=200000)
        st = int(r["status"][0])
        print("translate K %d eps %g: status %d nodes %d levels %d frontier %d dist %.17g" %
              (K, eps, st, r["nodes"][0], r["levels"][0], r["frontier"][0], r["res"][0][0]))
        assert st in (capi.MD_OK, capi.MD_NODE_CAP)
        check_mdr(s, 0, r["res"][0], eps, T.ALLOW["mdr"][K], lower_only=st != capi.MD_OK)
        assert 1 <= r["nodes"][0] <= 200000 + 4 * r["frontier"][0] and r["levels"][0] >= 1 and 1 <= r["frontier"][0] <= 1024
    # parallel segments, the second one shifted along itself by 0.3 (no end points opposite each other at any level) and by 1
    # across: a line of minimisers that d = (difference of the mid points) does not prune at once.  y is 0 on one and 1 on
    # the other, so 1 is a lower bound whatever the rounding of x + 0.3 does.
    i = np.arange(K)
    P = np.array([i / 8.0, 0.0 * i, 0.0 * i])
    Q = np.array([i / 8.0 + 0.3, 0.0 * i + 1.0, 0.0 * i])
    s = dict(curves=np.array([P, Q]), pa=[0], pb=[1], kinds=["oblique parallel"], scale=[Fr(float(np.abs(Q).max()))],
             bracket=[dict(lo=Fr(1), hi=Fr(1))])
    for eps in EPS:
        r = ctx.min_dist_robust(s["curves"], [0], [1], eps=eps, max_nodes=200000)
        st = int(r["status"][0])
        print("oblique parallel K %d eps %g: status %d nodes %d levels %d frontier %d dist %.17g" %
              (K, eps, st, r["nodes"][0], r["levels"][0], r["frontier"][0], r["res"][0][0]))
        assert st in (capi.MD_OK, capi.MD_NODE_CAP)
        check_mdr(s, 0, r["res"][0], eps, T.ALLOW["mdr"][K], lower_only=st != capi.MD_OK)
        assert 1 <= r["nodes"][0] <= 200000 + 4 * r["frontier"][0] and r["levels"][0] >= 1 and 1 <= r["frontier"][0] <= 1024
    g = T.shared("curves", K)
    idx = [i for i, k in enumerate(g["kinds"]) if k in ("generic3d", "far", "edge_s0", "c01")]
    r = ctx.min_dist_robust(g["curves"], g["pa"][idx], g["pb"][idx], eps=1e-9, max_nodes=5)
    assert set(r["status"].tolist()) <= {capi.MD_OK, capi.MD_NODE_CAP} and capi.MD_NODE_CAP in r["status"]
    for j, i in enumerate(idx):
        check_mdr(g, i, r["res"][j], 1e-9, T.ALLOW["mdr"][K], lower_only=r["status"][j] != capi.MD_OK)
        assert 1 <= r["nodes"][j] <= 5 + 4 * r["frontier"][j] and r["levels"][j] >= 1


# ------------------------------------------------------------------ (d) identities that need no yardstick
@pytest.mark.parametrize("K", (4, 5))
def test_min_dist_robust_is_scale_free(ctx, K):
    """Every coordinate times 2^40, and 2^-40: dist scales by exactly that power; t1, t2, nodes, levels, status are the same.
    (Every operation of the search is a sum, a product, a quotient or a square root of coordinates, compared with one
    another: none overflows or goes subnormal at these sizes.)"""
    s = T.shared("curves", K)
    r = ctx.min_dist_robust(s["curves"], s["pa"], s["pb"], eps=1e-9)
    for f in (2.0 ** 40, 2.0 ** -40):
        q = ctx.min_dist_robust(s["curves"] * f, s["pa"], s["pb"], eps=1e-9)
        assert np.array_equal(_bits(q["res"][:, 0]), _bits(r["res"][:, 0] * f)), (K, f)
        assert np.array_equal(_bits(q["res"][:, 1:]), _bits(r["res"][:, 1:]))
        assert _same(q, r, ("nodes", "levels", "frontier", "status"))


@pytest.mark.parametrize("K", (4, 5))
def test_min_dist_robust_pairs_do_not_see_each_other(ctx, K):
    s = T.shared("curves", K)
    pa, pb = s["pa"], s["pb"]
    r = ctx.min_dist_robust(s["curves"], pa, pb, eps=1e-9)
    for i in range(len(pa)):
        one = ctx.min_dist_robust(s["curves"], pa[i:i + 1], pb[i:i + 1], eps=1e-9)
        assert _same(one, r, MDR_KEYS, slice(None), slice(i, i + 1)), s["kinds"][i]
    twice = ctx.min_dist_robust(s["curves"], np.concatenate((pa, pa[::-1])), np.concatenate((pb, pb[::-1])), eps=1e-9)
    n = len(pa)
    assert _same(twice, r, MDR_KEYS, slice(0, n)) and _same(twice, r, MDR_KEYS, slice(n, 2 * n), slice(None, None, -1))


@pytest.mark.parametrize("K", (4, 6, 11))
def test_register_form_is_the_any_count_form_on_the_cases(ctx, K, monkeypatch):
    s = T.shared("curves", K)
    fast = ctx.min_dist_robust(s["curves"], s["pa"], s["pb"], eps=1e-9)
    monkeypatch.setenv("OBTG_MDR_GENERIC", "1")
    slow = ctx.min_dist_robust(s["curves"], s["pa"], s["pb"], eps=1e-9)
    monkeypatch.delenv("OBTG_MDR_GENERIC")
    assert _same(fast, slow, MDR_KEYS)


# ------------------------------------------------------------------ (e) curve against polygon
def check_md2r(s, i, res, eps, mult):
    A, poly = s["curves"][s["pc"][i]], s["polys"][s["pp"][i]]
    br, scale, kind = s["bracket"][i], s["scale"][i], (s["ckind"][i], s["pkind"][s["pp"][i]])
    unit = U53 * scale
    allow = mult * unit
    dist, t = Fr(float(res[0])), Fr(float(res[1]))
    c = [Fr(float(x)) for x in res[2:5]]
    assert R.is_dyadic_unit(t), (kind, float(t))
    touch = dist <= Fr(eps) * scale
    e2 = sum((a - b) ** 2 for a, b in zip(R.eval_curve(A, t), c))
    h2 = R.hull_dist_sq([c], poly)[0]
    m = dict(dist=abs(T.excess(dist, e2)) / unit, hull=R.sqrt_dn(h2) / unit)
    assert R.within(dist, e2, allow), (kind, float(dist), float(m["dist"]))
    assert h2 <= allow ** 2, (kind, float(h2) ** 0.5)
    assert R.ge_sqrt(dist + allow, br["lo"]), (kind, float(dist), float(br["lo"]) ** 0.5)
    assert R.le_sqrt(dist * (1 - Fr(eps)) - allow, br["hi"]) or touch, (kind, float(dist), float(br["hi"]) ** 0.5)
    return m


def md2r_against_bracket(ctx, capi, K, eps, mult):
    s = T.shared("poly", K)
    r = ctx.min_dist2poly_robust(s["curves"], s["pts"], s["off"], s["pc"], s["pp"], eps=eps)
    assert (r["status"] == capi.MD_OK).all(), [(k, st) for k, st in zip(s["ckind"], r["status"]) if st != capi.MD_OK]
    ms = [check_md2r(s, i, r["res"][i], eps, mult) for i in range(len(s["ckind"]))]
    return r, T.worst(ms)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("K", T.MD2R_K)
def test_min_dist2poly_robust_against_the_bracket(ctx, capi, K, eps):
    """the bounds of the curve search, and: the returned polygon point lies in the hull, and its exact distance to A(t) is
    dist, both within the allowance"""
    r, w = md2r_against_bracket(ctx, capi, K, eps, T.ALLOW["md2r"][K])
    print("min_dist2poly_robust K %d eps %g: multiples of 2^-53 scale %s; nodes %s" % (K, eps, w, r["nodes"].tolist()))


# ------------------------------------------------------------------ (f) non-finite input
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
@pytest.mark.parametrize("where", ("first", "interior"))
@pytest.mark.parametrize("K", (4, 5))
def test_min_dist_robust_non_finite_input(ctx, capi, K, where, bad):
    s = T.shared("curves", K)
    idx = [s["kinds"].index(k) for k in ("generic3d", "edge_s0", "c11")]
    pa, pb = s["pa"][idx], s["pb"][idx]
    clean = ctx.min_dist_robust(s["curves"], pa, pb, eps=1e-9)
    for side, row in ((pa, 0), (pb, 2), (pa, 1)):
        dirty = s["curves"].copy()
        dirty[side[1], row, 0 if where == "first" else K // 2] = bad
        r = ctx.min_dist_robust(dirty, pa, pb, eps=1e-9)
        assert _same(r, clean, MDR_KEYS, [0, 2], [0, 2])
        assert np.isnan(r["res"][1][0]) and r["res"][1][1] == -1 and r["res"][1][2] == -1
        assert r["nodes"][1] == 0 and r["status"][1] == capi.MD_OK


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
@pytest.mark.parametrize("where", ("first", "interior", "vertex"))
@pytest.mark.parametrize("K", (4, 5))
def test_min_dist2poly_robust_non_finite_input(ctx, capi, K, where, bad):
    s = T.shared("poly", K)
    idx = [i for i, (ck, p) in enumerate(zip(s["ckind"], s["pp"])) if (ck, s["pkind"][p]) in
           (("edge", "poly4"), ("outside3d", "poly5"), ("vertex", "poly6"))]
    pc, pp = s["pc"][idx], s["pp"][idx]
    clean = ctx.min_dist2poly_robust(s["curves"], s["pts"], s["off"], pc, pp, eps=1e-9)
    for row in (0, 1, 2):
        curves, pts = s["curves"].copy(), s["pts"].copy()
        if where == "vertex":
            pts[s["off"][pp[1]] + 2, row] = bad
        else:
            curves[pc[1], row, 0 if where == "first" else K // 2] = bad
        r = ctx.min_dist2poly_robust(curves, pts, s["off"], pc, pp, eps=1e-9)
        assert _same(r, clean, MDR_KEYS, [0, 2], [0, 2])
        assert np.isnan(r["res"][1][0]) and r["res"][1][1] == -1 and np.isnan(r["res"][1][2:]).all()
        assert r["nodes"][1] == 0 and r["status"][1] == capi.MD_OK


def test_bezier_hands_the_nan_on(capi):
    """Bezier.minDist(robust=True) returns the NaN; collCheck(robust=True) and collCheck2Poly(robust=True) answer "collision"
    (0): `NaN > tolerance` is false"""
    from optimalbeziertrajectorygeneration_amd.bezier import Bezier
    s = T.shared("curves", 4)
    i = s["kinds"].index("generic3d")
    A, B = s["curves"][s["pa"][i]], s["curves"][s["pb"][i]]
    assert Bezier(A).collCheck(Bezier(B), robust=True) == 1
    for bad in (np.nan, np.inf):
        D = B.copy()
        D[1, 2] = bad
        d, t1, t2 = Bezier(A).minDist(Bezier(D), robust=True)
        assert np.isnan(d) and t1 == -1 and t2 == -1
        assert Bezier(A).collCheck(Bezier(D), robust=True) == 0 and Bezier(D).collCheck(Bezier(A), robust=True) == 0
        sq = np.array([[3.0, 0, 0], [4, 0, 0], [4, 1, 0], [3, 1, 0]])
        assert Bezier(D).collCheck2Poly(sq, robust=True) == 0
        d, t, pt = Bezier(D).minDist2Poly(sq, robust=True)
        assert np.isnan(d) and t == -1 and np.isnan(pt).all()
