"""The collision checks on the MI355X (obtg_coll_check, obtg_coll_check2poly, Bezier.collCheck / collCheck2Poly) held to the
reference's recorded values (tests/golden/collcheck.npz) and to tests/collcheck_ref.py, the restatement of both
recursions over the CPU oracle: value, node count, gjkNew-call count, depth and status.

What this file runs: the builds of 4, 6, 8, 9, 11 and 16 control points and the any-count build at 5 (2 in the fixture), with the
default eps, max_iter and md_cap; the planar kernels to depth 100 and the `-1` return; the 3-D machine on random 3-D walks,
which are rarely close (the restatement's deepest node there is 5); polygons of 3 .. 16 vertices; config 5's pair list.
tests/test_gpu_collcheck_forms.py holds the forms left over: the any-count build's other counts and its two-pass split
(12 .. 15), the 3-D machine walked deep, polygons of 1 and 2 vertices, the parameters off their defaults, the node budget's
edge, non-finite input, and one context through changing calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collcheck_ref as R  # noqa: E402
from collcheck_cases import walks as _walks  # noqa: E402
from util import assert_identical  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "collcheck.npz")
FAST_COUNTS = (4, 6, 8, 9, 11, 16)        # the control-point counts with a kernel build of their own (OBTG_NC_DYN)
OFF_LIST = 5                              # one count that runs the any-count build


def _capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    return _capi


def _groups(gold, kind):
    for name in gold[kind + "_groups"]:
        name = str(name)
        yield name, {k[len(name) + 1:]: gold[k] for k in gold.files if k.startswith(name + "_") and
                     k[len(name) + 1:] in ("curves", "pa", "pb", "pts", "off", "pc", "pp", "fin", "val", "calls")}


def _same(got, ref, what):
    """device result == restatement: value, nodes, calls, depth, status"""
    for k in ("status", "nodes", "gjk_calls", "depth"):
        bad = np.flatnonzero(got[k] != ref[k])
        assert bad.size == 0, "%s: %s differs on %d pairs, first %d: %d vs %d" % (what, k, bad.size, bad[0], got[k][bad[0]], ref[k][bad[0]])
    assert_identical(got["res"], ref["res"], what)


@pytest.mark.gpu
def test_fixtures_values_and_call_counts_are_the_references():
    capi, gold = _capi(), np.load(GOLDEN)
    ctx = capi.scratch_context()
    n = 0
    for name, g in _groups(gold, "cc"):
        r = ctx.coll_check(g["curves"], g["pa"], g["pb"], max_nodes=20000)
        fin = g["fin"] == 0
        print("%s: %d pairs, %d finished in the reference; device calls %s" % (name, len(fin), fin.sum(), r["gjk_calls"].tolist()))
        assert (r["status"][fin] == capi.MD_OK).all(), name
        assert (r["gjk_calls"][fin] == g["calls"][fin]).all(), (name, r["gjk_calls"][fin], g["calls"][fin])
        assert_identical(r["res"][fin], g["val"][fin], name)
        assert (r["status"][~fin] != capi.MD_OK).all() and (r["res"][~fin] == 0).all(), name
        n += int(fin.sum())
    for name, g in _groups(gold, "cp"):
        r = ctx.coll_check2poly(g["curves"], g["pts"], g["off"], g["pc"], g["pp"], max_nodes=20000)
        fin = g["fin"] == 0
        print("%s: %d pairs, %d finished in the reference; device calls %s" % (name, len(fin), fin.sum(), r["gjk_calls"].tolist()))
        assert (r["status"][fin] == capi.MD_OK).all(), name
        assert (r["gjk_calls"][fin] == g["calls"][fin]).all(), (name, r["gjk_calls"][fin], g["calls"][fin])
        assert_identical(r["res"][fin], g["val"][fin], name)
        assert (r["status"][~fin] != capi.MD_OK).all() and (r["res"][~fin] == 0).all(), name
        n += int(fin.sum())
    assert n >= 150


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_campaign_against_the_restatement(dim):
    """Seeded random curves at every control-point count of the fast list and one off it: all pairs of 26 curves (325) and
    20 curves x 10 polygons (200) per count, 3675 searches per dimension, under a node budget some of them run into."""
    capi = _capi()
    ctx = capi.scratch_context()
    total = 0
    for K in FAST_COUNTS + (OFF_LIST,):
        rng = np.random.default_rng(1000 * dim + K)
        curves = _walks(rng, 26, K, dim, 6.0)
        pa, pb = np.triu_indices(26, 1)
        kw = dict(max_nodes=600)
        got, ref = ctx.coll_check(curves, pa, pb, **kw), R.coll_check_pairs(curves, pa, pb, **kw)
        _same(got, ref, "curve-curve K=%d dim=%d" % (K, dim))
        polys = []
        for _ in range(10):
            k = int(rng.integers(3, 17))
            p = np.zeros((k, 3))
            p[:, :dim] = rng.uniform(0.0, 6.0, size=(1, dim)) + rng.normal(0.0, 1.5, size=(k, dim))
            polys.append(p)
        pts, off = np.vstack(polys), np.concatenate(([0], np.cumsum([len(p) for p in polys]))).astype(np.int32)
        pc, pp = np.repeat(np.arange(20), 10), np.tile(np.arange(10), 20)
        got2 = ctx.coll_check2poly(curves[:20], pts, off, pc, pp, **kw)
        ref2 = R.coll_check2poly_pairs(curves[:20], pts, off, pc, pp, **kw)
        _same(got2, ref2, "curve-polygon K=%d dim=%d" % (K, dim))
        print("K=%d dim=%d: curve-curve values 1: %d, 0: %d, -1: %d, other %d, not OK %d, most calls %d; curve-polygon 1: %d, 0: %d, not OK %d, most calls %d" % (
            K, dim, (ref["res"] == 1).sum(), ((ref["res"] == 0) & (ref["status"] == 0)).sum(), (ref["res"] == -1).sum(),
            ((ref["res"] != 1) & (ref["res"] != 0) & (ref["res"] != -1)).sum(), (ref["status"] != 0).sum(), ref["gjk_calls"].max(),
            (ref2["res"] == 1).sum(), ((ref2["res"] == 0) & (ref2["status"] == 0)).sum(), (ref2["status"] != 0).sum(), ref2["gjk_calls"].max()))
        total += len(pa) + len(pc)
    assert total >= 3000


@pytest.mark.gpu
def test_c5_pair_list_in_one_call():
    """Config 5's 4560 pairs (64 vehicles + 32 curve obstacles, degree 10) in one call against the restatement."""
    capi = _capi()
    g = np.load(os.path.join(HERE, "golden", "c5.npz"))
    Yall = np.vstack((g["Y"], g["Yobs"]))
    curves = np.zeros((96, 3, 11))
    curves[:, :2] = Yall.reshape(96, 2, 11)
    pa, pb = np.triu_indices(96, 1)
    assert len(pa) == 4560
    got = capi.scratch_context().coll_check(curves, pa, pb, max_nodes=2000)
    ref = R.coll_check_pairs(curves, pa, pb, max_nodes=2000)
    _same(got, ref, "C5 pair list")
    print("C5: %d of 4560 pairs end at the root, %d gjkNew calls in all, most %d, not OK %d" % (
        (ref["gjk_calls"] == 1).sum(), ref["gjk_calls"].sum(), ref["gjk_calls"].max(), (ref["status"] != 0).sum()))


@pytest.mark.gpu
def test_usage_example_c1_poly2_stops_under_the_same_budget():
    """Examples/BezierUsageExamples.py section 4, which the reference does not come back from: the same status after the same
    number of calls, device and restatement, under two node budgets."""
    capi, gold = _capi(), np.load(GOLDEN)
    c1, poly2 = gold["usage_curves"][0], gold["usage_poly_pts"][gold["usage_poly_off"][1]:gold["usage_poly_off"][2]]
    for budget in (300, 3000):
        got = capi.scratch_context().coll_check2poly(c1[None], poly2, [0, len(poly2)], [0], [0], max_nodes=budget)
        ref = R.coll_check2poly(c1, poly2, max_nodes=budget)
        print("c1 / poly2, max_nodes %d: device %s, restatement %s" % (budget, {k: v.tolist() for k, v in got.items()}, ref))
        assert ref["status"] != R.MD_OK
        for k in ("status", "nodes", "gjk_calls", "depth", "res"):
            assert got[k][0] == ref[k], (budget, k)


@pytest.mark.gpu
def test_bezier_methods_on_the_usage_example():
    from optimalbeziertrajectorygeneration_amd import bezier as bez
    gold = np.load(GOLDEN)
    c = [bez.Bezier(x) for x in gold["usage_curves"]]
    off, pts = gold["usage_poly_off"], gold["usage_poly_pts"]
    poly1, poly2 = pts[off[0]:off[1]], pts[off[1]:off[2]]
    v34 = c[2].collCheck(c[3])
    assert v34 == 0.0 and v34 != 1                                   # section 3: "Collision detected between C3 and C4"
    assert c[0].collCheck(c[1]) == 1 and isinstance(c[0].collCheck(c[1]), int)
    assert c[0].collCheck2Poly(poly1) == 1
    with pytest.raises(RuntimeError):                                # section 4: the reference does not come back
        c[0].collCheck2Poly(poly2, max_nodes=3000)
    # robust=True answers all four questions (NOT the reference's values): c3 and c4 cross, c1 passes through poly2's hull
    assert c[2].collCheck(c[3], robust=True) == 0
    assert c[0].collCheck(c[1], robust=True) == 1
    assert c[0].collCheck2Poly(poly1, robust=True) in (0, 1)
    assert c[0].collCheck2Poly(poly2, robust=True) in (0, 1)
    d1 = c[0].minDist2Poly(poly1, robust=True)[0]
    d2 = c[0].minDist2Poly(poly2, robust=True)[0]
    assert c[0].collCheck2Poly(poly1, robust=True) == (1 if d1 > 1e-9 * 5 else 0)
    assert c[0].collCheck2Poly(poly2, robust=True) == (1 if d2 > 1e-9 * 5 else 0)


@pytest.mark.gpu
def test_repeatable_and_empty_lists():
    capi = _capi()
    ctx = capi.scratch_context()
    rng = np.random.default_rng(7)
    curves = _walks(rng, 30, 11, 2, 6.0)
    pa, pb = np.triu_indices(30, 1)
    a, b = ctx.coll_check(curves, pa, pb, max_nodes=600), ctx.coll_check(curves, pa, pb, max_nodes=600)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    poly = np.array([[0.0, 0, 0], [3, 0, 0], [0, 3, 0]])
    pc = np.arange(30)
    a = ctx.coll_check2poly(curves, poly, [0, 3], pc, np.zeros(30, int), max_nodes=600)
    b = ctx.coll_check2poly(curves, poly, [0, 3], pc, np.zeros(30, int), max_nodes=600)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    e = ctx.coll_check(curves, [], [])
    assert e["res"].shape == (0,) and e["status"].shape == (0,)
    e = ctx.coll_check2poly(curves, poly, [0, 3], [], [])
    assert e["res"].shape == (0,)
    with pytest.raises(Exception):                                   # more than 16 control points: unsupported, not a fall-back
        ctx.coll_check(np.zeros((2, 3, 17)), [0], [1])
