"""obtg_coll_check / obtg_coll_check2poly held to the restatement (tests/collcheck_ref.py) in EVERY kernel form, on the inputs
of tests/collcheck_cases.py: value, node count, gjkNew-call count, depth and status of every pair.

    control-point counts   2, 3, 5, 7, 10 (the any-count build, one-pass split; 10 is its last one-pass count), 12 .. 15 (its
                           two-pass split), 4 (own build, one pass), 11 and 16 (own builds, two passes)
    machines               planar (z = +0) and the 3-D one: z = -0 (the planar results byte for byte), z = 1, and the plane
                           x = 0.5, where the 3-D machine walks to depth 100, returns -1 and runs out of 600 nodes
    polygons               1, 2, 3, 7 and 16 vertices, in the curves' plane in all four placings and off it
    parameters             eps, max_iter, md_cap off their defaults; max_nodes at N + 1, N, N - 1, 1 and 0
    non-finite input       NaN, +inf, -inf in a control point or a vertex: the restatement's (= the reference's,
                           tests/golden/collcheck_forms.npz) definite answers
    one context            K, form and machine changing from call to call; one list holding every group of a count

tests/test_collcheck_cases_ref.py (no GPU) asserts that the cases reach all of this in the restatement.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collcheck_cases as C  # noqa: E402
import collcheck_ref as R  # noqa: E402
from test_gpu_collcheck import _same  # noqa: E402
from util import assert_identical  # noqa: E402

FORMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collcheck_forms.npz")
ERR_ARG = -1


def _capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    return _capi


def _fresh():
    capi = _capi()
    return capi.Context(1, 2, 1, 0, device=capi.default_device())


def _bytes_equal(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("K", C.KS)
def test_every_group_of_a_count_against_the_restatement(K):
    ctx = _capi().scratch_context()
    got = {}
    for placing in C.PLACINGS:
        got[placing] = C.run_curves(ctx.coll_check, C.curve_group(K, placing))
        # (the restatement of minus_zero is planar's: tests/test_collcheck_cases_ref.py)
        ref = C.ref_curve_group(K, "planar" if placing == "minus_zero" else placing)
        _same(got[placing], ref, "curve-curve K=%d %s" % (K, placing))
    _bytes_equal(got["minus_zero"], got["planar"], "curve-curve K=%d: z = -0 (the 3-D machine) against z = +0 (the planar build)" % K)
    gotp = {}
    for placing in C.POLY_PLACINGS:
        gotp[placing] = C.run_polys(ctx.coll_check2poly, C.poly_group(K, placing))
        ref = C.ref_poly_group(K, "planar" if placing == "minus_zero" else placing)
        _same(gotp[placing], ref, "curve-polygon K=%d %s" % (K, placing))
    _bytes_equal(gotp["minus_zero"], gotp["planar"], "curve-polygon K=%d: z = -0 against z = +0" % K)
    g, ref = C.list_case(K)
    _same(C.run_curves(ctx.coll_check, g), ref, "one list of every group, K=%d" % K)


@pytest.mark.gpu
def test_parameters_off_their_defaults():
    ctx = _capi().scratch_context()
    g, gp = C.curve_group(C.PARAM_K, "planar"), C.poly_group(C.PARAM_K, "planar")
    for i, kw in enumerate(C.CURVE_PARAMS):
        _same(C.run_curves(ctx.coll_check, g, **kw), C.ref_curve_params(i), "curve-curve %s" % kw)
    for i, kw in enumerate(C.POLY_PARAMS):
        _same(C.run_polys(ctx.coll_check2poly, gp, **kw), C.ref_poly_params(i), "curve-polygon %s" % kw)


@pytest.mark.gpu
def test_node_budget_at_its_edge():
    """max_nodes = N + 1, N, N - 1 and 1 around a search of N nodes, in both forms; 0 is OBTG_ERR_ARG (include/obtg.h)."""
    capi = _capi()
    ctx = capi.scratch_context()
    b, p = C.budget_curve_case(), C.budget_poly_case()
    for m in C.budgets(b["N"]):
        got = ctx.coll_check(b["curves"], b["pa"], b["pb"], max_nodes=m)
        _same(got, R.coll_check_pairs(b["curves"], b["pa"], b["pb"], max_nodes=m), "curve-curve max_nodes=%d (N = %d)" % (m, b["N"]))
        assert got["status"][0] == (R.MD_OK if m >= b["N"] else R.MD_NODE_CAP) and got["nodes"][0] == min(m, b["N"])
    for m in C.budgets(p["N"]):
        got = ctx.coll_check2poly(p["curves"], p["pts"], p["off"], p["pc"], p["pp"], max_nodes=m)
        _same(got, R.coll_check2poly_pairs(p["curves"], p["pts"], p["off"], p["pc"], p["pp"], max_nodes=m),
              "curve-polygon max_nodes=%d (N = %d)" % (m, p["N"]))
        assert got["status"][0] == (R.MD_OK if m >= p["N"] else R.MD_NODE_CAP) and got["nodes"][0] == min(m, p["N"])
    with pytest.raises(capi.ObtgError) as e:
        ctx.coll_check(b["curves"], b["pa"], b["pb"], max_nodes=0)
    assert e.value.code == ERR_ARG
    with pytest.raises(capi.ObtgError) as e:
        ctx.coll_check2poly(p["curves"], p["pts"], p["off"], p["pc"], p["pp"], max_nodes=0)
    assert e.value.code == ERR_ARG


@pytest.mark.gpu
def test_non_finite_control_points_and_vertices():
    """Every case ends MD_OK in the restatement, so `res` is compared on every pair."""
    ctx = _capi().scratch_context()
    for (name, curves), ref in zip(C.nonfinite_curve_cases(), C.ref_nonfinite_curves()):
        assert (ref["status"] == R.MD_OK).all()
        _same(ctx.coll_check(curves, *C.NF_PAIRS, max_nodes=C.MAX_NODES), ref, "curve-curve " + name)
    for (name, curves, tri), ref in zip(C.nonfinite_poly_cases(), C.ref_nonfinite_polys()):
        assert (ref["status"] == R.MD_OK).all()
        got = ctx.coll_check2poly(curves, tri, C.NF_TRI["off"], C.NF_TRI["pc"], C.NF_TRI["pp"], max_nodes=C.MAX_NODES)
        _same(got, ref, "curve-polygon " + name)


@pytest.mark.gpu
def test_recorded_forms_are_the_references():
    """tests/golden/collcheck_forms.npz: the reference's value and gjkNew-call count wherever it finished."""
    capi, gold = _capi(), np.load(FORMS)
    ctx = capi.scratch_context()
    keys = ("curves", "pa", "pb", "pts", "off", "pc", "pp", "fin", "val", "calls")
    n = 0
    for kind in ("cc", "cp"):
        for name in gold[kind + "_groups"]:
            name = str(name)
            g = {k: gold[name + "_" + k] for k in keys if name + "_" + k in gold.files}
            if kind == "cc":
                r = ctx.coll_check(g["curves"], g["pa"], g["pb"], max_nodes=20000)
            else:
                r = ctx.coll_check2poly(g["curves"], g["pts"], g["off"], g["pc"], g["pp"], max_nodes=20000)
            fin = g["fin"] == 0
            assert (r["status"][fin] == capi.MD_OK).all(), name
            assert (r["gjk_calls"][fin] == g["calls"][fin]).all(), (name, r["gjk_calls"][fin], g["calls"][fin])
            assert_identical(r["res"][fin], g["val"][fin], name)
            assert (r["status"][~fin] != capi.MD_OK).all() and (r["res"][~fin] == 0).all(), name
            n += int(fin.sum())
    assert n >= 30


@pytest.mark.gpu
def test_seventeen_points_still_raise():
    capi = _capi()
    ctx = capi.scratch_context()
    c16 = C.curve_group(16, "planar")["curves"]
    with pytest.raises(capi.ObtgError) as e:
        ctx.coll_check(np.zeros((2, 3, 17)), [0], [1], max_nodes=C.MAX_NODES)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ObtgError) as e:
        ctx.coll_check2poly(np.zeros((2, 3, 17)), np.zeros((3, 3)), [0, 3], [0], [0], max_nodes=C.MAX_NODES)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ObtgError) as e:
        ctx.coll_check2poly(c16, np.zeros((17, 3)), [0, 17], [0], [0], max_nodes=C.MAX_NODES)
    assert e.value.code == capi.ERR_UNSUPPORTED
    p16 = C.poly_group(16, "planar")["pts"][6:22]                                                    # 16 and 16: the limit itself
    _same(ctx.coll_check2poly(c16, p16, [0, 16], [0], [0], max_nodes=C.MAX_NODES),
          R.coll_check2poly_pairs(c16, p16, [0, 16], [0], [0], max_nodes=C.MAX_NODES), "16 control points against 16 vertices")


@pytest.mark.gpu
def test_one_context_through_changing_counts_forms_and_machines():
    """The stack and the queue are re-sized per call: K = 16 in 3-D, K = 2 planar, polygons at K = 13 in 3-D, K = 12 planar, an
    empty list, K = 16 in 3-D again -- each what a fresh context answers, the last the first byte for byte."""
    steps = [("cc", C.curve_group(16, "plane_yz")), ("cc", C.curve_group(2, "planar")), ("cp", C.poly_group(13, "plane_z1")),
             ("cc", C.curve_group(12, "planar")), ("cc", dict(C.curve_group(12, "planar"), pa=[], pb=[])),
             ("cc", C.curve_group(16, "plane_yz"))]

    def run(ctx, kind, g):
        return C.run_curves(ctx.coll_check, g) if kind == "cc" else C.run_polys(ctx.coll_check2poly, g)

    one = _fresh()
    got = [{k: v.copy() for k, v in run(one, kind, g).items()} for kind, g in steps]
    one.close()
    for i, (kind, g) in enumerate(steps):
        ctx = _fresh()
        _bytes_equal(got[i], run(ctx, kind, g), "step %d" % i)
        ctx.close()
    assert got[4]["res"].shape == (0,) and got[4]["status"].shape == (0,)
    assert len(got[0]["res"]) == 120 and len(got[2]["res"]) == 128
    _bytes_equal(got[5], got[0], "K = 16 plane_yz after the other calls")


@pytest.mark.gpu
def test_one_list_equals_the_single_pair_calls():
    """Every group of K = 13 (the any-count build, two-pass split) in one call, with repeated, reversed and a == a pairs,
    permuted: each pair's result is what a call of that pair alone gives."""
    ctx = _capi().scratch_context()
    g, _ = C.list_case(13)
    whole = {k: v.copy() for k, v in C.run_curves(ctx.coll_check, g).items()}
    for i, (a, b) in enumerate(zip(g["pa"], g["pb"])):
        one = ctx.coll_check(g["curves"][[a, b]], [0], [1 if a != b else 0], max_nodes=C.MAX_NODES)
        for k in whole:
            assert one[k][0].tobytes() == whole[k][i].tobytes(), "pair %d = (%d, %d): %s %r alone, %r in the list" % (i, a, b, k, one[k][0], whole[k][i])
