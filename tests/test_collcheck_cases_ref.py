"""What tests/collcheck_cases.py reaches, by the restatement alone (no GPU): the conditions without which
tests/test_gpu_collcheck_forms.py would compare little, and the restatement held to what the reference itself returned on
the forms tests/golden/collcheck.npz does not hold (tests/golden/collcheck_forms.npz).

Figures of the restatement on these cases (printed by the tests; max_nodes 600, 120 pairs a curve group, 128 a polygon group):

  curve form, share of MD_OK / MD_OK pairs of depth >= 50 / results of -1 / runs of 600 nodes, per K:
    planar = minus_zero = plane_z1 (identical to the restatement at every K; every other end is MD_GJK_CAP, none MD_NODE_CAP)
        K = 13: 79.2 %, 25 deep;  K = 14: 77.5 %, 31 deep (the lowest shares);  K = 16: 88.3 %, 15 deep, one -1;
        K = 10 and 12: 90.8 %;  every other K >= 93.3 %;  K = 2: 100 %, exactly 2 deep pairs;  K >= 3: 9 .. 31 deep
    plane_yz (no MD_GJK_CAP at all: every other end is MD_NODE_CAP)
        K = 13: 93.3 % (the lowest), 42 deep, 6 x -1, 8 runs of 600;  K = 14: 95.0 %, 52 deep, 6 x -1, 6 runs
        K = 4: 96.7 %, 20 deep, 2 x -1, 4 runs;  K = 7: 94.2 %, 11 deep, 1 x -1, 7 runs;  K = 5: 99.2 %, 10 deep, 1 run
        K = 2: 100 %, 2 deep, most nodes 409;  K = 3: 99.2 %, 9 deep, the first run of 600
        over every K: 21 results of -1, 44 runs of 600 nodes
  polygon form: 100 % MD_OK everywhere; pairs of depth 100 (= results of 0) in planar / plane_z1: 12 (K = 2) .. 54 (K = 13),
    in plane_yz 19 (K = 2) .. 67 (K = 13); most nodes 468; `mixed`: 128 x 1 at the root
  parameters (planar K = 6; defaults: 96.7 % OK, 94 x 1, 17 x 0.0, 5 other, 4 MD_GJK_CAP, most nodes 233):
    eps 0 and 0.5: the defaults' results;  eps 1 and 2: nodes == 1 everywhere (80 x 1, 40 end-point distances)
    max_iter 1: 82 x -1 (depth 100, most nodes 405), 38 x 1;  3: 5 MD_GJK_CAP, most nodes 421;  6: the defaults' results
    md_cap 1: 106 MD_GJK_CAP;  4: 39;  16: the defaults' results
    polygon form (defaults 90 x 1, 38 x 0): max_iter 1: 35 x 1, 93 x 0;  3: 86 / 42;  md_cap 1: 93 MD_GJK_CAP;  4: 8
  budget edges: the curve pair ends MD_OK after N = 233 nodes at depth 57 (0.0); the polygon pair after N = 100 at depth 100 (0)
  non-finite, curve form (27 plantings x 4 pairs that hold the planted curve): 72 x -1 after 397 nodes at depth 100,
    24 x 1 at the root, 9 x 0.0 at the root (the pair (1, 1)), and 3 x 1 after 5 nodes at depth 2 (-inf in x of control
    point 0); the untouched pair (2, 3) is 1.  Polygon form (36 cases): 18 x 1 at the root, 1 x 1 after 3 nodes,
    17 x 0 at depth 100 (100, 124 or 199 nodes).  All MD_OK.
  the reference's records (collcheck_forms.npz): it finished all 171 non-finite cases, 20 of planar_K13's 24 (4 are
    MD_GJK_CAP here), all 48 of plane_yz (most calls 705) and answered 1 at the root for the six crossing pairs in z = x;
    the restatement returns its value after its number of gjkNew calls on every finished case.
CPU time: about half a minute for this file.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collcheck_cases as C  # noqa: E402
import collcheck_ref as R  # noqa: E402

FORMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collcheck_forms.npz")
DEEP = 50
# node budget for the recorded cases: far above what any case the reference finished in its time budget visits
RECORD_BUDGET = 20000


def _eq(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def _line(r):
    ok = r["status"] == R.MD_OK
    return "OK %5.1f %%, 1: %3d, 0: %3d, -1: %2d, other %2d, node cap %2d, gjk cap %2d, deep OK pairs %2d, depth 100: %2d, most nodes %3d" % (
        100 * ok.mean(), (ok & (r["res"] == 1)).sum(), (ok & (r["res"] == 0)).sum(), (ok & (r["res"] == -1)).sum(),
        (ok & (r["res"] != 1) & (r["res"] != 0) & (r["res"] != -1)).sum(), (r["status"] == R.MD_NODE_CAP).sum(),
        (r["status"] == R.MD_GJK_CAP).sum(), (ok & (r["depth"] >= DEEP)).sum(), (r["depth"] == 100).sum(), r["nodes"].max())


@pytest.mark.parametrize("K", C.KS)
def test_curve_groups_end_ok_and_walk_deep(K):
    """Conditions 1 and 2 per curve-form group: at least 75 % MD_OK; at least 2 MD_OK pairs of depth >= 50 in `planar`,
    `plane_z1` and `plane_yz`; `minus_zero` is `planar` to the restatement."""
    for placing in C.PLACINGS:
        r = C.ref_curve_group(K, placing)
        print("K=%2d %-10s %s" % (K, placing, _line(r)))
        ok = r["status"] == R.MD_OK
        assert ok.mean() >= 0.75, (K, placing)
        assert (ok & (r["depth"] >= DEEP)).sum() >= 2, (K, placing)
        assert (r["nodes"] == r["gjk_calls"]).all() and (r["res"][~ok] == 0).all()
    assert _eq(C.ref_curve_group(K, "minus_zero"), C.ref_curve_group(K, "planar")), K


@pytest.mark.parametrize("K", C.KS)
def test_polygon_groups_end_ok_and_walk_to_the_bottom(K):
    """Every polygon group is 100 % MD_OK; each of the four in the curves' plane has at least 12 pairs of depth 100; planar
    curves against polygons at z = 1 are apart at the root, all 128."""
    for placing in C.POLY_PLACINGS:
        r = C.ref_poly_group(K, placing)
        print("K=%2d %-10s %s" % (K, placing, _line(r)))
        assert (r["status"] == R.MD_OK).all(), (K, placing)
        assert np.isin(r["res"], (0.0, 1.0)).all()
        if placing == "mixed":
            assert (r["res"] == 1).all() and (r["nodes"] == 1).all(), K
        else:
            assert (r["depth"] == 100).sum() >= 12, (K, placing)
    assert _eq(C.ref_poly_group(K, "minus_zero"), C.ref_poly_group(K, "planar")), K
    g = C.poly_group(K, "planar")
    assert np.diff(g["off"]).tolist() == list(C.POLY_SIZES)
    assert C.ref_poly_group(K, "planar")["res"][0] == 0          # curve 0 starts on polygon 0's one vertex


def test_plane_yz_reaches_minus_one_and_the_node_cap():
    r = [C.ref_curve_group(K, "plane_yz") for K in C.KS]
    n_m1 = sum(int(((x["status"] == R.MD_OK) & (x["res"] == -1)).sum()) for x in r)
    n_cap = sum(int((x["status"] == R.MD_NODE_CAP).sum()) for x in r)
    print("plane_yz over every K: %d results of -1, %d runs of %d nodes" % (n_m1, n_cap, C.MAX_NODES))
    assert n_m1 >= 1 and n_cap >= 1
    for x in r:
        assert (x["nodes"][x["status"] == R.MD_NODE_CAP] == C.MAX_NODES).all()


def test_parameters_change_something():
    """Condition 3, on the planar base of K = 6."""
    d = C.ref_curve_params(-1)
    by = {}
    for i, kw in enumerate(C.CURVE_PARAMS):
        r = by[tuple(kw.items())[0]] = C.ref_curve_params(i)
        print("curve form %-14s %s" % (kw, _line(r)))
    print("curve form %-14s %s" % ("defaults", _line(d)))
    for eps in (1.0, 2.0):
        assert (by[("eps", eps)]["nodes"] == 1).all() and (by[("eps", eps)]["status"] == R.MD_OK).all()
    assert _eq(by[("eps", 0.5)], d)
    assert ((by[("max_iter", 1)]["status"] == R.MD_OK) & (by[("max_iter", 1)]["res"] == -1)).sum() >= 1
    assert (by[("md_cap", 4)]["status"] == R.MD_GJK_CAP).sum() > (d["status"] == R.MD_GJK_CAP).sum()
    dp = C.ref_poly_params(-1)
    print("polygon form %-12s %s" % ("defaults", _line(dp)))
    changed = 0
    for i, kw in enumerate(C.POLY_PARAMS):
        r = C.ref_poly_params(i)
        print("polygon form %-12s %s" % (kw, _line(r)))
        changed += not _eq(r, dp)
    assert changed >= 2


def test_budget_edges():
    """Condition 4: max_nodes = N + 1 and N give the pair's own answer after N nodes, N - 1 and 1 give MD_NODE_CAP after
    exactly that many."""
    b = C.budget_curve_case()
    print("curve form: N = %d at depth %d, value %r" % (b["N"], b["depth"], b["res"]))
    assert b["N"] >= 100 and b["depth"] >= DEEP
    p = C.budget_poly_case()
    print("polygon form: N = %d at depth %d, value %r" % (p["N"], p["depth"], p["res"]))
    assert p["N"] == 100 and p["depth"] == 100 and p["res"] == 0 and p["status"] == R.MD_OK
    for case, fn in ((b, lambda m: R.coll_check(b["curves"][0], b["curves"][1], max_nodes=m)),
                     (p, lambda m: R.coll_check2poly(p["curves"][0], p["pts"], max_nodes=m))):
        N = case["N"]
        for m in C.budgets(N):
            r = fn(m)
            if m >= N:
                assert (r["status"], r["nodes"], r["depth"], r["res"]) == (R.MD_OK, N, case["depth"], case["res"]), m
            else:
                assert (r["status"], r["nodes"], r["gjk_calls"], r["res"]) == (R.MD_NODE_CAP, m, m, 0.0), m


def test_non_finite_input_has_definite_answers():
    """Condition 4: every non-finite case ends MD_OK -- 1 at the root, 0.0 at the root, or -1 at depth 100 -- and the pair
    that does not hold the planted curve is 1."""
    names = [n for n, _ in C.nonfinite_curve_cases()]
    kinds = {}
    for name, r in zip(names, C.ref_nonfinite_curves()):
        assert (r["status"] == R.MD_OK).all(), name
        assert r["res"][C.NF_UNTOUCHED] == 1, name
        for k in range(5):
            if k == C.NF_UNTOUCHED:
                continue
            root = r["nodes"][k] == 1
            key = (float(r["res"][k]), bool(root))
            assert r["res"][k] in (1.0, 0.0, -1.0) and (r["res"][k] != 0 or root), (name, k, r)
            assert r["res"][k] != -1 or (r["depth"][k] == 100 and r["nodes"][k] == 397), (name, k, r)
            kinds.setdefault(key, []).append((name, k, int(r["nodes"][k])))
    for key, v in sorted(kinds.items()):
        print("curve form (value, at the root) = %s: %d searches, nodes %s" % (key, len(v), sorted(set(n for _, _, n in v))))
    assert (1.0, True) in kinds and (-1.0, False) in kinds
    pk = {}
    for (name, _, _), r in zip(C.nonfinite_poly_cases(), C.ref_nonfinite_polys()):
        assert (r["status"] == R.MD_OK).all() and r["res"][0] in (0.0, 1.0), name
        pk.setdefault((float(r["res"][0]), int(r["nodes"][0]), int(r["depth"][0])), []).append(name)
    for key, v in sorted(pk.items()):
        print("polygon form (value, nodes, depth) = %s: %d cases" % (key, len(v)))


def test_list_case_is_the_groups_and_more():
    g, ref = C.list_case(13)
    n = len(g["pa"])
    assert n == 4 * (120 + 2 * C.N_LIST_EXTRA + 4) and g["curves"].shape == (64, 3, 13)
    assert (g["pa"] == g["pb"]).sum() == 16
    pairs = set(zip(g["pa"].tolist(), g["pb"].tolist()))
    assert sum((b, a) in pairs for a, b in pairs if a != b) == 2 * 4 * C.N_LIST_EXTRA
    assert len(pairs) == n - 4 * C.N_LIST_EXTRA
    i = np.random.default_rng(1).choice(n, 40, replace=False)
    direct = R.coll_check_pairs(g["curves"], g["pa"][i], g["pb"][i], max_nodes=C.MAX_NODES)
    assert _eq(direct, {k: ref[k][i] for k in ref})


# ------------------------------------------------------------------------------------------------ the reference's own records
def _recorded(gold, kind):
    keys = ("curves", "pa", "pb", "pts", "off", "pc", "pp", "fin", "val", "calls")
    for name in gold[kind + "_groups"]:
        name = str(name)
        yield name, {k: gold[name + "_" + k] for k in keys if name + "_" + k in gold.files}


def test_recorded_inputs_are_the_cases():
    gold = np.load(FORMS)
    cc, cp = C.recorded_groups()
    assert [n for n, _ in _recorded(gold, "cc")] == [x[0] for x in cc]
    assert [n for n, _ in _recorded(gold, "cp")] == [x[0] for x in cp]
    for (name, g), (_, curves, pa, pb, _p) in zip(_recorded(gold, "cc"), cc):
        assert g["curves"].tobytes() == np.ascontiguousarray(curves).tobytes(), name
        assert (g["pa"] == pa).all() and (g["pb"] == pb).all(), name
    for (name, g), (_, curves, polys, pc, pp, _p) in zip(_recorded(gold, "cp"), cp):
        assert g["curves"].tobytes() == np.ascontiguousarray(curves).tobytes(), name
        assert g["pts"].tobytes() == np.vstack(polys).tobytes(), name


@pytest.mark.parametrize("kind", ["cc", "cp"])
def test_restatement_is_the_reference_on_the_recorded_forms(kind):
    """Value and gjkNew-call count wherever the reference finished; the status alone where it did not."""
    gold = np.load(FORMS)
    n = 0
    for name, g in _recorded(gold, kind):
        if kind == "cc":
            r = R.coll_check_pairs(g["curves"], g["pa"], g["pb"], max_nodes=RECORD_BUDGET)
        else:
            r = R.coll_check2poly_pairs(g["curves"], g["pts"], g["off"], g["pc"], g["pp"], max_nodes=RECORD_BUDGET)
        fin = g["fin"] == 0
        print("%-14s %3d cases, the reference finished %3d: %d x 1, %d x 0, %d x -1, %d other; most calls %d" % (
            name, len(fin), fin.sum(), (g["val"][fin] == 1).sum(), (g["val"][fin] == 0).sum(), (g["val"][fin] == -1).sum(),
            ((g["val"][fin] != 1) & (g["val"][fin] != 0) & (g["val"][fin] != -1)).sum(), g["calls"].max()))
        assert (r["status"][fin] == R.MD_OK).all(), (name, np.flatnonzero(fin & (r["status"] != R.MD_OK)))
        assert r["res"][fin].tobytes() == g["val"][fin].tobytes(), (name, r["res"][fin], g["val"][fin])
        assert (r["gjk_calls"][fin] == g["calls"][fin]).all(), (name, r["gjk_calls"][fin], g["calls"][fin])
        assert (r["status"][~fin] != R.MD_OK).all() and (r["res"][~fin] == 0).all(), name
        n += int(fin.sum())
        if name.startswith("nf"):
            assert fin.all(), name                     # the reference comes back from every non-finite case
        if name == "shear_zx_K4":
            assert fin.all() and (g["val"] == 1).all()      # crossing curves in a sheared plane: the 1 is the reference's
    assert n >= 30
