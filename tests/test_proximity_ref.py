"""CPU side of the proximity rows (obtg_proximity_poly, obtg_proximity_true[_jac], BezOptimization(waypoints=.., stayWithin=..)):
the two layers of proximity_ref.py held to each other and to plain evaluations, what the batch of the GPU tests holds (from the
yardstick alone), the ABI bookkeeping and the constructor's checks.  No GPU."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proximity_ref as PR  # noqa: E402
import extrema_ref as R  # noqa: E402

_cases = {}


def cases(dim, deg):
    if (dim, deg) not in _cases:
        bt = PR.batch(dim, deg)
        _cases[(dim, deg)] = (bt, PR.batch_cases(bt))
    return _cases[(dim, deg)]


def _bern_eval(c, t):
    c = list(c)
    while len(c) > 1:
        c = [(1 - t) * c[i] + t * c[i + 1] for i in range(len(c) - 1)]
    return c[0]


@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_batch_holds_every_case(dim, deg):
    """Every configuration's batch holds all eight combinations of kind x target x window and, by the yardstick: an item whose
    search has to split, a negative and a positive row of each kind, an extremum at a window end that is interior to the curve,
    and one at tau = 0 or 1."""
    bt, c = cases(dim, deg)
    combos = {(int(it[2]), int(it[1]) < PR.N_VEH, (w[1], w[2]) == (0.0, 1.0)) for it, w in zip(bt["items"], bt["params"])}
    assert len(combos) == 8
    assert bt["Y"].shape == (4, 3 * dim, deg + 1) and bt["pts"].shape == (2, dim) and len(bt["items"]) == 8
    assert c["splits"] >= 1
    for kind in (PR.WITHIN, PR.REACH):
        assert c["neg"][kind] >= 1 and c["pos"][kind] >= 1, (kind, c["neg"], c["pos"])
    assert c["window_end"] >= 1 and c["curve_end"] >= 1


@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_batch_holds_items_with_a_unique_interior_extremum(dim, deg):
    """Every configuration's batch holds at least two items whose extremum lies strictly inside the window in one basin
    (proximity_ref.unique_interior, from the float rows alone) -- the items on which the GPU test holds the blocks to a central
    difference of the exact extremum -- and the exact layer agrees that their extremum is interior."""
    bt, c = cases(dim, deg)
    todo = PR.unique_interior_items(bt, c["rows"])
    assert len(todo) >= 2, todo
    for r, p in todo:
        assert 0 < c["truth"][r * len(bt["items"]) + p]["t"] < 1, (r, p)


@pytest.mark.parametrize("dim,deg", PR.CONFIGS)
def test_float_layer_within_its_allowance_of_the_exact_layer(dim, deg):
    """Every float coefficient is within K 2^-53 M of the exact one (the allowance's search term only widens it), for both
    formations; and the exact polynomial IS (d/2)(rho^2 - |c_a - c_b|^2) at points of the window, from plain de Casteljau."""
    bt, c = cases(dim, deg)
    Y, pts = bt["Y"], bt["pts"]
    worst = Fraction(0)
    for r in range(Y.shape[0]):
        for p, (it, pr) in enumerate(zip(bt["items"], bt["params"])):
            ex = PR.item_exact(Y[r], pts, dim, PR.N_VEH, it, pr)
            al = PR.allowance(Y[r], pts, dim, PR.N_VEH, it, pr)
            for k, v in enumerate(c["rows"][r, p]):
                worst = max(worst, abs(Fraction(float(v)) - ex[k]) / al)
            if r == 0:
                ya, yb, _ = PR._pair(Y[r], pts, dim, PR.N_VEH, int(it[0]), int(it[1]))
                _, zh, _, zt = PR._cuts(float(pr[1]), float(pr[2]))
                tau0 = Fraction(float(pr[1]))
                tau1 = tau0 + Fraction(zt) * (1 - tau0) if float(pr[2]) < 1.0 else Fraction(1)
                for s in (Fraction(0), Fraction(3, 8), Fraction(1)):
                    tau = tau0 + s * (tau1 - tau0)
                    d2 = sum((_bern_eval(PR._fr(ya[q]), tau) - _bern_eval(PR._fr(yb[q]), tau)) ** 2 for q in range(dim))
                    assert _bern_eval(ex, s) == Fraction(dim, 2) * (Fraction(float(pr[0])) ** 2 - d2)
    print("worst |float - exact| / allowance: %.3g" % float(worst))
    assert worst <= 1


def test_exact_search_agrees_with_extrema_ref_on_float_rows():
    """certified_min_exact is extrema_ref.certified_min where both apply: the same bracket, parameter and node count"""
    rng = np.random.RandomState(5)
    for K in (2, 5, 12):
        for _ in range(4):
            c = rng.uniform(-1, 1, K)
            a, b = R.certified_min(c), PR.certified_min_exact([Fraction(float(x)) for x in c])
            assert (a["L"], a["H"], a["t"], a["nodes"]) == (b["L"], b["H"], b["t"], b["nodes"])
            mx, my = R.certified_max(c), PR.extremum_exact([Fraction(float(x)) for x in c], PR.REACH)
            assert (mx["L"], mx["H"], mx["t"]) == (my["L"], my["H"], my["t"])


def test_full_window_takes_no_cut_and_fma_is_one_rounding():
    assert PR._cuts(0.0, 1.0)[0] is False and PR._cuts(0.0, 1.0)[2] is False
    assert PR._cuts(0.25, 0.75) == (True, 0.25, True, (0.75 - 0.25) / (1.0 - 0.25))
    assert PR.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60      # the product alone would lose 2^-60
    assert PR.curve_t(0.5, 0.25, 0.75) == 0.5 and PR.curve_t(1.0, 0.0, 1.0) == 1.0


@pytest.mark.parametrize("dim,deg", [(2, 3), (3, 5)])
def test_envelope_restatement_is_the_derivative_of_g(dim, deg):
    """The float block is, to rounding, the exact partial derivative of g at t: -d B_i(t) (c_a - c_b)_c(t)"""
    bt, _ = cases(dim, deg)
    y, pts = bt["Y"][0], bt["pts"]
    t = 0.3125
    for it in bt["items"]:
        blk = PR.envelope_float(y, pts, dim, PR.N_VEH, it, t)
        ya, yb, _ = PR._pair(y, pts, dim, PR.N_VEH, int(it[0]), int(it[1]))
        for c in range(dim):
            dl = _bern_eval(PR._fr(ya[c]), Fraction(t)) - _bern_eval(PR._fr(yb[c]), Fraction(t))
            for i in range(deg + 1):
                e = [Fraction(0)] * (deg + 1)
                e[i] = Fraction(1)
                want = -dim * _bern_eval(e, Fraction(t)) * dl
                assert abs(Fraction(float(blk[c, i])) - want) <= Fraction(1, 10 ** 13)


NEW_SYMBOLS = ("obtg_ctx_set_proximity", "obtg_len_proximity", "obtg_proximity_poly", "obtg_proximity_poly_dev", "obtg_proximity_true",
               "obtg_proximity_true_dev", "obtg_proximity_true_jac", "obtg_proximity_true_jac_dev")


def test_library_exports_the_proximity_rows():
    """The eight names are in the header, the library, obtg_abi_symbols and the binding table.  New symbols alone do not move
    the ABI number (every sibling family's test holds it at 7)."""
    import ctypes as C
    from optimalbeziertrajectorygeneration_amd import _capi, build
    lib = C.CDLL(build.build())
    lib.obtg_abi_symbols.restype = C.POINTER(C.c_char)
    p, syms, i = lib.obtg_abi_symbols(), [], 0
    while True:
        s = b""
        while p[i] != b"\0":
            s += p[i]
            i += 1
        i += 1
        if not s:
            break
        syms.append(s.decode())
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "obtg.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in syms, name
        assert name in _capi.abi_symbol_names(), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "Later, still 7: new: the proximity rows" in header
    assert "#define OBTG_PROX_WITHIN 0" in header and "#define OBTG_PROX_REACH 1" in header
    assert (_capi.PROX_WITHIN, _capi.PROX_REACH) == (PR.WITHIN, PR.REACH) == (0, 1)
    for m in ("set_proximity", "len_proximity", "proximity_poly", "proximity_poly_dev", "proximity_true", "proximity_true_jac",
              "proximity_true_dev"):
        assert hasattr(_capi.Context, m), m


# ------------------------------------------------------------------------------------------------ the constructor's checks
def test_constructor_messages_and_tables():
    """Every refusal of _proximity_tables, in its words; the rows are the waypoints in list order, then the stayWithin entries;
    both lists are kept on the object."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    kw = dict(numVeh=2, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=1, maxSpeed=5, tf=10.0,
              initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)])
    good = (0, (1.0, 2.0), 0.5)
    bad = [
        ("abc", "waypoints must be a list of entries"),
        ([], "waypoints must be a list of entries"),
        ([(0, 1)], r"waypoints\[0\] must be \(vehicle, target, radius\)"),
        ([good, 7], r"waypoints\[1\] must be \(vehicle, target, radius\)"),
        ([(2, (1.0, 2.0), 0.5)], r"waypoints\[0\] needs a vehicle index in 0 .. 1, not 2"),
        ([(0.0, (1.0, 2.0), 0.5)], r"waypoints\[0\] needs a vehicle index in 0 .. 1"),
        ([(0, 0, 0.5)], r"waypoints\[0\] needs another vehicle's index in 0 .. 1 as its target, not 0"),
        ([(0, 2, 0.5)], r"waypoints\[0\] needs another vehicle's index"),
        ([(0, (1.0, 2.0, 3.0), 0.5)], r"waypoints\[0\] needs a target that is a vehicle index or a finite point of dimension 2"),
        ([(0, (1.0, np.nan), 0.5)], r"waypoints\[0\] needs a target that is a vehicle index or a finite point"),
        ([(0, "p", 0.5)], r"waypoints\[0\] needs a target that is a vehicle index or a finite point"),
        ([(0, 1, 0.0)], r"waypoints\[0\] needs a finite radius > 0, not 0.0"),
        ([(0, 1, -1.0)], r"waypoints\[0\] needs a finite radius > 0"),
        ([(0, 1, np.inf)], r"waypoints\[0\] needs a finite radius > 0"),
        ([(0, 1, "r")], r"waypoints\[0\] needs a finite radius > 0"),
        ([(0, 1, 0.5, (0.5, 0.5))], r"waypoints\[0\] needs a window \(tau0, tau1\) with 0 <= tau0 < tau1 <= 1"),
        ([(0, 1, 0.5, (-0.1, 0.5))], r"waypoints\[0\] needs a window"),
        ([(0, 1, 0.5, (0.5, 1.5))], r"waypoints\[0\] needs a window"),
        ([(0, 1, 0.5, (np.nan, 1.0))], r"waypoints\[0\] needs a window"),
        ([(0, 1, 0.5, 0.5)], r"waypoints\[0\] needs a window"),
    ]
    for arg, msg in bad:
        with pytest.raises(ValueError, match=msg):
            BezOptimization(waypoints=arg, **kw)
        with pytest.raises(ValueError, match=msg.replace("waypoints", "stayWithin")):
            BezOptimization(stayWithin=arg, **kw)
    with pytest.raises(ValueError, match="waypoints and stayWithin need dimension 2 or 3, not 1"):
        opt._proximity_tables([good], None, 2, 1)
    with pytest.raises(ValueError, match="both None"):
        opt._proximity_tables(None, None, 2, 2)
    wp, st = [good, (1, 0, 2.0, (0.5, 1.0))], [(0, 1, 8.0), (1, (3.0, 4.0), 6.0, (0.0, 0.25))]
    bo = BezOptimization(waypoints=wp, stayWithin=st, **kw)
    assert bo.waypoints is wp and bo.stayWithin is st
    items, params, pts = opt._proximity_tables(wp, st, 2, 2)
    assert items.dtype == np.int32 and items.tolist() == [[0, 2, 1], [1, 0, 1], [0, 1, 0], [1, 3, 0]]
    assert params.tolist() == [[0.5, 0.0, 1.0], [2.0, 0.5, 1.0], [8.0, 0.0, 1.0], [6.0, 0.0, 0.25]]
    assert pts.tolist() == [[1.0, 2.0], [3.0, 4.0]]
    assert opt._FAMILY['proximity'] is opt._PROXIMITY and opt._PROXIMITY.rows is None and opt._PROXIMITY.span is False
    assert opt._PROXIMITY not in opt._ROW_FAMILIES
    only = BezOptimization(stayWithin=st, **kw)
    assert opt._proximity_tables(None, st, 2, 2)[0][:, 2].tolist() == [0, 0] and only.waypoints is None
