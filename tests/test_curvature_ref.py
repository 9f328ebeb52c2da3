"""tests/curvature_ref.py on its own (no device): closed forms, invariances, its search against a dense sample, its envelope
formula against a 50-digit central difference -- and what the curvature family adds to the layers that can be checked without
a device: the ABI entries in the header and in _capi._SIGNATURES, and the key of a kept finite-difference batch."""
import os
import re
import sys
from fractions import Fraction

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curvature_ref as C  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SYMBOLS = ["obtg_curvature_poly", "obtg_curvature_true_min", "obtg_curvature_true_min_jac", "obtg_bern_curvature"]
REL = Fraction(1, 10 ** 12)


def _inside(bracket, value, slack=0):
    return bracket[0] - slack <= value <= bracket[1] + slack


def test_the_parabola():
    """(-1,1),(0,-1),(1,1): y = x^2... in the parameter: kappa = 2 at t = 1/2 (exactly: kappa^2 = 4) and 2 / 5^(3/2) at the ends"""
    assert C.kappa2(C.PARABOLA, 0.5) == (1, Fraction(4))
    assert C.kappa2(C.PARABOLA, 0.0) == (1, Fraction(4, 125)) and C.kappa2(C.PARABOLA, 1.0) == (1, Fraction(4, 125))
    lo, hi = C.curvature_range(C.PARABOLA, REL)
    end = Fraction(2) / (5 * C._isqrt_frac(5, True)), Fraction(2) / (5 * C._isqrt_frac(5, False))
    assert lo[0] <= end[1] and end[0] <= lo[1] and lo[1] - lo[0] <= REL * lo[1]
    assert hi[0] <= 2 <= hi[1] and hi[1] - hi[0] <= 2 * REL
    r = C.certified_max(C.PARABOLA, 0, 1.0, REL)
    assert r['status'] == 'ok' and r['t'] == Fraction(1, 2) and r['L'] <= 2 <= r['H']
    # it never turns right: side 1 is the clamp's 0, from the first step
    r = C.certified_max(C.PARABOLA, 1, 1.0, REL)
    assert (r['L'], r['H'], r['t'], r['nodes']) == (0, 0, 0, 1)


def test_a_straight_line_and_degree_one():
    for yv in (np.array([[0.0, 1.0, 4.0, 10.0], [0.0, 0.25, 1.0, 2.5]]), np.array([[0.0, 2.0], [1.0, 5.0]]), np.zeros((2, 4))):
        num = C.coeffs(yv)[0]
        assert not any(num)
        for side in range(2):
            r = C.certified_max(yv, side, 1.0, REL)
            assert (r['L'], r['H'], r['t'], r['status']) == (0, 0, 0, 'ok')
        assert C.curvature_range(yv) == ((0, 0), (0, 0))


@pytest.mark.parametrize("deg", [2, 3, 5])
def test_elevation_and_mirror_image(deg):
    yv = C.seeded(deg, 3)
    base = C.curvature_range(yv, REL)
    assert base[0][1] <= base[1][0]
    # elev(3) of the same curve, in exact rationals: the same curve, the same range
    P = C._ctrl(yv)
    for _ in range(3):
        n = len(P[0]) - 1
        P = [[r[0]] + [Fraction(i, n + 1) * r[i - 1] + (1 - Fraction(i, n + 1)) * r[i] for i in range(1, n + 1)] + [r[n]] for r in P]
    up = C.curvature_range(P, REL)
    for a, b in zip(base, up):
        assert a[0] <= b[1] and b[0] <= a[1], (a, b)               # the brackets overlap, and both are 1e-12 wide
    # the mirror image (y -> -y) swaps the sides
    mirror = np.stack((yv[0], -yv[1]))
    for side in range(2):
        a, b = C.certified_max(yv, side, 1.0, REL), C.certified_max(mirror, 1 - side, 1.0, REL)
        assert (a['L'], a['H'], a['t'], a['nodes']) == (b['L'], b['H'], b['t'], b['nodes'])
    m = C.curvature_range(mirror, REL)
    assert m[0] == (-base[1][1], -base[1][0]) and m[1] == (-base[0][1], -base[0][0])


@pytest.mark.parametrize("deg", [2, 3, 6, 10])
def test_coefficients_and_search_against_points(deg):
    yv = C.seeded(deg, 1)
    co = C.coeffs(yv)
    for t in (Fraction(0), Fraction(1, 3), Fraction(5, 8), Fraction(1)):
        assert (C._bern(co[0], t), C._bern(co[1], t)) == C.num_den(yv, t)
    assert all(m >= abs(v) for v, m in zip(co[0] + co[1], co[2] + co[3]))
    for side in range(2):
        r = C.certified_max(yv, side, 1.0, Fraction(1, 10 ** 9), co=co)
        assert r['status'] == 'ok' and r['waiting'] <= 32 and r['H'] - r['L'] <= Fraction(1, 10 ** 9) * max(1, r['L'])
        # nothing on a 1025-point sample is above H; the incumbent's point attains L
        assert C.sample_exceeds(yv, side, r['H'], 1025, co=co) == []
        if r['L'] > 0:
            sign, k2 = C.kappa2(yv, r['t'])
            assert sign == C.SIGMA[side] and k2 >= r['L'] ** 2
            assert C.sample_exceeds(yv, side, r['L'] * (1 - Fraction(1, 100)), 1025, co=co) != [] or r['t'] in (0, 1)
        K, M = C.kappa_majorant(yv, r['t'], co=co)
        assert K == 2 * deg + 29 + 2 * deg * C.depth_of(r['t']) and mpmath.isfinite(M) and M >= abs(C.kappa(yv, r['t']))


def test_the_bound_covers_every_coefficient():
    """Two coefficients, (num, den) = (1, 10) and (-0.001, 1): the tangent at the mid-range of den is negative at den = 1, and
    a rule that enforces lambda g_k >= num_k for num_k > 0 alone answers 0.0348, below the curve's 0.0378.  The yardstick's
    bound stands above every sampled value, in either order of the coefficients."""
    for Ns, Ds in (([1000, -1], [10, 1]), ([-1, 1000], [1, 10])):
        ub = C._node_bound(Ns, Ds, Fraction(1, 1000), True)
        top = max((Ns[0] * (1 - t) + Ns[1] * t) / 1000.0 / (Ds[0] * (1 - t) + Ds[1] * t) ** 1.5 for t in np.linspace(0.0, 1.0, 2001))
        assert top > 0.0377 and ub >= top


def test_a_curve_whose_speed_varies_widely():
    """curvature_ref.WIDE_SPEED: on the root node max den_k > 5 min den_k; side 1's maximum is 0.034917 near t = 0.0462, not the
    0.02801 at t = 1, at every tolerance; nothing on the 4097-point sample is above H, something is above 0.0349."""
    yv = C.WIDE_SPEED
    co = C.coeffs(yv)
    assert max(co[1]) > 5 * min(co[1])            # (some den_k are even below 0 on the root node: the hull is wider than the curve)
    values = C.sample_values(yv, 4097, co)
    for rel in (Fraction(1, 10 ** 6), Fraction(1, 10 ** 9), Fraction(1, 10 ** 12)):
        r = C.certified_max(yv, 1, 1.0, rel, co=co)
        assert r['status'] == 'ok' and r['waiting'] <= 32 and r['H'] - r['L'] <= rel
        assert Fraction(34917, 10 ** 6) < r['L'] and r['H'] < Fraction(34918, 10 ** 6) and abs(r['t'] - Fraction(462, 10 ** 4)) < Fraction(1, 1000)
        assert C.sample_exceeds(yv, 1, r['H'], values=values) == []
    assert C.sample_exceeds(yv, 1, Fraction(349, 10 ** 4), values=values) != []


@pytest.mark.parametrize("deg", [3, 4, 6])
def test_the_search_on_curves_whose_speed_varies_widely(deg):
    """control points N(0, 1): den varies by more than 5x across the root node (and across many nodes below it).  Where the
    search ends, nothing on a 1025-point sample is above H, for both sides, and the point it names attains L."""
    ended = wide = 0
    for seed in range(6):
        yv = C.wild(deg, seed)
        co = C.coeffs(yv)
        wide += max(co[1]) > 5 * min(co[1])
        values = C.sample_values(yv, 1025, co)
        for side in range(2):
            r = C.certified_max(yv, side, 1.0, Fraction(1, 10 ** 9), max_nodes=4000, co=co)
            if r['status'] != 'ok':
                continue                      # (a curve that nearly stops may run out of nodes: no bracket is claimed then)
            ended += 1
            assert C.sample_exceeds(yv, side, r['H'], values=values) == [], (deg, seed, side)
            if r['L'] > 0:
                assert C.kappa2(yv, r['t'])[1] >= r['L'] ** 2
    assert wide == 6 and ended >= 8, (wide, ended)


@pytest.mark.parametrize("deg,t", [(2, 0.5), (3, 0.0), (5, 0.3125), (5, 1.0), (10, 0.71875)])
def test_envelope_formula_against_a_central_difference(deg, t):
    """every entry of the block against (row(P + h e) - row(P - h e)) / 2h at 50 digits, h = 2^-60 on exact rationals"""
    yv = C.seeded(deg, 2)
    h = Fraction(1, 2 ** 60)
    P = C._ctrl(yv)
    K, M = C.block_majorant(yv, t)
    assert K == 20 * deg + 21
    for side in range(2):
        blk = C.envelope_block(yv, side, t)
        for c in range(2):
            for i in range(deg + 1):
                up, dn = [list(r) for r in P], [list(r) for r in P]
                up[c][i] += h
                dn[c][i] -= h
                fd = -C.SIGMA[side] * (C.kappa(up, t) - C.kappa(dn, t)) / (2 * C._mp(h))
                scale = max(abs(v) for row in blk for v in row)
                assert abs(fd - blk[c][i]) <= mpmath.mpf(10) ** -30 * scale, (side, c, i)
                assert mpmath.isfinite(M[c][i]) and M[c][i] >= abs(blk[c][i])


# ------------------------------------------------------------------------------------------------ the other layers, without a device
def test_abi_entries():
    from optimalbeziertrajectorygeneration_amd import _capi
    header = open(os.path.join(ROOT, "include", "obtg.h")).read()
    capi = open(os.path.join(ROOT, "optimalbeziertrajectorygeneration_amd", "csrc", "capi.cpp")).read()
    for base in SYMBOLS:
        for name in (base, base + "_dev"):
            assert re.search(r"\bint %s\(obtg_ctx\*" % name, header), name
            assert name + "\\0" in capi and re.search(r"^int %s\(obtg_ctx\* c" % name, capi, re.M), name
            assert name in _capi._SIGNATURES and name in _capi.abi_symbol_names()
    assert "OBTG_K_COUNT = 9" in header and "OBTG_K_END = 10" in header
    # nothing takes tf: Y, B, (max_curv, eps_rel, max_nodes,) then outputs
    assert len(_capi._SIGNATURES["obtg_curvature_poly"][1]) == 4
    assert len(_capi._SIGNATURES["obtg_curvature_true_min"][1]) == 9
    assert len(_capi._SIGNATURES["obtg_curvature_true_min_jac_dev"][1]) == 10
    assert len(_capi._SIGNATURES["obtg_bern_curvature"][1]) == 11
    for method in ("curvature_poly", "curvature_poly_dev", "curvature_true_min", "curvature_true_min_dev", "curvature_true_min_jac",
                   "curvature_true_min_jac_dev", "bern_curvature"):
        assert callable(getattr(_capi.Context, method)), method


def _problem(**kw):
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    return opt.BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal='TimeOpt', maxSep=0.9, maxSpeed=5.0, maxAngRate=1.0,
                               initPoints=[(0, 0), (1, 3)], finalPoints=[(6, 1), (7, 4)], tf=8.0, **kw)


def test_serve_key_only_sees_a_curvature_bound_that_is_set():
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    assert ('maxCurvature', 'maxCurvature', None) in opt._MODEL_FIELDS and opt._FAMILY['curv'].rows is None
    assert _problem(maxCurvature=0.5).model['maxCurvature'] == 0.5
    bound = _problem()                                    # (one problem throughout: the model's byte key holds object identities)
    assert bound.model['maxCurvature'] is None
    k0 = bound._serve_key(True)
    bound.model['maxCurvature'] = 0.5
    k1 = bound._serve_key(True)
    assert len(k0) == 17 and k1[:17] == k0 and k1[17:] == (('maxCurvature', 0.5),)
    bound.model['maxCurvature'] = 0.25                    # an edited bound: a kept batch must not be served
    k2 = bound._serve_key(True)
    assert k2 != k1 and k2[:17] == k0
    bound.model['maxCurvature'] = None
    assert bound._serve_key(True) == k0
    assert 'curvatureRows' not in opt.BezOptimization.__init__.__code__.co_varnames and opt._ROWS_OPTIONS == (
        'speedRows', 'angRateRows', 'accelRows', 'jerkRows')
