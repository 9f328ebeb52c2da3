"""tests/space_curvature_ref.py held to what it can be held to without a device: curvature_ref.py's planar search on lifted
planar curves, a known-wrong bound it must reject, the block's rational form against differences in exact rationals, and
the degenerate rows."""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curvature_ref as C  # noqa: E402
import space_curvature_ref as S  # noqa: E402

REL = Fraction(1, 10 ** 9)


def test_the_rotation_is_a_rotation():
    R = S.ROTATION
    for i in range(3):
        for j in range(3):
            assert sum(R[i][k] * R[j][k] for k in range(3)) == (1 if i == j else 0)
    assert (R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0])
            + R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0])) == 1


@pytest.mark.parametrize("deg,seed", [(2, 0), (3, 1), (5, 0), (5, 3), (8, 2), (10, 1)])
def test_lifted_planar_curves_meet_the_planar_search(deg, seed):
    """a planar curve under the exact rational rotation and a translation: kappa in space is |kappa| in the plane, so the
    bracket here contains max(|k_min|, |k_max|) of curvature_ref.py's search -- up to the two brackets' widths"""
    planar = C.seeded(deg, seed) if deg > 2 else C.PARABOLA
    space = S.lift(planar)
    # the exact coefficients agree first: |w|^2 = num^2 and den = den, coefficient for coefficient of the squares' sums
    w, den = S.coeffs(space)[:2]
    num2, den2 = C.coeffs(planar)[:2]
    assert den == den2
    # w = R (0, 0, num): the third column of the rotation times num
    for c in range(3):
        assert w[c] == [S.ROTATION[c][2] * v for v in num2]
    r = S.certified_max(space, 0.0, REL)
    (kmin_lo, kmin_hi), (kmax_lo, kmax_hi) = C.curvature_range(planar, REL)
    assert r['status'] == 'ok'
    lo, hi = max(-kmin_hi, kmax_lo), max(-kmin_lo, kmax_hi)           # the bracket of max |kappa| from the planar search
    assert r['L'] <= hi and lo <= r['H'], (float(r['L']), float(r['H']), float(lo), float(hi))
    assert r['H'] - r['L'] <= REL * r['L'] and hi - lo <= 2 * REL * hi
    # and the value met is kappa at the point the search names
    assert abs(mpmath.sqrt(C._mp(S.kappa2(space, r['t']))) - C._mp(r['L'])) <= mpmath.mpf(2) ** -60 * C._mp(r['L'])


def _unguarded(yv, rel, max_nodes=4000):
    """The device's search in floats with the KNOWN-WRONG bound: the tangent of den^(3/2) at the mid-range of den taken
    whatever its sign at the smallest den_k, coefficients whose g_k is not positive left out of the largest ratio.  Returns
    the maximum it reports."""
    w, den = S.coeffs(yv)[:2]
    co = [np.array([float(v) for v in row]) for row in (w[0], w[1], w[2], den)]

    def kap(c, i):
        return np.sqrt(c[0][i] ** 2 + c[1][i] ** 2 + c[2][i] ** 2) / c[3][i] ** 1.5 if c[3][i] > 0 else -np.inf

    def bound(c):
        nu = np.sqrt(c[0] ** 2 + c[1] ** 2 + c[2] ** 2)
        d0 = 0.5 * (c[3].min() + c[3].max())
        g = 1.5 * np.sqrt(d0) * c[3] - 0.5 * d0 ** 1.5
        ok = g > 0
        return (nu[ok] / g[ok]).max() if ok.any() else 0.0

    def split(a):
        left, right, row = [a[0]], [a[-1]], a.copy()
        for _ in range(len(a) - 1):
            row = 0.5 * row[:-1] + 0.5 * row[1:]
            left.append(row[0]); right.append(row[-1])
        return np.array(left), np.array(right[::-1])
    U = max(0.0, kap(co, 0), kap(co, -1))
    todo, nodes = [co], 1
    while todo and nodes < max_nodes:
        c = todo.pop()
        if bound(c) - U <= float(rel) * U:
            continue
        halves = [split(a) for a in c]
        l, r = [h[0] for h in halves], [h[1] for h in halves]
        nodes += 2
        U = max(U, kap(l, -1))
        todo += [l, r]
    return U


def test_the_unguarded_tangent_is_rejected_on_a_wide_speed_curve():
    """space_curvature_ref.wide_speed(), curvature_ref.WIDE_SPEED from t = 1/64 on in space: the speed varies by far more than
    5 x, and the tangent at the mid-range is negative at coefficients whose nu_k is positive.  First: the lifted curve still trips the unguarded rule
    -- it reports less than a value the curve takes.  Then: the yardstick's bracket lies above what the rule reports."""
    space = S.wide_speed()
    wrong = _unguarded(space, REL)
    k2, at = S.sample_max2(space, 1025)
    met = float(mpmath.sqrt(C._mp(k2)))
    assert wrong < met * (1 - 1e-3), ("the lifted curve no longer trips the unguarded rule", wrong, met, float(at))
    r = S.certified_max(space, 0.5, REL)
    assert r['status'] == 'ok' and r['waiting'] <= 32
    assert float(r['L']) >= met * (1 - 1e-12) and float(r['L']) > wrong * (1 + 1e-3)
    # the same rule with the guard (the search of this file) agrees with the sample to its spacing
    assert float(r['H']) >= met


@pytest.mark.parametrize("deg,seed,t", [(3, 0, Fraction(3, 8)), (5, 1, Fraction(5, 16)), (8, 2, Fraction(11, 32))])
def test_the_blocks_rational_form_against_differences(deg, seed, t):
    """d kappa^2 / d P[d][i] = 2 (G / den^3 - |w|^2 H / den^4) in exact rationals against a Richardson-extrapolated
    symmetric difference of the exact kappa^2 (error h^4 times a fifth derivative: h = 2^-12), and the block as
    -(d kappa^2) / (2 kappa)"""
    P = S._ctrl(S.seeded(deg, seed))
    grad = S.kappa2_gradient(P, t)
    blk = S.envelope_block(P, t)
    kap = S.kappa(P, t)
    scale = max(abs(g) for row in grad for g in row)

    def diff(d, i, h):
        up = [list(r) for r in P]
        dn = [list(r) for r in P]
        up[d][i] += h
        dn[d][i] -= h
        return (S.kappa2(up, t) - S.kappa2(dn, t)) / (2 * h)
    h = Fraction(1, 2 ** 12)
    for d in range(3):
        for i in range(deg + 1):
            rich = (4 * diff(d, i, h / 2) - diff(d, i, h)) / 3
            assert abs(rich - grad[d][i]) <= Fraction(1, 10 ** 9) * scale, (d, i, float(rich), float(grad[d][i]))
            assert abs(blk[d][i] + C._mp(grad[d][i]) / (2 * kap)) <= mpmath.mpf(10) ** -40 * (1 + abs(blk[d][i]))


def test_the_planar_block_is_the_space_block_with_wh_along_z():
    planar = C.seeded(5, 2)
    space = [list(r) for r in C._ctrl(planar)] + [[Fraction(0)] * 6]
    t = Fraction(5, 16)
    num = C.num_den(planar, t)[0]
    side = 0 if num > 0 else 1                       # the side on which the planar row is max_curv - |kappa|
    b2, b3 = C.envelope_block(planar, side, t), S.envelope_block(space, t)
    for c in range(2):
        for i in range(6):
            assert abs(b2[c][i] - b3[c][i]) <= mpmath.mpf(10) ** -40 * (1 + abs(b2[c][i]))
    assert all(v == 0 for v in b3[2])


def test_degenerate_rows():
    # degree 1, a straight path of degree 4, a vehicle at rest: w == 0 identically, the bracket is [0, 0] at t = 0, one node
    line = np.stack((np.linspace(0.0, 4.0, 5), np.linspace(1.0, -1.0, 5), np.linspace(0.0, 2.0, 5)))
    for yv in (np.array([[0.0, 2.0], [1.0, 5.0], [3.0, -1.0]]), line, np.full((3, 6), 2.5)):
        r = S.certified_max(yv, 0.5, REL)
        assert r['status'] == 'ok' and r['L'] == 0 and r['H'] == 0 and r['t'] == 0 and r['nodes'] == 1
        w = S.coeffs(yv)[0]
        assert not any(any(row) for row in w)
    # a cusp: den = 0 inside with w != 0 nearby -- the bound stays infinite and the search ends on a cap, with a value met
    r = S.certified_max(S.CUSP, 0.5, REL, max_nodes=400)
    assert r['status'] in ('node_cap', 'depth_cap') and r['H'] is None and r['L'] > 0


def test_majorants_are_finite_on_the_seeded_family():
    yv = S.seeded(5, 0)
    co = S.coeffs(yv)
    K, M = S.kappa_majorant(yv, 0.375, co)
    assert K == S.point_count(5, 3) + 8 and mpmath.isfinite(M) and M > 0
    Kb, Mb = S.block_majorant(yv, 0.375)
    assert Kb == 43 * 5 + 50 and all(mpmath.isfinite(v) for row in Mb for v in row)
    assert mpmath.isfinite(S.bound_majorant(yv, 20, co))
