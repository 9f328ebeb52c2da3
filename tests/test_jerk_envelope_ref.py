"""CPU side of the true jerk rows (obtg_jerk_true_min[_jac]): the exact-rational yardstick of jerk_envelope_ref.py
held to the oracle's jerk coefficients, the inputs the GPU tests share (and what the yardstick says about them), and
the ABI bookkeeping.  No GPU."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jerk_envelope_ref as S  # noqa: E402
from util import assert_close  # noqa: E402

FAST = (5, 7, 10, 20)        # degrees with a fused kernel (control-point counts 6, 8, 11, 21 of the fast-kernel list)
SLOW = (4, 6, 13)            # degrees off that list (counts 5, 7, 14): obtg_jerk's R = 0 rows, the search, the block launch
DIMS = (2, 3)
TFS = (1.0, 2.5)
BOUND = 30.0                 # of the GPU cases (any value: the minimiser does not depend on it)
# noise seed per (deg, dim): test_shared_inputs_hold_interior_and_end_minima says what a seed has to deliver
SEEDS = {}


def seed_of(deg, dim):
    return SEEDS.get((deg, dim), 10 * deg + dim)


def _vehicles(deg, dim, seed):
    """Y[4 * dim][deg + 1]: four vehicles whose first coordinate, on u_i = i / deg, is 9 cos(pi u) (the third differences
    peak in the middle: the jerk peaks inside), 10 u^4 (the jerk grows: its maximum is at t = 1),
    10 (1 - u)^4 (at t = 0) and one vehicle of synth.swarm_control_points; the other coordinates are small ramps (no
    jerk); N(0, 0.005) on every coordinate."""
    from optimalbeziertrajectorygeneration_amd import synth
    rng = np.random.default_rng(seed)
    u = np.arange(deg + 1) / deg
    Y = np.zeros((4 * dim, deg + 1))
    Y[0 * dim] = 9.0 * np.cos(np.pi * u)
    Y[1 * dim] = 10.0 * u ** 4
    Y[2 * dim] = 10.0 * (1.0 - u) ** 4
    for v in range(3):
        for c in range(1, dim):
            Y[v * dim + c] = (0.25 * c + 0.1 * v) * u
    Y[3 * dim:4 * dim] = synth.swarm_control_points(1, dim, deg, seed=seed)
    return Y + rng.normal(0.0, 0.005, Y.shape)


def _row(dim, deg, seed):
    """one vehicle's control points on a 2^-12 grid in (-8, 8): y +- 0.5 is exact"""
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(-8.0, 8.0, (dim, deg + 1)) * 4096.0) / 4096.0


@pytest.mark.parametrize("deg,dim", [(3, 2), (4, 3), (5, 2), (7, 3)])
def test_yardstick_against_the_oracle(deg, dim):
    """The block formula equals sum_k B_k^2n(t) d c_k / d P of the oracle's R = 0 jerk coefficients (central
    differences, step 0.5, exact for a quadratic), t at both ends and inside; d/dtf against the closed form
    q - bound^2 ~ tf^-6 on the oracle's coefficients at tf and 2 tf."""
    yv = _row(dim, deg, seed=100 * deg + dim)
    tf, bound = 2.0, 1.5
    worst = 0.0
    for t in (0.0, 1.0, 0.3125):
        ref = S.oracle_block(yv, tf, bound, t)
        blk, dtf = S.envelope_block(yv, tf, t)
        got = np.array([[float(v) for v in r] for r in blk])
        worst = max(worst, assert_close(got, ref, what="deg %d dim %d t %g" % (deg, dim, t)))
        if t in (0.0, 1.0):
            keep = [0, 1, 2, 3] if t == 0.0 else [deg - 3, deg - 2, deg - 1, deg]
            assert (np.delete(got, keep, axis=1) == 0.0).all() and (got[:, keep] != 0.0).all()
        q1 = S.oracle_row_minus_offset(yv, tf, bound, t)
        q2 = S.oracle_row_minus_offset(yv, 2.0 * tf, bound, t)
        scale = float(max(abs(Fraction(float(c))) for c in S.jerk_coeffs(yv, dim, tf, bound)[0]))
        assert abs(float(q2 - q1 / 64)) <= 1e-9 * scale                      # the tf^-6 law on the oracle's coefficients
        assert abs(float(S.row_minus_offset(yv, tf, t) - q1)) <= 1e-9 * scale
        assert abs(float(dtf + 6 * q1 / Fraction(tf))) <= 1e-9 * scale       # d/dtf = -6 (q - bound^2) / tf
        assert float(q1) < 0
    print("deg %d dim %d: largest scaled |yardstick - oracle| = %.3e" % (deg, dim, worst))


def test_degrees_one_and_two_have_no_jerk():
    """exactly none in rational arithmetic; the oracle's degree-1 rows are bound^2 bit for bit, its degree-2 rows bound^2 up to
    the residue of three rounded passes"""
    for deg in (1, 2):
        yv = _row(2, deg, seed=7)
        blk, dtf = S.envelope_block(yv, 2.0, 0.25)
        assert all(x == 0 for r in blk for x in r) and dtf == 0 and S.row_minus_offset(yv, 2.0, 0.25) == 0
        co = S.jerk_coeffs(yv, 2, 2.0, 1.5)
        if deg == 1:
            assert (co == 1.5 ** 2).all()
        else:
            assert_close(co, np.full(co.shape, 1.5 ** 2), what="degree 2")


def test_degree_three_block_is_the_same_at_every_t():
    yv = _row(3, 3, seed=11)
    b0, d0 = S.envelope_block(yv, 2.0, 0.0)
    for t in (0.25, 1.0):
        assert S.envelope_block(yv, 2.0, t) == (b0, d0)
    assert any(x != 0 for r in b0 for x in r)


def test_true_row_is_the_certified_minimum_of_the_oracle_row():
    """The bracket is 1e-13 of the largest coefficient wide, its upper end is the formula's q at the returned t, and the row
    is bound^2 - max (d/2)|a|^2 (the bound only shifts it)."""
    dim, tf = 2, 2.5
    Y = _vehicles(5, dim, seed_of(5, dim))
    off = S.offset(BOUND)
    rows = S.true_rows(Y, dim, tf, BOUND)
    bare = S.true_rows(Y, dim, tf, 0.0)
    for v, (r, o) in enumerate(zip(rows, bare)):
        s = float(r["s"])
        assert r["L"] <= r["H"] and r["H"] - r["L"] <= Fraction(1, 10 ** 13) * r["s"]
        assert abs(float(r["H"] - off - o["H"])) <= 1e-12 * s
        assert abs(float(S.row_minus_offset(Y[v * dim:(v + 1) * dim], tf, r["t"]) + off - r["H"])) <= 1e-9 * s


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("deg", FAST + SLOW)
def test_shared_inputs_hold_interior_and_end_minima(deg, dim):
    """From the yardstick alone: at tf 1.0 and 2.5 at least one of the four vehicles has its minimiser inside (0, 1) and at
    least one at an end.  Degree 4 is the exception a quartic forces: its jerk is linear in t, |c'''|^2 a convex
    quadratic and the row concave, so EVERY minimiser is at an end -- asserted as that."""
    Y = _vehicles(deg, dim, seed_of(deg, dim))
    for tf in TFS:
        t = [r["t"] for r in S.true_rows(Y, dim, tf, BOUND)]
        inside = [0 < x < 1 for x in t]
        if deg == 4:
            assert not any(inside), (deg, dim, tf, [float(x) for x in t])
        else:
            assert any(inside) and not all(inside), (deg, dim, tf, [float(x) for x in t])


def yardstick_gap(bo, x, hc=2.0 ** -17, rel=Fraction(1, 10 ** 20)):
    """([N], [N]): per jerk row of the BezOptimization `bo` at x (bound bo.model['maxJerk']) the largest gap between
    the yardstick's envelope entries -- at its own minimiser, bracket rel * s -- and central differences (step hc) of its
    certified minima, over every variable of x; and s, the row's largest coefficient.  No device: reshapeVector is host code."""
    x = np.asarray(x, dtype=float)
    N, dim = bo.model['numVeh'], bo.model['dim']
    first, cols = bo._rv_parts()[1], bo._numCols
    n_pts = N * dim * cols

    def certified(xx, vehicles):
        Y, tf = bo.reshapeVector(xx), float(bo._tf_of(xx))
        return {v: S.true_rows(Y[v * dim:(v + 1) * dim], dim, tf, bo.model['maxJerk'], rel)[0] for v in vehicles}
    y0 = certified(x, range(N))
    blk, dtf = S.envelope_blocks(bo.reshapeVector(x), dim, float(bo._tf_of(x)), [float(y0[v]["t"]) for v in range(N)])
    J = S.scatter(blk, dtf, N, dim, first, cols, bo._dY_dtf() if bo._timeopt() else None)
    assert J.shape == (N, x.size)
    Cd = np.zeros(J.shape)
    for k in range(x.size):
        vehicles = [k // (dim * cols)] if k < n_pts else range(N)      # a control point moves its own vehicle's row alone
        xp, xm = x.copy(), x.copy()
        xp[k] += hc
        xm[k] -= hc
        gp, gm = certified(xp, vehicles), certified(xm, vehicles)
        for v in vehicles:
            Cd[v, k] = float(gp[v]["H"] - gm[v]["H"]) / (xp[k] - xm[k])
    return np.abs(J - Cd).max(axis=1), np.array([float(y0[v]["s"]) for v in range(N)])


NEW_SYMBOLS = ("obtg_jerk", "obtg_jerk_dev", "obtg_jerk_true_min", "obtg_jerk_true_min_dev", "obtg_jerk_true_min_jac",
               "obtg_jerk_true_min_jac_dev")


def test_library_exports_the_jerk_rows():
    """The six names are in the header, the library, obtg_abi_symbols and the binding table; ABI revision 7, K_COUNT 9;
    the jerkRows keyword is checked."""
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
    assert "Later, still 7: new: the jerk-bound rows" in header
    lib.obtg_abi_version.restype = C.c_int
    assert lib.obtg_abi_version() == 7
    assert _capi.K_COUNT == 9
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    with pytest.raises(ValueError, match="jerkRows"):
        BezOptimization(jerkRows='bogus')
    bo = BezOptimization(jerkRows='true_min', maxJerk=2.0)
    assert bo.jerkRows == 'true_min' and bo.model['maxJerk'] == 2.0
    assert BezOptimization().jerkRows == 'all' and BezOptimization().model['maxJerk'] is None
    assert callable(BezOptimization.trueJerkMax) and callable(BezOptimization.maxJerkJacobian)
    # both enter the key of a kept finite-difference batch
    a = BezOptimization(numVeh=1, dimension=2, degree=4, initPoints=[(0, 0)], finalPoints=[(1, 1)], maxJerk=2.0)
    k0 = a._serve_key(True)
    a.model['maxJerk'] = 3.0
    k1 = a._serve_key(True)
    a.jerkRows = 'true_min'
    assert k0 != k1 and k1 != a._serve_key(True)
