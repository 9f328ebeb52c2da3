"""CPU side of the true speed rows (obtg_speed_true_min[_jac]): the exact-rational yardstick of speed_envelope_ref.py held to
the oracle's speed coefficients, the inputs the GPU tests share (and what the yardstick says about them), and the ABI
bookkeeping.  No GPU."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speed_envelope_ref as S  # noqa: E402
from util import assert_close  # noqa: E402

FAST = (3, 5, 7, 10, 20)     # degrees with a fused kernel (control-point counts 4, 6, 8, 11, 21 of the fast-kernel list)
SLOW = (6, 13)               # degrees off that list (counts 7, 14): obtg_speed's R = 0 rows, the search, the block launch
DIMS = (2, 3)
TFS = (1.0, 2.5)
BOUND = {0: 3.0, 1: 30.0}    # is_max -> bound of the GPU cases (any value: the minimiser does not depend on it)
# noise seed per (deg, dim): test_shared_inputs_hold_interior_and_end_minima says what a seed has to deliver
SEEDS = {(20, 2): 203}


def seed_of(deg, dim):
    return SEEDS.get((deg, dim), 10 * deg + dim)


def _vehicles(deg, dim, seed):
    """Y[4 * dim][deg + 1]: four vehicles whose first coordinate, on u_i = i / deg, is 18 (3u^2 - 2u^3) - 9 (the speed peaks
    inside), 9 (2u - 1)^3 (the speed dips inside), 20 u^2 (the speed is monotone: both extrema at the ends) and one vehicle
    of synth.swarm_control_points; the other coordinates are small ramps; N(0, 0.05) on every coordinate."""
    from optimalbeziertrajectorygeneration_amd import synth
    rng = np.random.default_rng(seed)
    u = np.arange(deg + 1) / deg
    Y = np.zeros((4 * dim, deg + 1))
    Y[0 * dim] = 18.0 * (3.0 * u ** 2 - 2.0 * u ** 3) - 9.0
    Y[1 * dim] = 9.0 * (2.0 * u - 1.0) ** 3
    Y[2 * dim] = 20.0 * u ** 2
    for v in range(3):
        for c in range(1, dim):
            Y[v * dim + c] = (0.25 * c + 0.1 * v) * u
    Y[3 * dim:4 * dim] = synth.swarm_control_points(1, dim, deg, seed=seed)
    return Y + rng.normal(0.0, 0.05, Y.shape)


def _row(dim, deg, seed):
    """one vehicle's control points on a 2^-12 grid in (-8, 8): y +- 0.5 is exact"""
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(-8.0, 8.0, (dim, deg + 1)) * 4096.0) / 4096.0


@pytest.mark.parametrize("is_max", [0, 1])
@pytest.mark.parametrize("deg,dim", [(5, 2), (10, 3)])
def test_yardstick_against_the_oracle(deg, dim, is_max):
    """The block formula equals sum_k B_k^2n(t) d c_k / d P of the oracle's R = 0 speed coefficients (central differences,
    step 0.5, exact for a quadratic), t at both ends and inside; d/dtf against the closed form q - offset ~ tf^-2 on the
    oracle's coefficients at tf and 2 tf."""
    yv = _row(dim, deg, seed=100 * deg + dim)
    tf, bound = 2.0, 1.5
    worst = 0.0
    for t in (0.0, 1.0, 0.3125):
        ref = S.oracle_block(yv, tf, bound, is_max, t)
        blk, dtf = S.envelope_block(yv, tf, is_max, t)
        got = np.array([[float(v) for v in r] for r in blk])
        worst = max(worst, assert_close(got, ref, what="deg %d dim %d is_max %d t %g" % (deg, dim, is_max, t)))
        if t in (0.0, 1.0):
            keep = [0, 1] if t == 0.0 else [deg - 1, deg]
            assert (np.delete(got, keep, axis=1) == 0.0).all() and (got[:, keep] != 0.0).all()
        q1 = S.oracle_row_minus_offset(yv, tf, bound, is_max, t)
        q2 = S.oracle_row_minus_offset(yv, 2.0 * tf, bound, is_max, t)
        scale = float(max(abs(Fraction(float(c))) for c in S.speed_coeffs(yv, dim, tf, bound, is_max)[0]))
        assert abs(float(q2 - q1 / 4)) <= 1e-9 * scale                       # the tf^-2 law on the oracle's coefficients
        assert abs(float(S.row_minus_offset(yv, tf, is_max, t) - q1)) <= 1e-9 * scale
        assert abs(float(dtf + 2 * q1 / Fraction(tf))) <= 1e-9 * scale       # d/dtf = -2 (q - offset) / tf
        assert (float(q1) < 0) == bool(is_max)
    print("deg %d dim %d is_max %d: largest scaled |yardstick - oracle| = %.3e" % (deg, dim, is_max, worst))


def test_true_row_is_the_certified_minimum_of_the_oracle_row():
    """The bracket is 1e-13 of the largest coefficient wide, its upper end is the formula's q at the returned t, and for
    is_max the row is bound^2 - max s (the bound only shifts it)."""
    dim, tf = 2, 2.5
    Y = _vehicles(5, dim, seed_of(5, dim))
    for is_max in (0, 1):
        off = S.transform(BOUND[is_max], is_max)[1]
        rows = S.true_rows(Y, dim, tf, BOUND[is_max], is_max)
        bare = S.true_rows(Y, dim, tf, 0.0, is_max)
        for v, (r, o) in enumerate(zip(rows, bare)):
            s = float(r["s"])
            assert r["L"] <= r["H"] and r["H"] - r["L"] <= Fraction(1, 10 ** 13) * r["s"]
            assert abs(float(r["H"] - off - o["H"])) <= 1e-12 * s
            assert abs(float(S.row_minus_offset(Y[v * dim:(v + 1) * dim], tf, is_max, r["t"]) + off - r["H"])) <= 1e-9 * s


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("deg", FAST + SLOW)
def test_shared_inputs_hold_interior_and_end_minima(deg, dim):
    """From the yardstick alone: at tf 1.0 and 2.5, for either bound, at least one of the four vehicles has its minimiser
    inside (0, 1) and at least one at an end."""
    Y = _vehicles(deg, dim, seed_of(deg, dim))
    for tf in TFS:
        for is_max in (0, 1):
            t = [r["t"] for r in S.true_rows(Y, dim, tf, BOUND[is_max], is_max)]
            inside = [0 < x < 1 for x in t]
            assert any(inside) and not all(inside), (deg, dim, tf, is_max, [float(x) for x in t])


def yardstick_gap(bo, x, key, is_max, hc=2.0 ** -17, rel=Fraction(1, 10 ** 20)):
    """([N], [N]): per speed row of the BezOptimization `bo` at x (bound bo.model[key]) the largest gap between the yardstick's
    envelope entries -- at its own minimiser, bracket rel * s -- and central differences (step hc) of its certified minima,
    over every variable of x; and s, the row's largest coefficient.  No device: reshapeVector is host code."""
    x = np.asarray(x, dtype=float)
    N, dim = bo.model['numVeh'], bo.model['dim']
    first, cols = bo._rv_parts()[1], bo._numCols
    n_pts = N * dim * cols

    def certified(xx, vehicles):
        Y, tf = bo.reshapeVector(xx), float(bo._tf_of(xx))
        return {v: S.true_rows(Y[v * dim:(v + 1) * dim], dim, tf, bo.model[key], is_max, rel)[0] for v in vehicles}
    y0 = certified(x, range(N))
    blk, dtf = S.envelope_blocks(bo.reshapeVector(x), dim, float(bo._tf_of(x)), is_max, [float(y0[v]["t"]) for v in range(N)])
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


def test_library_exports_the_true_speed_rows():
    """The four names are in the header, the library, obtg_abi_symbols and the binding table; ABI revision 7, K_COUNT 9;
    the speedRows keyword is checked."""
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
    for name in ("obtg_speed_true_min", "obtg_speed_true_min_dev", "obtg_speed_true_min_jac", "obtg_speed_true_min_jac_dev"):
        assert hasattr(lib, name), name
        assert name in syms, name
        assert name in _capi.abi_symbol_names(), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "Later, still 7: new: the true speed rows" in header
    lib.obtg_abi_version.restype = C.c_int
    assert lib.obtg_abi_version() == 7
    assert _capi.K_COUNT == 9
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    with pytest.raises(ValueError, match="speedRows"):
        BezOptimization(speedRows='bogus')
    assert BezOptimization(speedRows='true_min').speedRows == 'true_min' and BezOptimization().speedRows == 'all'
    assert callable(BezOptimization.trueSpeedRange)
