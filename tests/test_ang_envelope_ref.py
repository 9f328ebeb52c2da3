"""CPU side of the true angular-rate rows (obtg_ang_rate_poly, obtg_ang_rate_true_min[_jac]): the exact-rational yardstick of
ang_envelope_ref.py held to the oracle's Bernstein algebra and, through a fixture, to the reference's _angularRate; the
inputs the GPU tests share; the ABI bookkeeping.  No GPU."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ang_envelope_ref as A  # noqa: E402
from util import assert_close  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
LISTED = (3, 5, 10, 20)        # degrees with a fused kernel (control-point counts 4, 6, 11, 21)
UNLISTED = (1, 2, 4, 12, 31)   # degrees off that list: obtg_ang_rate_poly's rows, the search, the block launch
NAMES = ("obtg_ang_rate_poly", "obtg_ang_rate_poly_dev", "obtg_ang_rate_true_min", "obtg_ang_rate_true_min_dev",
         "obtg_ang_rate_true_min_jac", "obtg_ang_rate_true_min_jac_dev")


def random_walk(rng, deg):
    """[2][deg + 1]: a planar random walk from a random start, the same extent at every degree"""
    K = deg + 1
    return rng.uniform(0.0, 3.0, size=(2, 1)) + np.cumsum(rng.normal(0.0, 4.0 / np.sqrt(K), size=(2, K)), axis=1)


def batch(deg, B, n_veh=3, seed=None):
    """(Y[B][n_veh * 2][deg + 1], tf[B]): seeded random walks, tf in [1, 3] -- the inputs of the GPU cases"""
    rng = np.random.default_rng(1000 * deg + B if seed is None else seed)
    Y = np.stack([np.concatenate([random_walk(rng, deg) for _ in range(n_veh)]) for _ in range(B)])
    return np.ascontiguousarray(Y), rng.uniform(1.0, 3.0, B)


def _row(deg, seed):
    """one vehicle's control points on a 2^-12 grid in (-8, 8): y +- 0.5 is exact"""
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(-8.0, 8.0, (2, deg + 1)) * 4096.0) / 4096.0


@pytest.mark.parametrize("deg", [2, 3, 6, 10])
def test_yardstick_against_the_oracle(deg):
    """(1) the exact p_sigma(t) against the oracle's coefficients (diff, diff, mul) contracted with the exact B^2n(t): within
    1e-12 of the row's largest coefficient (measured: 2.7e-15); (2) the block formula against central differences, step 0.5,
    of the oracle's coefficients -- exact because p is at most quadratic in each control point; (3) d/dT against the closed
    form from the oracle's coefficients at T and 2T: den scales by 1/4, num by 1/8, both exactly."""
    yv = _row(deg, seed=100 * deg + 2)
    tf, W = 2.0, 1.5
    worst_p = worst_b = 0.0
    for side in (0, 1):
        scale = float(np.abs(A.ang_coeffs(yv, tf, W)[0, side]).max())
        for t in (0.0, 1.0, 0.3125, 0.8125):
            p = A.row(yv, tf, W, side, t)
            err = abs(float(p - A.oracle_row(yv, tf, W, side, t))) / scale
            worst_p = max(worst_p, err)
            assert err <= 1e-12, (deg, side, t, err)
            blk, dT = A.envelope_block(yv, tf, W, side, t)
            got = np.array([[float(v) for v in r] for r in blk])
            worst_b = max(worst_b, assert_close(got, A.oracle_block(yv, tf, W, side, t), what="deg %d side %d t %g" % (deg, side, t)))
            if t in (0.0, 1.0) and deg >= 3:
                keep = [0, 1, 2] if t == 0.0 else [deg - 2, deg - 1, deg]
                assert (np.delete(got, keep, axis=1) == 0.0).all() and (got[:, keep] != 0.0).any()
            d1, n1 = A.oracle_den_num(yv, tf, t)
            d2, n2 = A.oracle_den_num(yv, 2.0 * tf, t)
            assert abs(float(d2 - d1 / 4)) <= 1e-12 * scale and abs(float(n2 - n1 / 8)) <= 1e-12 * scale
            sg = A.SIGMA[side]
            closed = (-2 * Fraction(W) * d1 + 3 * sg * n1) / Fraction(tf)
            assert abs(float(dT - closed)) <= 1e-9 * scale, (deg, side, t)
    print("deg %d: largest scaled |exact p - oracle| = %.3e, |block - oracle differences| = %.3e" % (deg, worst_p, worst_b))


def test_degree_one_has_no_numerator():
    yv = _row(1, seed=11)
    for side in (0, 1):
        blk, dT = A.envelope_block(yv, 2.0, 1.5, side, 0.25)
        den, num = A.den_num(yv, 2.0, 0.25)
        assert num == 0 and A.row(yv, 2.0, 1.5, side, 0.25) == Fraction(3, 2) * den
        assert_close(np.array([[float(v) for v in r] for r in blk]), A.oracle_block(yv, 2.0, 1.5, side, 0.25), what="degree 1")
        assert dT == -3 * den / 2


def _omega_samples(Y, tf, m=4001):
    """|omega| of every vehicle of the row on m points of [0, 1], float64, from the oracle's den and num coefficients"""
    from math import comb
    den, num = A.den_num_coeffs(Y, tf)
    K = den.shape[1] - 1
    t = np.linspace(0.0, 1.0, m)
    Bm = np.array([comb(K, k) * t ** k * (1.0 - t) ** (K - k) for k in range(K + 1)])
    return np.abs((num @ Bm) / (den @ Bm))


# seeds of the sign property: a random walk that nearly stops has a peak of |omega| too sharp for 4001 points (a sample
# maximum more than 0.1 % below the true one says nothing about W = 1.001 x it), so the seeds are those whose sample maximum a
# grid 16 times finer confirms within 1e-4 -- asserted in the test, from the inputs alone
SIGN_SEEDS = {3: 80, 5: 501, 10: 87, 15: 92}


@pytest.mark.parametrize("deg", [3, 5, 10, 15])
def test_sign_of_the_true_rows_is_the_angular_rate_bound(deg):
    """W at 0.5, 0.999, 1.001 and 2 times the maximum of |omega| sampled on 4001 points: the certified min(r_+, r_-) is
    negative for the first two and not below -1e-9 s for the last two."""
    Y, tf = batch(deg, 1, n_veh=4, seed=SIGN_SEEDS[deg])
    peak = _omega_samples(Y[0], tf[0]).max(axis=1)
    assert (_omega_samples(Y[0], tf[0], m=64001).max(axis=1) <= peak * (1.0 + 1e-4)).all(), "the samples must resolve the peak"
    for v in range(4):
        yv = Y[0, 2 * v:2 * v + 2]
        for f in (0.5, 0.999, 1.001, 2.0):
            r = A.true_rows(yv, tf[0], f * peak[v])[0]
            low = min((r[0]["H"], r[1]["H"]))
            s = max(r[0]["s"], r[1]["s"])
            if f < 1.0:
                assert low < 0, (deg, v, f, float(low))
            else:
                assert low >= -Fraction(1, 10 ** 9) * s, (deg, v, f, float(low), float(s))


def test_true_row_is_the_certified_minimum_and_the_formula_at_its_minimiser():
    Y, tf = batch(5, 1)
    for v, sides in enumerate(A.true_rows(Y[0], tf[0], 1.25)):
        for side, r in enumerate(sides):
            assert r["L"] <= r["H"] and r["H"] - r["L"] <= Fraction(1, 10 ** 13) * r["s"]
            assert abs(float(A.row(Y[0, 2 * v:2 * v + 2], tf[0], 1.25, side, r["t"]) - r["H"])) <= 1e-12 * float(r["s"])


def test_oracle_chain_reproduces_the_reference():
    """tests/golden/angrate_poly.npz (gen_angrate_poly.py: the reference's _angularRate on 8 random walks per degree, tf 2.5):
    the oracle's diff, diff, mul give its `weights` and `cpts * weights` within 1e-13 of the row's largest."""
    g = np.load(os.path.join(HERE, "golden", "angrate_poly.npz"))
    tf = float(g["tf"])
    assert tuple(g["degrees"]) == (3, 5, 10, 15) and tf == 2.5
    for deg in g["degrees"]:
        Y = g["Y%d" % deg]
        assert Y.shape == (8, 2, deg + 1)
        den, num = A.den_num_coeffs(Y.reshape(16, deg + 1), tf)
        for got, key in ((den, "weights%d" % deg), (num, "cw%d" % deg)):
            ref = g[key]
            err = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
            print("degree %d %s: largest scaled difference %.3e" % (deg, key, err.max()))
            assert (err <= 1e-13).all(), (deg, key, err)


def yardstick_gap(bo, x, hc=2.0 ** -17, rel=Fraction(1, 10 ** 20)):
    """([2N], [2N], [2N] bool): per true angular-rate row (2 v + side) of the BezOptimization `bo` at x the largest gap between
    the yardstick's envelope entries -- at its own minimiser, bracket rel * s -- and central differences (step hc) of its
    certified minima, over every variable of x; s, the row's largest coefficient; and whether the row is a TIE: its certified
    minimiser moves by more than 1e-3 between x + hc and x - hc in some variable.  No device: reshapeVector is host code."""
    x = np.asarray(x, dtype=float)
    N = bo.model['numVeh']
    W = bo.model['maxAngRate']
    first, cols = bo._rv_parts()[1], bo._numCols
    n_pts = N * 2 * cols

    def certified(xx, vehicles):
        Y, tf = bo.reshapeVector(xx), float(bo._tf_of(xx))
        return {v: A.true_rows(Y[2 * v:2 * v + 2], tf, W, rel)[0] for v in vehicles}
    y0 = certified(x, range(N))
    t0 = np.array([[float(y0[v][s]["t"]) for s in range(2)] for v in range(N)])
    blk, dtf = A.envelope_blocks(bo.reshapeVector(x), float(bo._tf_of(x)), W, t0)
    J = A.scatter(blk, dtf, N, first, cols, bo._dY_dtf() if bo._timeopt() else None)
    assert J.shape == (2 * N, x.size)
    Cd = np.zeros(J.shape)
    tie = np.zeros(2 * N, bool)
    for k in range(x.size):
        vehicles = [k // (2 * cols)] if k < n_pts else range(N)
        xp, xm = x.copy(), x.copy()
        xp[k] += hc
        xm[k] -= hc
        gp, gm = certified(xp, vehicles), certified(xm, vehicles)
        for v in vehicles:
            for s in range(2):
                Cd[2 * v + s, k] = float(gp[v][s]["H"] - gm[v][s]["H"]) / (xp[k] - xm[k])
                tie[2 * v + s] |= abs(float(gp[v][s]["t"] - gm[v][s]["t"])) > 1e-3
    return np.abs(J - Cd).max(axis=1), np.array([float(y0[v][s]["s"]) for v in range(N) for s in range(2)]), tie


def test_library_exports_the_true_angular_rate_rows():
    """The six names are in the header, the library, obtg_abi_symbols and the binding table; ABI revision 7, K_COUNT 9; the
    angRateRows keyword is checked."""
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
    header = open(os.path.join(HERE, "..", "include", "obtg.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in syms, name
        assert name in _capi.abi_symbol_names(), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "Later, still 7: new: the true angular-rate rows" in header
    lib.obtg_abi_version.restype = C.c_int
    assert lib.obtg_abi_version() == 7
    assert _capi.K_COUNT == 9
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    with pytest.raises(ValueError, match="angRateRows"):
        BezOptimization(angRateRows='bogus')
    assert BezOptimization(angRateRows='true_min').angRateRows == 'true_min' and BezOptimization().angRateRows == 'all'
