"""tests/extrema_ref.py -- the exact yardstick of the true-extrema tests -- against closed forms and against the oracle's
de Casteljau evaluation on a fine grid; and the new entries' presence in header, library and binding table."""
import os
import re
import sys
from fractions import Fraction
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extrema_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

C6_Y = [5.0, 0.0, 2.0, 5.0, 7.0, 5.0]          # the reference's example: c6 = Bezier([(0,1,2,3,4,5), (5,0,2,5,7,5)])
C6_MIN, C6_MAX = 2.2606668630782703, 5.699106677492463


def _bern_of_power(a):
    """Bernstein coefficients (exact Fractions) of sum a_i t^i at degree len(a) - 1"""
    n = len(a) - 1
    return [sum(Fraction(comb(k, i), comb(n, i)) * a[i] for i in range(k + 1)) for k in range(n + 1)]


def _elev(c, R_):
    c = list(c)
    for _ in range(R_):
        n = len(c)
        c = [c[0]] + [Fraction(i, n) * c[i - 1] + Fraction(n - i, n) * c[i] for i in range(1, n)] + [c[-1]]
    return c


def test_constants_and_lines():
    for K in (1, 2, 5, 21):
        r = R.certified_min([3.25] * K)
        assert r["L"] == r["H"] == Fraction(3.25) and r["nodes"] == 1
    r = R.certified_min([2.0, -1.0])
    assert r["H"] == -1 and r["t"] == 1 and r["L"] == -1
    r = R.certified_max([2.0, -1.0])
    assert r["L"] == r["H"] == 2 and r["t"] == 0


@pytest.mark.parametrize("elev", [0, 1, 3, 8, 18])
@pytest.mark.parametrize("a", [Fraction(1, 4), Fraction(3, 8), Fraction(5, 16), Fraction(1, 2)])
def test_shifted_square(a, elev):
    """(t - a)^2 + 1/8 with dyadic a, elevated.  Where an elevated coefficient is not exact in float64 the polynomial of the
    ROUNDED coefficients is what is bracketed: a Bernstein polynomial moves by at most the largest coefficient change,
    2^-53 s."""
    c = _elev(_bern_of_power([a * a + Fraction(1, 8), -2 * a, Fraction(1)]), elev)
    cf = [float(x) for x in c]
    r = R.certified_min(cf)
    slack = max(abs(Fraction(x) - y) for x, y in zip(cf, c))
    assert slack <= Fraction(1, 2 ** 53) * r["s"]
    assert r["L"] - slack <= Fraction(1, 8) <= r["H"] + slack
    assert r["H"] - r["L"] <= R.REL * r["s"]
    assert abs(r["t"] - a) <= Fraction(1, 1000)


def test_double_minimum():
    """((t - 1/4)(t - 3/4))^2 - 1/2: two equal minima of -1/2 (degree 4), elevated twice"""
    a, b = Fraction(1, 4), Fraction(3, 4)
    q = [a * b, -(a + b), Fraction(1)]
    sq = [sum(q[i] * q[k - i] for i in range(3) if 0 <= k - i < 3) for k in range(5)]
    sq[0] -= Fraction(1, 2)
    for elev in (0, 2):
        c = _elev(_bern_of_power(sq), elev)
        cf = [float(x) for x in c]
        slack = max(abs(Fraction(x) - y) for x, y in zip(cf, c))       # the rounded coefficients' polynomial is what is bracketed
        r = R.certified_min(cf)
        assert slack <= Fraction(1, 2 ** 53) * r["s"]
        assert r["L"] - slack <= Fraction(-1, 2) <= r["H"] + slack and r["H"] - r["L"] <= R.REL * r["s"]
        rmax = R.certified_max([-x for x in cf])
        assert rmax["L"] - slack <= Fraction(1, 2) <= rmax["H"] + slack


@pytest.mark.parametrize("K", [3, 4, 6, 11, 21, 31, 41])
def test_against_sampling(K):
    """20 001 samples of the oracle's de Casteljau evaluation: L <= sampled min, and the sampled minimum is above H by no
    more than the sampling bound -- |p''| <= n (n - 1) max |second difference| <= 4 n (n - 1) s, so within h = 1 / 40 000 of
    the minimiser p rises by at most 2 n (n - 1) s h^2 (first derivative zero inside, or an end point sampled exactly) --
    plus the evaluation's rounding, 2 n x 1.1e-16 x s."""
    rng = np.random.default_rng(100 + K)
    tau = np.linspace(0.0, 1.0, 20001)
    n = K - 1
    for trial in range(6):
        c = rng.uniform(-10.0, 10.0, K) * 10.0 ** rng.integers(-3, 4)
        r = R.certified_min(c)
        assert r["H"] - r["L"] <= R.REL * r["s"] and r["nodes"] <= 400
        s = float(r["s"])
        sm = float(O.curve_eval(c, tau, 0.0, 1.0).min())
        rnd = 2 * K * 1.2e-16 * s
        assert float(r["L"]) <= sm + rnd
        assert sm - float(r["H"]) <= 2.0 * n * (n - 1) * s * (1.0 / 40000.0) ** 2 + rnd
        rx = R.certified_max(c)
        sx = float(O.curve_eval(c, tau, 0.0, 1.0).max())
        assert float(rx["H"]) >= sx - rnd and float(rx["L"]) - sx <= 2.0 * n * (n - 1) * s * (1.0 / 40000.0) ** 2 + rnd


def test_reference_example_c6():
    """C6_MIN / C6_MAX are the extrema over 200 001 samples: above the minimum (below the maximum) by at most the sampling
    bound 2 n (n - 1) s h^2 = 2 * 5 * 4 * 7 * (1 / 400 000)^2 = 1.75e-9."""
    r = R.certified_min(C6_Y)
    assert float(r["L"]) <= C6_MIN and C6_MIN - float(r["H"]) <= 1.75e-9
    r = R.certified_max(C6_Y)
    assert float(r["H"]) >= C6_MAX and float(r["L"]) - C6_MAX <= 1.75e-9


def test_separation_coeffs_are_the_oracle_rows():
    rng = np.random.default_rng(5)
    y = rng.uniform(-5, 5, (3 * 2, 6))
    c = R.separation_coeffs(y, 3, 2, 0.9)
    assert c.shape == (3, 11)
    assert np.array_equal(c.ravel(), O.temporal_sep(y, 3, 2, 0, 0.9))


def test_library_exports_the_extrema():
    """The four names are in the header, the library, obtg_abi_symbols and the binding table; new symbols alone do not move
    the ABI revision, and the launches are timed under existing ids."""
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
    for name in ("obtg_bern_extrema", "obtg_bern_extrema_dev", "obtg_temporal_sep_true_min", "obtg_temporal_sep_true_min_dev"):
        assert hasattr(lib, name), name
        assert name in syms, name
        assert name in _capi.abi_symbol_names(), name
        assert re.search(r"\bint %s\(" % name, header), name
    lib.obtg_abi_version.restype = C.c_int
    assert lib.obtg_abi_version() == 7
    assert _capi.K_COUNT == 9
    from optimalbeziertrajectorygeneration_amd import bezier
    assert callable(bezier.Bezier.min) and callable(bezier.Bezier.max)
