"""Holds tests/accel_rows_ref.py honest, on the CPU: (a) the CPU oracle's acceleration rows -- its maximum-speed rows of the
first derivative's control points -- pass the exact-rational bound at every shape tests/test_gpu_accel_rows.py uses, (b) the
same composition agrees with what the REFERENCE's diff().diff().normSquare().elev(R) returned (tests/golden/accel_rows.npz)
within RTOL, and those outputs pass the bound too, (c) degree 1 is bound**2 exactly and the yardstick says so.  No GPU.
The largest shares of the bound are printed (pytest -s)."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accel_rows_ref as AR  # noqa: E402
import constraint_rows_ref as C  # noqa: E402
from util import RTOL, assert_close  # noqa: E402


def test_oracle_acceleration_at_every_device_shape(oracle):
    worst = {}
    for name, N, d, n, R, kind, form in AR.ACCEL_CASES:
        Y = C.swarm(12, N, d, n, kind)
        for tf in AR.ACCEL_TF:
            ref = AR.accel(Y, N, d, R, tf, AR.ACCEL_BOUND)
            got = AR.oracle_rows(oracle, Y, N, d, R, tf, AR.ACCEL_BOUND)
            key = "generic shapes" if "generic" in form else ("R > 0" if R else "R = 0")
            worst[key] = max(worst.get(key, 0.0), AR.assert_within(got, ref, "%s tf %r" % (name, tf)))
    print("\nCPU oracle, acceleration: largest share of the bound used")
    for k in sorted(worst):
        print("  %-16s %.3f" % (k, worst[k]))
    assert all(v <= 1.0 for v in worst.values())


def test_counts_are_the_speed_grant_plus_the_second_diff():
    for d, n, R in ((2, 5, 0), (3, 10, 7)):
        sp, ac = C._counts_rows(d, n, R, 16), C._counts_rows(d, n, R, 32)
        assert [a - s for a, s in zip(ac, sp)] == [16] * (2 * n + R + 1)
        ref = AR.accel(C.swarm(3, 2, d, n), 2, d, R, 1.0, 1.0)
        assert ref.K == ac * 2 and ref.shape == (2, 2 * n + R + 1)


def test_degree_one_rows_are_the_squared_bound():
    Y = C.swarm(5, 3, 2, 1)
    ref = AR.accel(Y, 3, 2, 0, 0.013, 3.7)
    b2 = Fraction(3.7 ** 2)
    assert all(ref.value(i) == b2 for i in range(9)) and all(ref.majorant(i) >= b2 for i in range(9))


def test_degree_two_rows_are_constant():
    """a degree-2 curve has a constant acceleration 2 (P0 - 2 P1 + P2) / T^2: every coefficient of the row is the same value"""
    Y = C.swarm(6, 2, 3, 2)
    tf = 2.5
    ref = AR.accel(Y, 2, 3, 0, tf, 0.0)
    for v in range(2):
        a = [2 * (Fraction(float(Y[v * 3 + c, 0])) - 2 * Fraction(float(Y[v * 3 + c, 1])) + Fraction(float(Y[v * 3 + c, 2]))) / Fraction(tf) ** 2
             for c in range(3)]
        want = -Fraction(3, 2) * sum(x * x for x in a)
        assert all(ref.value(v * 5 + k) == want for k in range(5))


def test_reference_fixture(oracle, golden_dir):
    """The oracle's composition against the reference's own outputs, scale-aware within RTOL (measured: 3.7e-16 worst over
    these shapes), and the reference's outputs inside the exact bound (bound 0: the rows are -c)."""
    worst = share = 0.0
    count = 0
    for name, Y, dim, deg, R, tf, c in AR.fixture_rows(golden_dir):
        N = Y.shape[0] // dim
        assert c.shape == (N, 2 * deg + R + 1)
        got = AR.oracle_rows(oracle, Y, N, dim, R, tf, 0.0)
        worst = max(worst, assert_close(-got, c, what=name))
        share = max(share, AR.assert_within(0.0 - c, AR.accel(Y, N, dim, R, tf, 0.0), name))
        count += 1
    assert count == 4 * 2 * 2 * 2
    print("reference fixture: largest scaled |oracle - reference| = %.3e (RTOL %.0e); largest share of the exact bound %.3f"
          % (worst, RTOL, share))
