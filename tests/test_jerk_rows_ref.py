"""Holds tests/jerk_rows_ref.py honest, on the CPU: (a) the CPU oracle's jerk rows -- its maximum-speed rows of the second
derivative's control points, composed from existing functions -- pass the exact-rational bound at every shape
tests/test_gpu_jerk_rows.py uses, (b) the same composition agrees with what the REFERENCE's
diff().diff().diff().normSquare().elev(R) returned (tests/golden/jerk_rows.npz) within RTOL, and those outputs pass the bound
too, (c) degree 1 is bound**2 exactly, degree 2 is bound**2 in exact arithmetic with a majorant that does not vanish, degree 3
is constant, and the yardstick says so.  No GPU.  The largest shares of the bound are printed (pytest -s)."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jerk_rows_ref as JR  # noqa: E402
import constraint_rows_ref as C  # noqa: E402
from util import RTOL, assert_close  # noqa: E402


def test_oracle_jerk_at_every_device_shape(oracle):
    worst = {}
    for name, N, d, n, R, kind, form in JR.JERK_CASES:
        Y = C.swarm(12, N, d, n, kind)
        for tf in JR.JERK_TF:
            ref = JR.jerk(Y, N, d, R, tf, JR.JERK_BOUND)
            got = JR.oracle_rows(oracle, Y, N, d, R, tf, JR.JERK_BOUND)
            key = "generic shapes" if "generic" in form else ("R > 0" if R else "R = 0")
            worst[key] = max(worst.get(key, 0.0), JR.assert_within(got, ref, "%s tf %r" % (name, tf)))
    print("\nCPU oracle, jerk: largest share of the bound used")
    for k in sorted(worst):
        print("  %-16s %.3f" % (k, worst[k]))
    assert all(v <= 1.0 for v in worst.values())


def test_counts_are_the_acceleration_grant_plus_the_third_diff():
    for d, n, R in ((2, 5, 0), (3, 10, 7)):
        sp, ac, jk = C._counts_rows(d, n, R, 16), C._counts_rows(d, n, R, 32), C._counts_rows(d, n, R, 48)
        assert [a - s for a, s in zip(jk, ac)] == [16] * (2 * n + R + 1)
        assert [a - s for a, s in zip(jk, sp)] == [32] * (2 * n + R + 1)
        ref = JR.jerk(C.swarm(3, 2, d, n), 2, d, R, 1.0, 1.0)
        assert ref.K == jk * 2 and ref.shape == (2, 2 * n + R + 1)


def test_degree_one_and_two_rows_are_the_squared_bound():
    """exactly bound**2 in rational arithmetic; at degree 2 the majorant still stands above it (the rows are held to
    K 2^-53 M there, not to bit equality)"""
    b2 = Fraction(3.7 ** 2)
    for deg in (1, 2):
        Y = C.swarm(5, 3, 2, deg)
        ref = JR.jerk(Y, 3, 2, 0, 0.013, 3.7)
        cnt = 3 * (2 * deg + 1)
        assert all(ref.value(i) == b2 for i in range(cnt)) and all(ref.majorant(i) >= b2 for i in range(cnt))
        if deg == 2:
            assert all(ref.majorant(i) > b2 for i in range(cnt))


def test_degree_three_rows_are_constant():
    """a cubic has the constant jerk 6 (P3 - 3 P2 + 3 P1 - P0) / T^3: every coefficient of the row is the same value"""
    Y = C.swarm(6, 2, 3, 3)
    tf = 2.5
    ref = JR.jerk(Y, 2, 3, 0, tf, 0.0)
    for v in range(2):
        P = [[Fraction(float(x)) for x in Y[v * 3 + c]] for c in range(3)]
        j = [6 * (p[3] - 3 * p[2] + 3 * p[1] - p[0]) / Fraction(tf) ** 3 for p in P]
        want = -Fraction(3, 2) * sum(x * x for x in j)
        assert all(ref.value(v * 7 + k) == want for k in range(7))


def test_closed_form_at_degree_five():
    """the yardstick's R = 0 row, contracted with the exact B_k^2n(t), is bound^2 - (d/2)|c'''(t)|^2 of the closed form"""
    import envelope_ref as E
    n, d, tf = 5, 2, 2.5
    Y = C.swarm(9, 1, d, n)
    ref = JR.jerk(Y, 1, d, 0, tf, 1.5)
    T = Fraction(tf)
    for t in (Fraction(0), Fraction(1), Fraction(5, 16)):
        w2, u = E.basis(2 * n, t), E.basis(n - 3, t)
        q = sum(w2[k] * ref.value(k) for k in range(2 * n + 1))
        P = [[Fraction(float(x)) for x in row] for row in Y]
        j = [Fraction(n * (n - 1) * (n - 2)) / T ** 3 * sum(u[i] * (p[i + 3] - 3 * p[i + 2] + 3 * p[i + 1] - p[i]) for i in range(n - 2))
             for p in P]
        assert q == Fraction(1.5 ** 2) - Fraction(d, 2) * sum(x * x for x in j)


def test_reference_fixture(oracle, golden_dir):
    """The oracle's composition against the reference's own outputs, scale-aware within RTOL, and the reference's outputs inside
    the exact bound (bound 0: the rows are -c)."""
    worst = share = 0.0
    count = 0
    for name, Y, dim, deg, R, tf, c in JR.fixture_rows(golden_dir):
        N = Y.shape[0] // dim
        assert c.shape == (N, 2 * deg + R + 1)
        got = JR.oracle_rows(oracle, Y, N, dim, R, tf, 0.0)
        worst = max(worst, assert_close(-got, c, what=name))
        share = max(share, JR.assert_within(0.0 - c, JR.jerk(Y, N, dim, R, tf, 0.0), name))
        count += 1
    assert count == 5 * 2 * 2 * 2
    print("reference fixture: largest scaled |oracle - reference| = %.3e (RTOL %.0e); largest share of the exact bound %.3f"
          % (worst, RTOL, share))
