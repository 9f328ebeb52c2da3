"""The yardstick of the jerk-bound rows (obtg_jerk): every output element in EXACT arithmetic, with the forward-error
bound a float64 evaluation of the same formula has to meet.  Built on tests/bezier_algebra_ref.py and
tests/constraint_rows_ref.py (Ref, assert_within, the integer helpers, the case tables); no device, no oracle, no reference code.

    jerk   diff() [derivative, then elev(1)] three times, normSquare(), elev(R), then bound**2 - c

bound**2 enters as the float64 Python's `**` gives (constraint_rows_ref.square).

With the integers v of one coordinate row (x = v 2^e) and T = Tp / 2^Ts, `_diff_nums` applied three times is T^3 x''' exactly,
its majorant the same formula on magnitudes (the derivative's majorant is the SUM of magnitudes at every level: each product is
rounded at the magnitude of its operand, constraint_rows_ref's module docstring).  `_normsq_nums` of the d rows is
2 C(2n, k) T^6 times the (d/2)-scaled coefficient, `_elev_ints` makes that 2 C(2n + R, k) T^6 times the elevated one, so the
element is num / (2 C(2n + R, k) Tp^6) * 2^(2 (e + 3 Ts)), and `_affine` puts it under sign = -1 and offset = bound**2.

The count K per element is constraint_rows_ref._counts_rows(dim, n, R, 48).  Against the device code (bern_device.h
diff_elev1_at, three times): `val * (p[c] - p[c-1])`, `val * (p[c+1] - p[c])`, the ratio, the product and the fma are 6
roundings per level with `val = N / tf` shared -- accel_rows_ref's count of one level --, and what a level inherits from the one
below is carried by the majorant, which is formed level by level on magnitudes.  Each level is granted 8 per factor, as
bezier_algebra_ref.diff grants one diff(): 8 for the speed rows' source curve, 16 for the acceleration's ("x'', y'' carry 16"
in constraint_rows_ref's derivation of the angular rate), 24 here: counted 18, granted 24 per factor, 48 for the two factors
where the acceleration rows have 32, the speed rows 16 and the separation rows 2.  Everything after the source curve is the
speed rows' body and keeps their grant.  A derivation, not a measurement.

Degrees 1 and 2: the exact value of every element is bound**2 (num = 0).  At degree 1 the second pass is exactly zero on the
device as well (differences of equal numbers), so the rows are bound**2 bit for bit; at degree 2 three float64 passes need not
cancel, and the rows are held to K 2^-53 M like any other -- M, formed on magnitudes, does not vanish.
"""
import numpy as np

import bezier_algebra_ref as A
import constraint_rows_ref as C
from bezier_algebra_ref import Ref, assert_within, shares, within  # noqa: F401  (the tests take them from here)


def jerk(Y, n_veh, dim, R, tf, bound):
    """Rows of obtg_jerk for one evaluation row Y[n_veh * dim][n + 1] and its tf.  -> Ref of shape (n_veh, 2 n + R + 1)"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    nc = Y.shape[1]
    n = nc - 1
    assert n >= 1 and Y.shape[0] == n_veh * dim and tf != 0
    v, e = A._ints(Y)
    Tp, Ts = A._dyadic(tf)
    den_row = [2 * c * Tp ** 6 for c in A._binrow(2 * n + R)]
    K_row = C._counts_rows(dim, n, R, 48)
    off = C.square(bound)
    num, mnum, den, K = [], [], [], []
    for veh in range(n_veh):
        rows = [v[(veh * dim + q) * nc:(veh * dim + q + 1) * nc] for q in range(dim)]
        d1 = [A._diff_nums(r, A._absl(r), n) for r in rows]                     # T x', and its majorant
        d2 = [A._diff_nums(a, m, n) for a, m in d1]                             # T^2 x''
        d3 = [A._diff_nums(a, m, n) for a, m in d2]                             # T^3 x'''
        a, m = C._elev_ints(A._normsq_nums([x[0] for x in d3], nc), A._normsq_nums([x[1] for x in d3], nc), 2 * n, R)
        num += a
        mnum += m
        den += den_row
        K += K_row
    num, mnum, E = C._affine(num, mnum, den, 2 * (e + 3 * Ts), -1, off)
    return Ref(num, den, mnum, E, K, (n_veh, 2 * n + R + 1))


def oracle_rows(O, Y, n_veh, dim, R, tf, bound):
    """The ORACLE's jerk rows: its maximum-speed rows of the second derivative's control points, [n_veh][2 n + R + 1]"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    return O.speed(O.diff(O.diff(Y, float(tf)), float(tf)), n_veh, dim, R, float(tf), float(bound), True).reshape(n_veh, -1)


# (name, n_veh, dim, deg, R, kind, form): jerk through obtg_jerk -- the shapes of constraint_rows_ref.SPEED_CASES the
# issue names, with degree 1 (every row is bound**2), degree 2 (no jerk: rounding residue) and degree 3 (a constant jerk; the
# count 4 of NC_SEP)
JERK_TF = C.SPEED_TF
JERK_BOUND = 4.0
JERK_CASES = (
    [("N = %d" % N, N, 2, 5, 0, "full", "k_normsq_elev<MODE 3>") for N in (1, 64, 65)] +
    [("nc %d, %d-D" % (nc, d), 3, d, nc - 1, 0, "offset" if d == 3 else "full", "k_normsq_elev<MODE 3>") for nc in C.NC_SEP for d in (2, 3)] +
    [("R = 1", 5, 2, 10, 1, "full", "k_normsq_elev<MODE 3, ELEV>"),
     ("R = 100, 3-D", 3, 3, 7, 100, "offset", "k_normsq_elev<MODE 3, ELEV>"),
     ("R = 513", 2, 2, 3, 513, "full", "k_generic_normsq_elev<3>"),
     ("generic dim 1", 3, 1, 6, 0, "full", "k_generic_normsq_elev<3>"),
     ("generic deg 12, R = 5", 3, 2, 12, 5, "offset", "k_generic_normsq_elev<3>"),
     ("generic deg 31, 3-D", 2, 3, 31, 0, "full", "k_generic_normsq_elev<3>"),
     ("deg 1", 3, 2, 1, 0, "full", "k_generic_normsq_elev<3>"),
     ("deg 2", 3, 3, 2, 0, "full", "k_generic_normsq_elev<3>")])


def fixture_rows(golden_dir):
    """tests/golden/jerk_rows.npz as (name, Y[4 * dim][deg + 1], dim, deg, R, tf, c[4][2 deg + R + 1]): what the reference's
    Bezier(y, tf=tf).diff().diff().diff().normSquare().elev(R).cpts returned (tests/golden/gen_jerk_rows.py)"""
    import os
    g = np.load(os.path.join(golden_dir, "jerk_rows.npz"))
    for deg in g["degrees"].tolist():
        for dim in g["dims"].tolist():
            Y = g["Y%d_%d" % (deg, dim)]
            for R in g["elevs"].tolist():
                for it, tf in enumerate(g["tfs"].tolist()):
                    yield ("deg %d dim %d R %d tf %g" % (deg, dim, R, tf), Y, dim, deg, R, tf, g["c%d_%d_%d_%d" % (deg, dim, R, it)])
