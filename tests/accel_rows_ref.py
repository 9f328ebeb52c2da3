"""The yardstick of the acceleration-bound rows (obtg_accel): every output element in EXACT arithmetic, with the forward-error
bound a float64 evaluation of the same formula has to meet.  Built on tests/bezier_algebra_ref.py and
tests/constraint_rows_ref.py (Ref, assert_within, the integer helpers, the case tables); no device, no oracle, no reference code.

    acceleration   diff() [derivative, then elev(1)], diff() again, normSquare(), elev(R), then bound**2 - c

bound**2 enters as the float64 Python's `**` gives (constraint_rows_ref.square).

With the integers v of one coordinate row (x = v 2^e) and T = Tp / 2^Ts, `_diff_nums` applied twice is T^2 x'' exactly, its
majorant the same formula on magnitudes (the derivative's majorant is the SUM of magnitudes at every level: each product is
rounded at the magnitude of its operand, constraint_rows_ref's module docstring).  `_normsq_nums` of the d rows is
2 C(2n, k) T^4 times the (d/2)-scaled coefficient, `_elev_ints` makes that 2 C(2n + R, k) T^4 times the elevated one, so the
element is num / (2 C(2n + R, k) Tp^4) * 2^(2 (e + 2 Ts)), and `_affine` puts it under sign = -1 and offset = bound**2.

The count K per element is constraint_rows_ref._counts_rows(dim, n, R, 32): the speed rows' grant with the second diff's 8 per
factor on top of the first's -- "x'', y'' carry 16" in that module's derivation of the angular rate --, so 32 for the two
factors' source curve where the speed rows have 16 and the separation rows 2.  Against the device code (bern_device.h
diff_elev1_at, twice): `val * (p[c] - p[c-1])`, `val * (p[c+1] - p[c])`, the ratio, the product and the fma are 6 roundings per
level with `val = N / tf` shared, 12 for both levels, granted 16 per factor.  A derivation, not a measurement.
"""
import numpy as np

import bezier_algebra_ref as A
import constraint_rows_ref as C
from bezier_algebra_ref import Ref, assert_within, shares, within  # noqa: F401  (the tests take them from here)


def accel(Y, n_veh, dim, R, tf, bound):
    """Rows of obtg_accel for one evaluation row Y[n_veh * dim][n + 1] and its tf.  -> Ref of shape (n_veh, 2 n + R + 1)"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    nc = Y.shape[1]
    n = nc - 1
    assert n >= 1 and Y.shape[0] == n_veh * dim and tf != 0
    v, e = A._ints(Y)
    Tp, Ts = A._dyadic(tf)
    den_row = [2 * c * Tp ** 4 for c in A._binrow(2 * n + R)]
    K_row = C._counts_rows(dim, n, R, 32)
    off = C.square(bound)
    num, mnum, den, K = [], [], [], []
    for veh in range(n_veh):
        rows = [v[(veh * dim + q) * nc:(veh * dim + q + 1) * nc] for q in range(dim)]
        d1 = [A._diff_nums(r, A._absl(r), n) for r in rows]                     # T x', and its majorant
        d2 = [A._diff_nums(a, m, n) for a, m in d1]                             # T^2 x''
        a, m = C._elev_ints(A._normsq_nums([x[0] for x in d2], nc), A._normsq_nums([x[1] for x in d2], nc), 2 * n, R)
        num += a
        mnum += m
        den += den_row
        K += K_row
    num, mnum, E = C._affine(num, mnum, den, 2 * (e + 2 * Ts), -1, off)
    return Ref(num, den, mnum, E, K, (n_veh, 2 * n + R + 1))


def oracle_rows(O, Y, n_veh, dim, R, tf, bound):
    """The ORACLE's acceleration rows: its maximum-speed rows of the first derivative's control points, [n_veh][2 n + R + 1]"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    return O.speed(O.diff(Y, float(tf)), n_veh, dim, R, float(tf), float(bound), True).reshape(n_veh, -1)


# (name, n_veh, dim, deg, R, kind, form): acceleration through obtg_accel -- the shapes of constraint_rows_ref.SPEED_CASES the
# issue names, with degree 1 (every row is bound**2) and degree 2 (a constant acceleration)
ACCEL_TF = C.SPEED_TF
ACCEL_BOUND = 4.0
ACCEL_CASES = (
    [("N = %d" % N, N, 2, 5, 0, "full", "k_normsq_elev<MODE 2>") for N in (1, 64, 65)] +
    [("nc %d, %d-D" % (nc, d), 3, d, nc - 1, 0, "offset" if d == 3 else "full", "k_normsq_elev<MODE 2>") for nc in C.NC_SEP for d in (2, 3)] +
    [("R = 1", 5, 2, 10, 1, "full", "k_normsq_elev<MODE 2, ELEV>"),
     ("R = 100, 3-D", 3, 3, 7, 100, "offset", "k_normsq_elev<MODE 2, ELEV>"),
     ("R = 513", 2, 2, 3, 513, "full", "k_generic_normsq_elev<2>"),
     ("generic dim 1", 3, 1, 6, 0, "full", "k_generic_normsq_elev<2>"),
     ("generic deg 12, R = 5", 3, 2, 12, 5, "offset", "k_generic_normsq_elev<2>"),
     ("generic deg 31, 3-D", 2, 3, 31, 0, "full", "k_generic_normsq_elev<2>"),
     ("deg 1", 3, 2, 1, 0, "full", "k_generic_normsq_elev<2>"),
     ("deg 2", 3, 3, 2, 0, "full", "k_generic_normsq_elev<2>")])


def fixture_rows(golden_dir):
    """tests/golden/accel_rows.npz as (name, Y[4 * dim][deg + 1], dim, deg, R, tf, c[4][2 deg + R + 1]): what the reference's
    Bezier(y, tf=tf).diff().diff().normSquare().elev(R).cpts returned (tests/golden/gen_accel_rows.py)"""
    import os
    g = np.load(os.path.join(golden_dir, "accel_rows.npz"))
    for deg in g["degrees"].tolist():
        for dim in g["dims"].tolist():
            Y = g["Y%d_%d" % (deg, dim)]
            for R in g["elevs"].tolist():
                for it, tf in enumerate(g["tfs"].tolist()):
                    yield ("deg %d dim %d R %d tf %g" % (deg, dim, R, tf), Y, dim, deg, R, tf, g["c%d_%d_%d_%d" % (deg, dim, R, it)])
