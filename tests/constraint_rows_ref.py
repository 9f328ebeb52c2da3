"""The yardstick of the three constraint-row families SLSQP evaluates on every iteration -- obtg_temporal_sep, obtg_speed,
obtg_ang_rate with their reduced and fused forms: every output element in EXACT arithmetic, with the forward-error bound a
float64 evaluation of the same formula has to meet.  Built on tests/bezier_algebra_ref.py (Ref, shares, assert_within, the
integer helpers); no device, no oracle, no reference code.

    separation   (v_i - v_j).normSquare().elev(R) - max_sep**2, point obstacles as constant curves
    speed        diff() [derivative, then elev(1)], normSquare(), elev(R), then sign * c + offset: bound**2 - c or c - bound**2
    angular rate max_rate**2 - num_k / den_k, num = (y'' x' - x'' y')^2, den = (x'^2 + y'^2)^2, both elevated by 4 R

max_sep**2, bound**2, max_rate**2 enter as the float64 Python's `**` gives (include/obtg.h; csrc/tables.cpp square_as_python).

Separation and speed return a bezier_algebra_ref.Ref: per element the exact value, the majorant M (the same formula on
magnitudes) and the count K of rounded operations; a candidate c passes when |c - value| <= K * 2^-53 * M.

The first difference.  v_i - v_j of a separation pair is formed by every kernel as ONE subtraction of two inputs (bern_device.h
normsq_elev_body `a[q][c] = vi[..] - vj[..]`, bern_kernels.hip k_generic_normsq_elev `(vi - vj) * bn[c]`): one rounding of its
exact value.  Its majorant is therefore |v_i - v_j|, not |v_i| + |v_j|, at a cost of 1 in K per factor -- which keeps the bound
sharp for a swarm far from the origin.  The derivative of a SPEED row is not formed that way, neither on the device nor in
the reference: Bezier.diff() is cpts.dot(diffMatrix) (bezier.py:497-519, 1101-1124), `p_c * (-n/T) + p_(c+1) * (n/T)` (the same
line in normsq_elev_body, diff_elev1 and k_generic_normsq_elev), so each product is rounded at the magnitude of the POSITION.
With |P_(i+1) - P_i| as that majorant the reference's own arithmetic on a swarm offset by 1e6 sits 8.7e3 (the NumPy statement
of bezier.py:514) to 2.8e4 (the oracle) bounds outside the count (tests/test_constraint_rows_ref.py
test_diff_majorant_is_the_sum_of_magnitudes keeps the figures), so that count would be wrong, not the kernels: the derivative's
majorant is (n/T)(|P_i| + |P_(i+1)|), as bezier_algebra_ref.diff has it.  Every later subtraction is a sum of magnitudes in all three families.

The counts K, against the device code (u = one rounding; a sum of T terms is granted T whatever its association, so the order
of an MFMA accumulation, the folding of the symmetric product and any BLAS order on the reference's side need no special
case; a fused multiply-add only lowers a count).  T_k = min(n, k) - max(0, k - n) + 1 terms of the product's coefficient k,
Te_k = the terms of elevation column k.

  separation, specialised body (bern_device.h), R = 0
      `a[q][c] = vi - vj`                                   1 per factor                                  2
      normsq_coeffs `u[q][j] = Cn[j] * a[q][j]`             1 per factor (C(n, j) is exact up to n = 57)  2
      the folded chain `so = fma(u, u, so)`, `dg`           <= d T_k terms                                d T_k
      `fma(2.0, so, dg)`                                                                                  1
      table entry S_k = (d/2) / C(2n, k) (tables.cpp folded_product_weights): binomial, quotient          2
      `c[k] = Sk[k] * s`                                                                                  1
      `p.sign * cf[k] + p.offset`                                                                         1
                                                                            counted d T_k + 9, granted d T_k + 20
  separation, specialised body, R > 0 (elev_rows_mfma / elev_at / sep_elev_coop_body: out_k = offset + sum_j ch_j T[j][k])
      c_j as above without its last line                    <= d (n + 1) + 8
      table entry T[j][k] (elev_table_frag / elev_table_T_ld: long double chain, rounded once)            2
      the chain from `offset`, by matrix row or by MFMA accumulation (zero entries add nothing)           Te_k
                                                        counted d (n + 1) + Te_k + 10, granted d (n + 1) + Te_k + 28
  separation, generic kernels (bern_kernels.hip k_generic_normsq_elev, generic_normsq_elev_tail)
      `ah[e] = (vi - vj) * bn[c]`                           2 per factor (bn: a long double chain of <= 511 steps, 1/2 u,
                                                            rounded once: counted 2 wherever a binomial row is read)  6
      conv_at per dimension, `s += ...`                     d T_k + d
      `(0.5 * dim) * s / b2n[k]`                            product, entry, quotient                      4
      R = 0: `p.sign * c + p.offset`                                                                      1
                                                                        counted d T_k + d + 11, granted d T_k + 20
      R > 0: `ch[k] = c * b2n[k]` 1; conv_at(ch, bR) Te_k, bR's entry 2; `/ b2nR[k]` 3; `p.sign * s + p.offset` 1
                                                counted d (n + 1) + d + Te_k + 17, granted d (n + 1) + Te_k + 28
  speed: the same bodies in MODE 1 (vehicle).  Each factor is the derivative elevated by one:
      `val = N / tf` 1; `t[c] = v * (-val) + v * val` 2; `t[c-1] * (c / N) + t[c] * ((N - c) / N)` 3 (ratio, product, sum)
                                                            6 per factor, granted 8 as bezier_algebra_ref.diff: 16
      in place of the separation's 2 for its first difference     -> the separation's grant + 14
  angular rate (k_dynamics / k_dynamics2 / k_dynamics_elev through diff_elev1, ang_scale, ang_raw_num, ang_raw_den,
  fold_square_at / dyn2_tail; k_generic_angrate through conv_at, conv_tile, conv_pairs), m = the degree the products run at
  (n, or n + R where the position is elevated first), E = 0 or, elevated first, (n + 1) + 10 for `conv_at(tm, bR) / bm[k]`:
      x', y'      E + 8;     x'', y''   E + 16 (diff of a row that carries 8)
      q = y'' x' - x'' y'    operands 24 + 2 E; each product a chain of <= m + 1 terms, its two scalings (`u = Cn * a`,
                             `d * bm[c]`) and, in k_generic_angrate, `(t1 / c - t2 / c) * c`: granted m + 1 + 14; the
                             difference 1                                                   K_q = 2 E + m + 40
      s = x'^2 + y'^2        operands 16 + 2 E; two chains 2 (m + 1), as above 14, the sum 1   K_s = 2 E + 2 m + 33
      num = q^2, den = s^2   twice the operand, a chain of <= 2 m + 1 terms, weights / scalings 14
                                                            KN = 2 K_q + 2 m + 15,  KD = 2 K_s + 2 m + 15
      products first (k_dynamics_elev): the elevation by 4 R of both, <= 4 n + 1 terms and its table entry: + 4 n + 11
  The slack over the counted figures is 9 to 18 roundings per row family and more where folding halves a chain; it is there so
  that one formula serves every launch form of a family.  A derivation, not a measurement.

The angular rate is a quotient, so it gets a quotient test in place of a majorant.  With exact N_k, D_k, majorants MN_k, MD_k
and counts KN, KD the device holds Nh = N + dN, |dN| <= KN u MN, and Dh = D + dD, |dD| <= KD u MD (u = 2^-53).  It returns
c = fl(m2 - qh), qh = fl(Nh / Dh), m2 = fl(max_rate**2): qh = (Nh / Dh)(1 + e1), c = (m2 - qh)(1 + e2), |e1|, |e2| <= u.  Put
q = m2 - c, the quotient the candidate stands for.  Then qh = q + e2' c with |e2'| <= u / (1 - u), and from qh Dh = Nh (1 + e1):
    q D - N = dN + e1 Nh - q dD - e2' c Dh,
    |q D - N| <= u (KN MN + |Nh| + KD |q| MD + |c| |Dh| / (1 - u)) <= 2^-53 ((KN + 2) MN + (KD |q| + 2 |c|) MD)
with |Nh| <= (1 + KN u) MN and |Dh| <= (1 + KD u) MD; the 2s take the second-order terms (KN u < 1e-12).  The test is that
inequality in exact arithmetic.  It is loose by itself where D is small against MD (a vehicle that nearly stops) and tight
elsewhere; a common factor of N, D (the binomial C(4 m, k) the kernels leave in both) drops out of it.
Where N = D = 0 the candidate must be NaN; where D = 0 != N it must be -sign(N) * inf (c = m2 - N / (+0)).
"""
import math
from fractions import Fraction

import numpy as np

import bezier_algebra_ref as A
from bezier_algebra_ref import Ref, shares, share, assert_within, within  # noqa: F401  (the tests take them from here)

UNIT = Fraction(1, 1 << A.UNIT_BITS)
DBL_MAX = Fraction(float.fromhex("0x1.fffffffffffffp+1023"))


def square(x):
    """x**2 as Python gives it (libm pow): what the kernels receive as max_sep^2 / bound^2 / max_rate^2"""
    return float(x) ** 2


def all_pairs(n_obj):
    return [(i, j) for i in range(n_obj) for j in range(i + 1, n_obj)]


def _elev_ints(num, mnum, n_in, R):
    """conv with C(R, .) of rows that are C(n_in, k) times Bernstein coefficients: C(n_in + R, k) times the elevated ones"""
    if R == 0:
        return num, mnum
    bR = A._binrow(R)
    return A._conv(num, bR), A._conv(mnum, bR)


def _affine(num, mnum, den, e, sign, off):
    """sign * (num / den * 2^e) + off for the float `off`, over the common exponent: (num', mnum', e')"""
    p, s = A._dyadic(off)
    E = min(e, -s)
    up, uo = 1 << (e - E), 1 << (-s - E)
    return ([sign * a * up + p * d * uo for a, d in zip(num, den)],
            [m * up + abs(p) * d * uo for m, d in zip(mnum, den)], E)


def _counts_rows(d, n, R, first):
    """K per element of one separation / speed row; first = the count of the two factors' first operation (2 or 16)"""
    nc = n + 1
    if R == 0:
        return [d * A._terms(nc, nc, k) + 18 + first for k in range(2 * n + 1)]
    return [d * nc + A._terms(2 * n + 1, R + 1, k) + 26 + first for k in range(2 * n + R + 1)]


# ---------------------------------------------------------------------------------------------------------------------
#  separation
# ---------------------------------------------------------------------------------------------------------------------
def _objects(Y, n_veh, dim, obs):
    """-> (integer rows per object [dim][nc], e): the vehicles of Y[n_veh * dim][nc], then the point obstacles as constant curves"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    nc = Y.shape[1]
    assert Y.shape[0] == n_veh * dim
    flat = [Y.reshape(-1)]
    if obs is not None and len(obs):
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, dim)
        flat.append(np.repeat(obs.reshape(-1), nc))
    v, e = A._ints(np.concatenate(flat))
    n_obj = len(v) // (dim * nc)
    return [[v[(o * dim + q) * nc:(o * dim + q + 1) * nc] for q in range(dim)] for o in range(n_obj)], e


def temporal_sep(Y, n_veh, dim, R, max_sep, obs=None, pairs=None):
    """Rows of obtg_temporal_sep for one evaluation row Y[n_veh * dim][n + 1]: every pair of the n_veh + len(obs) objects in
    lexicographic order, or the listed `pairs`.  -> Ref of shape (P, 2 n + R + 1)"""
    objs, e = _objects(Y, n_veh, dim, obs)
    nc = len(objs[0][0])
    n = nc - 1
    if pairs is None:
        pairs = all_pairs(len(objs))
    den_row = [2 * c for c in A._binrow(2 * n + R)]
    K_row = _counts_rows(dim, n, R, 2)
    off = -square(max_sep)
    num, mnum, den, K = [], [], [], []
    for i, j in pairs:
        D = [list(map(int.__sub__, objs[i][q], objs[j][q])) for q in range(dim)]
        a, m = _elev_ints(A._normsq_nums(D, nc), A._normsq_nums([A._absl(r) for r in D], nc), 2 * n, R)
        num += a
        mnum += m
        den += den_row
        K += K_row
    num, mnum, E = _affine(num, mnum, den, 2 * e, 1, off)
    return Ref(num, den, mnum, E, K, (len(pairs), 2 * n + R + 1))


# ---------------------------------------------------------------------------------------------------------------------
#  speed
# ---------------------------------------------------------------------------------------------------------------------
def speed(Y, n_veh, dim, R, tf, bound, is_max, majorant="sum"):
    """Rows of obtg_speed for one evaluation row and its tf.  -> Ref of shape (n_veh, 2 n + R + 1).
    majorant = "difference": the derivative's majorant as (n / T) |P_(i+1) - P_i| -- NOT what any float64 evaluation of
    diff() meets (module docstring); kept so that the test which shows it can form it."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    nc = Y.shape[1]
    n = nc - 1
    assert n >= 1 and Y.shape[0] == n_veh * dim and tf != 0
    v, e = A._ints(Y)
    Tp, Ts = A._dyadic(tf)
    den_row = [2 * c * Tp * Tp for c in A._binrow(2 * n + R)]
    K_row = _counts_rows(dim, n, R, 16)
    sign, off = (-1, square(bound)) if is_max else (1, -square(bound))
    num, mnum, den, K = [], [], [], []
    for veh in range(n_veh):
        rows = [v[(veh * dim + q) * nc:(veh * dim + q + 1) * nc] for q in range(dim)]
        dd = [A._diff_nums(r, A._absl(r), n) for r in rows]                     # T * diff, and its majorant
        D = [x[0] for x in dd]
        Dm = [x[1] for x in dd]
        if majorant != "sum":
            # |c (a_c - a_(c-1))| + |(n - c)(a_(c+1) - a_c)|: the two first differences taken as single roundings
            Dm = [[(c * abs(r[c] - r[c - 1]) if c > 0 else 0) + ((n - c) * abs(r[c + 1] - r[c]) if c < n else 0)
                   for c in range(nc)] for r in rows]
        a, m = _elev_ints(A._normsq_nums(D, nc), A._normsq_nums(Dm, nc), 2 * n, R)
        num += a
        mnum += m
        den += den_row
        K += K_row
    num, mnum, E = _affine(num, mnum, den, 2 * (e + Ts), sign, off)
    return Ref(num, den, mnum, E, K, (n_veh, 2 * n + R + 1))


# ---------------------------------------------------------------------------------------------------------------------
#  the finiteness condition of the generic rows (generic_normsq_elev_tail forms conv_at(ch, C(R, .)) before `/ C(2n + R, k)`)
# ---------------------------------------------------------------------------------------------------------------------
def unnormalised_peak(ref_rows, n, R):
    """The largest majorant of the sums sum_j C(2n, j) c_j C(R, k - j) the any-degree kernel forms for the rows of a
    temporal_sep / speed Ref computed with max_sep = bound = 0 (so that M is the product's alone): M_k * C(2n + R, k).
    Every partial sum of a chain is bounded by it, so the row is finite while it stays below DBL_MAX."""
    bo = A._binrow(2 * n + R)
    L = 2 * n + R + 1
    return max(ref_rows.majorant(i) * bo[i % L] for i in range(len(ref_rows.num)))


def longest_row_case():
    """Two planar vehicles of degree 2 at R = 1019, scaled by a power of two so that the unnormalised peak lies in
    [DBL_MAX / 8, DBL_MAX / 2) -> (Y, peak)"""
    n, R = 2, 1019
    Y = swarm(41, 2, 2, n)
    peak = unnormalised_peak(temporal_sep(Y, 2, 2, R, 0.0), n, R)
    while peak >= DBL_MAX / 2:
        Y, peak = Y / 2, peak / 4
    while peak < DBL_MAX / 8:
        Y, peak = Y * 2, peak * 4
    return Y, peak


# ---------------------------------------------------------------------------------------------------------------------
#  angular rate
# ---------------------------------------------------------------------------------------------------------------------
class AngRef(object):
    """Per element (flat over (n_veh, 4 (n + R) + 1)): integers N, D, MN, MD with num / den = N / D (a common positive factor
    left in), the counts KN, KD and m2 = fl(max_rate**2)."""

    def __init__(self, N, D, MN, MD, KN, KD, m2, shape, peak=None):
        self.N, self.D, self.MN, self.MD, self.KN, self.KD, self.m2, self.shape = N, D, MN, MD, KN, KD, Fraction(m2), tuple(shape)
        self.peak = peak          # largest majorant of the unnormalised sums C(4m, k) num_k, C(4m, k) den_k (see ang_rate)

    def value(self, i):
        return self.m2 - Fraction(self.N[i], self.D[i]) if self.D[i] else None

    def nearest(self):
        return np.array([float(self.value(i)) if self.D[i] else math.nan for i in range(len(self.N))]).reshape(self.shape)


def ang_counts(n, R, order):
    """(KN, KD) of a row; order as obtg_ctx_ang_rate_order_in_effect: 1 = the position elevated first (products at degree
    n + R), 0 / 2 = products at degree n, then the elevation by 4 R of numerator and denominator"""
    first = order == 1 and R > 0
    E = (n + 1) + 10 if first else 0
    m = n + R if first else n
    Kq = 2 * E + m + 40
    Ks = 2 * E + 2 * m + 33
    KN, KD = 2 * Kq + 2 * m + 15, 2 * Ks + 2 * m + 15
    if R > 0 and not first:
        KN, KD = KN + 4 * n + 11, KD + 4 * n + 11
    return KN, KD


def _scaled(row, n):
    return [c * x for c, x in zip(A._binrow(n), row)]


def ang_rate(Y, n_veh, R, tf, max_rate, order=0):
    """Rows of obtg_ang_rate (dim 2) for one evaluation row and its tf -> AngRef.  Elevation commutes with diff, mul and
    add exactly, and on magnitudes too, so N, D, MN, MD do not depend on the order of operations; only the counts do.
    AngRef.peak: the any-degree kernel (k_generic_angrate) divides C(4m, k) num_k by C(4m, k) den_k, m = n + R, both formed
    as plain sums -- `first[i] / da`, `(sn[i] / b4m[k]) / (sd[i] / b4m[k])` --, so its rows are finite only while the majorants
    of those sums, whose largest is `peak`, stay below DBL_MAX (include/obtg.h).  k_dynamics_elev scales its binomial row by a
    power of two (tables.cpp elev_conv_padded `normalise`) and k_dynamics2 multiplies by weights below 1: no such condition."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    nc = Y.shape[1]
    n = nc - 1
    assert n >= 1 and Y.shape[0] == 2 * n_veh and tf != 0
    v, e = A._ints(Y)                                                  # (the inputs' common power of two cancels in N / D)
    peak = Fraction(0)
    Tp, Ts = A._dyadic(tf)
    b4R = A._binrow(4 * R)
    KN, KD = ang_counts(n, R, order)
    N, D, MN, MD = [], [], [], []
    for veh in range(n_veh):
        d1, d2, m1, m2 = [], [], [], []
        for q in range(2):
            r = v[(2 * veh + q) * nc:(2 * veh + q + 1) * nc]
            a, am = A._diff_nums(r, A._absl(r), n)                     # T x'
            b, bm = A._diff_nums(a, am, n)                             # T^2 x''
            d1.append(_scaled(a, n)); m1.append(_scaled(am, n)); d2.append(_scaled(b, n)); m2.append(_scaled(bm, n))
        # C(2n, k) times q = y'' x' - x'' y' (T^3) and s = x'^2 + y'^2 (T^2)
        Q = list(map(int.__sub__, A._conv(d2[1], d1[0]), A._conv(d2[0], d1[1])))
        Qm = list(map(int.__add__, A._conv(m2[1], m1[0]), A._conv(m2[0], m1[1])))
        S = list(map(int.__add__, A._conv(d1[0], d1[0]), A._conv(d1[1], d1[1])))
        Sm = list(map(int.__add__, A._conv(m1[0], m1[0]), A._conv(m1[1], m1[1])))
        num, numm = A._conv(Q, Q), A._conv(Qm, Qm)                     # C(4n, k) num T^6
        den, denm = A._conv(S, S), A._conv(Sm, Sm)                     # C(4n, k) den T^4
        if R:
            num, numm, den, denm = (A._conv(x, b4R) for x in (num, numm, den, denm))
        # num / den = [num' / T^6] / [den' / T^4] = num' 2^(2 Ts) / (den' Tp^2)
        peak = max(peak, Fraction(max(numm) << (6 * Ts), Tp ** 6), Fraction(max(denm) << (4 * Ts), Tp ** 4))
        N += [x << (2 * Ts) for x in num]
        MN += [x << (2 * Ts) for x in numm]
        D += [x * Tp * Tp for x in den]
        MD += [x * Tp * Tp for x in denm]
    return AngRef(N, D, MN, MD, KN, KD, square(max_rate), (n_veh, 4 * (n + R) + 1), peak * Fraction(2) ** (4 * e))


def ang_shares(cand, ref, dd=False):
    """The quotient test per element -> (shares as floats, verdicts).  Share = |q D - N| over its bound (0 where both are 0).
    dd: the bound of a row formed in double-double arithmetic from tables that carry 64 bits (k_angrate_dd; tables.cpp
    angrate_dd_tables: (hi, lo) of a long double) and rounded once -- N and D are off by their counts at 2^-64 instead of
    2^-53, `n / tf` is one float64 (num / den goes with its square: 2 u |q|, granted 4), the result one rounding of c:
        |q D - N| <= 2^-64 ((KN + 2) MN + (KD |q| + 2 |c|) MD) + 2^-53 (|c| + 4 |q|) |D|"""
    c = np.asarray(cand, dtype=np.float64)
    assert c.shape == ref.shape, "shape %s, expected %s" % (c.shape, ref.shape)
    out = np.zeros(c.size)
    ok = np.ones(c.size, dtype=bool)
    for i, x in enumerate(c.reshape(-1).tolist()):
        N, D, MN, MD = ref.N[i], ref.D[i], ref.MN[i], ref.MD[i]
        if D == 0:
            if N == 0:
                good = math.isnan(x)
            else:
                good = math.isinf(x) and (x < 0) == (N > 0)
            ok[i], out[i] = good, (0.0 if good else math.inf)
            continue
        if not math.isfinite(x):
            ok[i], out[i] = False, math.inf
            continue
        cf = Fraction(x)
        q = ref.m2 - cf
        lhs = abs(q * D - N)
        rhs = UNIT * ((ref.KN + 2) * MN + (ref.KD * abs(q) + 2 * abs(cf)) * MD)
        if dd:
            rhs = rhs / 2048 + UNIT * (abs(cf) + 4 * abs(q)) * abs(D)
        ok[i] = lhs <= rhs
        out[i] = float(lhs / rhs) if rhs else (0.0 if lhs == 0 else math.inf)
    return out.reshape(ref.shape), ok.reshape(ref.shape)


def ang_assert_within(cand, ref, what=""):
    s, ok = ang_shares(cand, ref)
    if not ok.all():
        i = int(np.argmax(np.where(ok, -1.0, s).reshape(-1)))
        v = ref.value(i)
        raise AssertionError("%s: %d of %d elements fail the quotient test; worst at flat index %d: got %r, exact %r, share %.3g"
                             % (what, int((~ok).sum()), ok.size, i, float(np.asarray(cand, dtype=np.float64).reshape(-1)[i]),
                                float(v) if v is not None else None, s.reshape(-1)[i]))
    return float(s.max()) if s.size else 0.0


def ang_within(cand, ref):
    return bool(ang_shares(cand, ref)[1].all())


def ang_rel_units(cand, ref, rows):
    """Largest |c - exact| / |exact| over the listed vehicles' rows in units of 2^-53 (the record of the double-double pass)"""
    c = np.asarray(cand, dtype=np.float64).reshape(ref.shape)
    worst = 0.0
    for r in rows:
        for k in range(ref.shape[1]):
            ex = ref.value(r * ref.shape[1] + k)
            if ex is None or ex == 0 or not math.isfinite(c[r, k]):
                continue
            worst = max(worst, float(abs(Fraction(float(c[r, k])) - ex) / abs(ex) / UNIT))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
#  reduced forms: the minimum of a row against the row's bounds
# ---------------------------------------------------------------------------------------------------------------------
def min_within(cand, ref):
    """cand[P]: per row of ref the minimum of SOME float64 evaluation that meets the bound: cand_p is within the bound of an
    element k, and no element's upper end lies below it"""
    c = np.asarray(cand, dtype=np.float64).reshape(-1)
    P, L = ref.shape
    assert c.size == P
    for p, x in enumerate(c.tolist()):
        if not math.isfinite(x):
            return False
        fx = Fraction(x)
        lo_ok = hit = False
        for k in range(L):
            i = p * L + k
            val, b = ref.value(i), ref.K[i] * UNIT * ref.majorant(i)
            if fx > val + b:
                break
            hit = hit or abs(fx - val) <= b
        else:
            lo_ok = True
        if not (lo_ok and hit):
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
#  inputs and cases both test modules use
# ---------------------------------------------------------------------------------------------------------------------
TOUCH_SEP = 0.75          # max_sep of the "edges" swarm: vehicles 0, 1 exactly that far apart (2-D: (d/2)|D|^2 = max_sep^2)


def swarm(seed, n_veh, dim, deg, kind="full"):
    """Y[n_veh * dim][deg + 1].
    full    full-mantissa rows: uniform(-10, 10) drawn at float64 resolution, every fourth vehicle times 1e-3 (slow, small)
    offset  1e6 + uniform(-2, 2): a swarm far from the origin with separations of order 1
    edges   `full`, then vehicle 1 = vehicle 0 + (TOUCH_SEP, 0, ..) on coordinates rounded to 2^-20 (the difference is exact:
            with dim 2 that pair's row is all zeros), and vehicle 3 = vehicle 2 (coincident: the row is -max_sep^2)"""
    rng = np.random.default_rng(seed)
    nc = deg + 1
    Y = rng.uniform(-10, 10, (n_veh, dim, nc))
    Y[3::4] *= 1e-3
    if kind == "offset":
        Y = 1e6 + rng.uniform(-2, 2, (n_veh, dim, nc))
    elif kind == "edges":
        assert n_veh >= 4
        Y[0] = np.round(Y[0] * 2.0 ** 20) / 2.0 ** 20
        Y[1] = Y[0]
        Y[1, 0] += TOUCH_SEP
        Y[3] = Y[2]
    else:
        assert kind == "full"
    return np.ascontiguousarray(Y.reshape(n_veh * dim, nc))


def rows_batch(seed, B, n_veh, dim, deg, kind="full"):
    return np.stack([swarm(seed + 1000 * b, n_veh, dim, deg, kind) for b in range(B)])


def point_obstacles(seed, M, dim):
    return np.random.default_rng(seed).uniform(-10, 10, (M, dim))


NC_SEP = (4, 6, 8, 9, 11, 16, 21)         # csrc/obtg_internal.h OBTG_NC_SEP
NC_DYN = (4, 6, 8, 9, 11, 16)             # OBTG_NC_DYN


# ---- the separation planner restated (bern_kernels.hip plan_temporal_sep, launch_ns_t, sep_elev_coop_lds): which form a launch takes
def sep_form(n_obj, dim, deg, R, B, pair_begin=0, pair_count=None, min_only=False):
    """-> dict(kernel, waves, groups_per_wg, wgs_per_row, staging, tile_rows)"""
    nc = deg + 1
    P = n_obj * (n_obj - 1) // 2
    if pair_count is None:
        pair_count = P - pair_begin
    if not (nc in NC_SEP and dim in (2, 3) and R <= 512):                        # fast_shape
        return dict(kernel="k_generic_normsq_elev", waves=1, groups_per_wg=0, wgs_per_row=pair_count, staging="none", tile_rows=0)
    vlen = dim * nc
    vp = vlen + 1 if vlen % 2 == 0 else vlen
    L = 2 * deg + 1
    tpf = L + 1 if L % 2 == 0 else L
    groups_total = (pair_count + 63) // 64
    if 8 * n_obj * vp <= 24 * 1024 or n_obj <= 128:                              # plan_temporal_sep: `row_bytes <= 24 * 1024 || ...`
        waves = 4 if groups_total >= 4 else groups_total
        gpw = 16
        while gpw > waves and B * ((groups_total + gpw - 1) // gpw) < 4096:
            gpw >>= 1
        gpw = max(gpw, waves)
        pairs = all_pairs(n_obj)
        slots = 0
        for it0 in range(pair_begin, pair_begin + pair_count, 64 * gpw):
            last = min(pair_begin + pair_count, it0 + 64 * gpw) - 1
            (fx, fy), (lx, ly) = pairs[it0], pairs[last]
            nI = lx - fx + 1
            nA = (ly - fy + 1) if nI == 1 else n_obj - fy
            nB = 0 if nI == 1 else max(0, ((n_obj - 1) if nI >= 3 else ly) - (fx + 2) + 1)
            slots = max(slots, nI + nA + nB)
        stage_all = n_obj <= slots
        stage_slots = n_obj if stage_all else slots
        staging, wgs = ("whole" if stage_all else "slots"), (groups_total + gpw - 1) // gpw
    else:
        waves, gpw, stage_all, stage_slots, staging = 4, 8, False, 8 + 64, "tiled"
        wgs = sum(len(range(((i0 + 1) // 64) * 64, n_obj, 64)) for i0 in range(0, n_obj - 1, 8))    # (a launch of every pair)
    stage = 8 * stage_slots * vp
    kernel, tile_rows = "k_normsq_elev", 0
    if min_only:
        kernel = "k_normsq_elev<MINONLY, ELEV>" if R > 0 else "k_normsq_elev<MINONLY>"
    elif R > 0:
        kernel, tile_rows = "k_normsq_elev<ELEV>", 64
        if stage_all and staging != "tiled" and L + R <= 128 and n_obj < 65536:  # sep_elev_coop_lds (its LDS stays below 160 KB here)
            kernel, waves = "k_sep_elev_coop", 4
    else:
        for tr in (64, 32, 16):
            tile_rows = tr
            if stage + 8 * waves * tr * tpf <= 76 * 1024:                        # launch_ns_t against kNsLdsBudget
                break
    return dict(kernel=kernel, waves=waves, groups_per_wg=gpw, wgs_per_row=wgs, staging=staging, tile_rows=tile_rows)


# (name, n_veh, dim, deg, R, n_obs, kind, B, (pair_begin, pair_count) or None, what the planner must answer)
SEP_CASES = (
    [("pairs %d" % pc, 24, 2, 5, 0, 0, "full", 2, (5, pc), dict(kernel="k_normsq_elev", waves=w, wgs_per_row=g))
     for pc, w, g in ((63, 1, 1), (64, 1, 1), (65, 2, 1), (255, 4, 1), (256, 4, 1), (257, 4, 2))] +
    [("64-row tile", 12, 2, 10, 0, 0, "edges", 3, None, dict(kernel="k_normsq_elev", tile_rows=64, waves=2, staging="whole")),
     ("N = 20, deg 20", 20, 2, 20, 0, 0, "full", 2, None, dict(kernel="k_normsq_elev", tile_rows=64, waves=3)),
     ("32-row tile", 21, 2, 20, 0, 0, "full", 2, None, dict(kernel="k_normsq_elev", tile_rows=32, waves=4, staging="whole")),
     ("N = 100, deg 20", 100, 2, 20, 0, 0, "full", 1, None, dict(kernel="k_normsq_elev", tile_rows=32, waves=4, staging="whole")),
     ("16-row tile", 110, 2, 20, 0, 0, "offset", 1, None, dict(kernel="k_normsq_elev", tile_rows=16, waves=4, staging="whole")),
     ("slot staging", 300, 2, 3, 0, 0, "full", 1, (250, 1500), dict(kernel="k_normsq_elev", staging="slots")),
     ("tiled", 140, 2, 10, 0, 0, "full", 1, None, dict(kernel="k_normsq_elev", staging="tiled", waves=4)),
     ("offset 1e6", 9, 3, 5, 0, 2, "offset", 3, None, dict(kernel="k_normsq_elev"))] +
    [("nc %d, %d-D, obstacles" % (nc, d), 5, d, nc - 1, 0, 2, "edges", 2, None, dict(kernel="k_normsq_elev", staging="whole"))
     for nc in NC_SEP for d in (2, 3)] +
    # R > 0: L = 2 deg + 1; L + R at 16 t and 16 t + 1, at the cooperative kernel's limit 128 | 129, at the last fast R | first generic
    [("R = 1", 7, 2, 5, 1, 1, "edges", 3, None, dict(kernel="k_sep_elev_coop")),
     ("L + R = 16", 7, 3, 5, 5, 0, "full", 2, None, dict(kernel="k_sep_elev_coop")),
     ("L + R = 17", 7, 2, 5, 6, 0, "offset", 2, None, dict(kernel="k_sep_elev_coop")),
     ("L + R = 128", 13, 2, 10, 107, 0, "edges", 2, None, dict(kernel="k_sep_elev_coop")),
     ("L + R = 129", 13, 2, 10, 108, 0, "edges", 2, None, dict(kernel="k_normsq_elev<ELEV>", staging="whole")),
     ("elevated, slot staging", 300, 2, 3, 9, 0, "full", 1, (250, 700), dict(kernel="k_normsq_elev<ELEV>", staging="slots")),
     ("elevated, tiled", 140, 2, 10, 3, 0, "full", 1, None, dict(kernel="k_normsq_elev<ELEV>", staging="tiled")),
     ("R = 512", 4, 2, 3, 512, 1, "edges", 1, None, dict(kernel="k_normsq_elev<ELEV>")),
     ("R = 513", 4, 2, 3, 513, 1, "edges", 1, None, dict(kernel="k_generic_normsq_elev")),
     ("deg 20, R = 30, 3-D", 6, 3, 20, 30, 0, "full", 1, None, dict(kernel="k_sep_elev_coop"))] +
    # the any-degree kernel: dim 1, degrees off the list
    [("generic dim 1", 6, 1, 5, 0, 1, "full", 2, None, dict(kernel="k_generic_normsq_elev")),
     ("generic dim 1, R = 4", 6, 1, 5, 4, 0, "offset", 2, None, dict(kernel="k_generic_normsq_elev")),
     ("generic deg 2", 5, 2, 2, 0, 0, "edges", 2, None, dict(kernel="k_generic_normsq_elev")),
     ("generic deg 12, R = 7", 5, 3, 12, 7, 1, "edges", 2, None, dict(kernel="k_generic_normsq_elev")),
     ("generic deg 31", 4, 2, 31, 0, 0, "edges", 2, None, dict(kernel="k_generic_normsq_elev")),
     ("generic deg 31, R = 66", 4, 2, 31, 66, 0, "full", 1, None, dict(kernel="k_generic_normsq_elev"))])

SEP_MAX_SEP = TOUCH_SEP

# (name, n_veh, dim, deg, R, kind, tf per row, form): speed through obtg_speed
SPEED_TF = (7.3, 0.013, 1.0)
SPEED_CASES = (
    [("N = %d" % N, N, 2, 5, 0, "full", "k_normsq_elev<MODE 1>") for N in (1, 64, 65)] +
    [("nc %d, %d-D" % (nc, d), 3, d, nc - 1, 0, "offset" if d == 3 else "full", "k_normsq_elev<MODE 1>") for nc in NC_SEP for d in (2, 3)] +
    [("R = 1", 5, 2, 10, 1, "full", "k_normsq_elev<MODE 1, ELEV>"),
     ("R = 100, 3-D", 3, 3, 7, 100, "offset", "k_normsq_elev<MODE 1, ELEV>"),
     ("R = 512", 2, 2, 3, 512, "full", "k_normsq_elev<MODE 1, ELEV>"),
     ("R = 513", 2, 2, 3, 513, "full", "k_generic_normsq_elev<1>"),
     ("generic dim 1", 3, 1, 6, 0, "full", "k_generic_normsq_elev<1>"),
     ("generic deg 12, R = 5", 3, 2, 12, 5, "offset", "k_generic_normsq_elev<1>"),
     ("generic deg 31, 3-D", 2, 3, 31, 0, "full", "k_generic_normsq_elev<1>")])
SPEED_BOUNDS = (5.0, 0.3)                 # max speed, min speed (the second bound of one pass)


def speed_form(dim, deg, R):
    return "generic" if not ((deg + 1) in NC_SEP and dim in (2, 3) and R <= 512) else ("fast" if R == 0 else "fast elevated")


# ---- angular rate: the launch form by shape (bern_kernels.hip dyn_fast, dyn_fast_elev, ang_rate_order_in_effect, launch_ang_rate)
def _conv_pairs_ok(n_out, T):
    Tn = (n_out + T - 1) // T
    return Tn % 4 == 0 and Tn // 2 <= 32


def angrate_balanced(m):
    return _conv_pairs_ok(4 * m + 1, 8)


def angrate_balanced2(m):
    return _conv_pairs_ok(2 * m + 1, 4) and 2 * m + 1 <= 256


def ang_form(deg, R, requested_order):
    """-> (kernel, order in effect)"""
    nc = deg + 1
    if R == 0:
        return ("k_dynamics2" if nc in NC_DYN else "k_generic_angrate"), 0
    if requested_order != 1 and nc in NC_DYN and deg <= 15 and 4 * R <= 1000:
        return ("k_dynamics_elev + k_angrate_dd" if requested_order == 2 else "k_dynamics_elev"), requested_order
    return "k_generic_angrate", 1


# (name, n_veh, deg, R, requested order, kind, form)
ANG_TF = (7.3, 0.013, 1.0)
ANG_CASES = (
    [("nc %d" % nc, 3, nc - 1, 0, 0, "full", ("k_dynamics2", 0)) for nc in NC_DYN] +
    [("N = 65", 65, 5, 0, 0, "full", ("k_dynamics2", 0)),
     ("elev R = 1", 3, 15, 1, 0, "full", ("k_dynamics_elev", 0)),
     ("elev R = 12", 3, 10, 12, 0, "full", ("k_dynamics_elev", 0)),
     ("elev R = 100", 2, 10, 100, 0, "full", ("k_dynamics_elev", 0)),
     ("elev 4 R = 1000", 2, 15, 250, 0, "full", ("k_dynamics_elev", 0)),
     ("order 1, R = 12", 3, 10, 12, 1, "full", ("k_generic_angrate", 1)),
     ("order 2, R = 12", 3, 10, 12, 2, "full", ("k_dynamics_elev + k_angrate_dd", 2)),
     ("deg 16, R = 3: no elevated kernel", 2, 16, 3, 0, "full", ("k_generic_angrate", 1)),
     ("m = 250", 2, 6, 244, 0, "full", ("k_generic_angrate", 1))])


def ang_tf_inside(Y, n_veh, R, tf, lo=7, hi=1):
    """tf times the power of two that puts AngRef.peak into [DBL_MAX / 2^lo, DBL_MAX / 2^hi): a row just inside the any-degree
    kernel's finiteness condition (the numerator goes with tf^-6: one step of tf is 2^6 in the peak)"""
    peak = ang_rate(Y, n_veh, R, tf, 1.0).peak
    while peak >= DBL_MAX / 2 ** hi:
        tf, peak = tf * 2, peak / 64
    while peak < DBL_MAX / 2 ** lo:
        tf, peak = tf / 2, peak * 64
    assert DBL_MAX / 2 ** lo <= peak < DBL_MAX / 2 ** hi
    return tf
# the any-degree kernel's four schedules: (deg, R) with m = deg + R, deg + 1 off OBTG_NC_DYN or the order set to 1
ANG_GENERIC_M = {(True, True): None, (True, False): None, (False, True): None, (False, False): None}
for _m in range(2, 251):
    _key = (angrate_balanced(_m), angrate_balanced2(_m))
    if ANG_GENERIC_M[_key] is None:
        ANG_GENERIC_M[_key] = _m
