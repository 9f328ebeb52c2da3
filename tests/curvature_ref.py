"""The yardstick of the curvature rows (obtg_curvature_poly, obtg_curvature_true_min[_jac], obtg_bern_curvature) in EXACT
rationals, with mpmath for the one irrational step (a square root).  No device, no reference code, and not a re-run of the
device's search: the search here has its own arithmetic (integers), its own bound constants and its own bracket.

For one planar curve with control points x_i, y_i (i <= n), derivatives with respect to the parameter (T = 1; curvature does
not depend on the time span):

    den(t) = x'^2 + y'^2,    num(t) = y'' x' - x'' y',    kappa(t) = num / den^(3/2)      (left turns positive)
    side 0 (sigma = +1), side 1 (sigma = -1):  m_sigma = max_t max(0, sigma kappa(t)),   row_sigma = max_curv - m_sigma

With w = B^(n-1)(t), u = B^(n-2)(t), entries out of range 0, A_i = n (w_(i-1) - w_i), C_i = n (n-1) (u_(i-2) - 2 u_(i-1) + u_i):

    d row_sigma / d x_i = -sigma [ (y'' A_i - y' C_i) / den^(3/2) - 3 num x' A_i / den^(5/2) ]
    d row_sigma / d y_i = -sigma [ (x' C_i - x'' A_i) / den^(3/2) - 3 num y' A_i / den^(5/2) ]

A float64 is a dyadic rational: control points and parameters are taken as Fractions; den_k, num_k, kappa^2 and every factor of
the block that is rational are exact, den^(1/2) is mpmath's at 50 digits.

ROUNDING MAJORANTS (unit UNIT = 2^-53; every count is derived below from the operations csrc/bern_device.h and
csrc/extrema_kernels.hip state, one rounding = one unit on the magnitude it rounds; the counts carry +1 for second-order terms):

  coefficients (coeff_count): x1 = diff_elev1_at: subtraction, times n, the weight c/n, its product, the fma: 5 on
    m1_c = n [(c/n)(|p_c| + |p_(c-1)|) + ((n-c)/n)(|p_(c+1)| + |p_c|)];  x2 the same from x1: 5 inherited + 5 = 10 on m2;
    u = C(n, j) x (C exact for n <= 31): +1, so 6 and 11;  a product u2 u1: 17 (den: u1 u1: 12);  the fma chain of at most
    2 (n + 1) terms: one each;  s_k = 1 / C(2n, k): the binomial from an 80-bit product rounded to binary64, the reciprocal,
    the product: 4.  Together 17 + 2 (n + 1) + 4 + 1 = 2 n + 24 on mnum_k / mden_k, the same sums on magnitudes.
  a bisection point at depth d (point_count): every bisection is 2 n levels of averages 0.5 a + 0.5 b, one rounding each on
    a convex combination of magnitudes, so 2 n d on MN(t) = sum_k B_k(t) mnum_k (MD likewise): K_pt = 2 n + 24 + 2 n d.
  sigma kappa(t) (kappa_majorant): with EN = K_pt UNIT MN, ED = K_pt UNIT MD and ED <= den / 4, the mean value theorem on
    d^(-3/2) over [0.75 den, 1.25 den] gives |N' D'^(-3/2) - N D^(-3/2)| <= 1.54 EN / den^(3/2) + 3.08 |num| ED / den^(5/2);
    the square root (2 units granted), the product, the quotient and second order: 5 on |kappa|.  So
        |device - exact| <= (K_pt + 5) UNIT M,   M = 1.54 MN / den^(3/2) + 3.08 |num| MD / den^(5/2) + |kappa|,
    and the row max_curv - m_sigma is one more rounding on max_curv + |kappa|.
  a block entry (block_majorant): the basis from n - 1 steps of s = 1 - t (once), a product and an fma: Kb = 3 n on a sum
    of non-negative terms;  x' : a difference, n fmas, the scale: K1 = Kb + n + 2 = 4 n + 2 on mx' = n sum w_i (|P_(i+1)| + |P_i|);
    x'': two levels of differences, n - 1 fmas, the scale: K2 = 4 n + 3 on mx'' = n (n-1) sum u_i (|P_(i+2)| + 2 |P_(i+1)| + |P_i|);
    A_i: Kb + 2 on mA_i = n (w_(i-1) + w_i);  C_i: Kb + 3 on mC_i;  den: 2 K1 + 2 on mden = mx'^2 + my'^2, rho = mden / den;
    num: K1 + K2 + 2 on mnum = my'' mx' + mx'' my';  G = y'' A - y' C: K2 + Kb + 4 = 7 n + 7 on mG = my'' mA + my' mC;
    r = 1 / (den sqrt(den)): 1.5 (2 K1 + 2) rho + 4 <= (3 K1 + 7) rho relative;  q = 3 num / (den (den sqrt(den))):
    (K1 + K2 + 4) on 3 mnum / den^(5/2) and (5 K1 + 10) rho relative;  (q x') A: K1 + Kb + 4 more on |q| mx' mA;  the outer
    fma: 1 on the entry.  The largest count is 5 K1 + 10 + 1 = 20 n + 21 = K_blk, and
        M_blk = (mG + rho |G|) / den^(3/2) + 3 mnum mx' mA / den^(5/2) + 2 rho |q| mx' mA + |entry|,
    valid to first order; 1.05 covers the second while K_blk UNIT rho <= 1e-3 (else the function answers inf: no bound)."""
import math
from fractions import Fraction

import mpmath
import numpy as np

mpmath.mp.dps = 50
UNIT = Fraction(1, 2 ** 53)
SIGMA = (1, -1)          # side -> sigma
_P = 64                  # extra bits of the rational square roots


def _F(x):
    return Fraction(float(x))


def _ctrl(yv):
    """the control points as [2][n + 1] Fractions: a float64 array, or rows of Fractions handed through as they are"""
    if isinstance(yv, (list, tuple)) and isinstance(yv[0][0], Fraction):
        return [list(r) for r in yv]
    return [[_F(v) for v in row] for row in np.asarray(yv, dtype=np.float64)]


def _binom(n, k):
    return math.comb(n, k) if 0 <= k <= n else 0


def basis(n, t):
    """[B_0^n(t) .. B_n^n(t)] as Fractions (n < 0: empty)"""
    if n < 0:
        return []
    t = Fraction(t)
    return [_binom(n, i) * t ** i * (1 - t) ** (n - i) for i in range(n + 1)]


# ------------------------------------------------------------------------------------------------ coefficients
def _diff_elev1(p, mags):
    """Bezier.diff() on T = 1 (derivative, then elev(1): degree n again) of the Fractions p, and the same sum on magnitudes"""
    n = len(p) - 1
    out, mag = [], []
    for c in range(n + 1):
        tl = n * (p[c] - p[c - 1]) if c > 0 else 0
        tr = n * (p[c + 1] - p[c]) if c < n else 0
        ml = n * (mags[c] + mags[c - 1]) if c > 0 else 0
        mr = n * (mags[c + 1] + mags[c]) if c < n else 0
        out.append(Fraction(c, n) * tl + Fraction(n - c, n) * tr)
        mag.append(Fraction(c, n) * ml + Fraction(n - c, n) * mr)
    return out, mag


def coeffs(yv):
    """(num[2n+1], den[2n+1], mnum, mden): the exact Bernstein coefficients of num and den of the curve yv[2][n+1], and the
    same sums on magnitudes"""
    P = _ctrl(yv)
    n = len(P[0]) - 1
    d1, m1, d2, m2 = [], [], [], []
    for c in range(2):
        a, ma = _diff_elev1(P[c], [abs(v) for v in P[c]])
        b, mb = _diff_elev1(a, ma)
        d1.append(a); m1.append(ma); d2.append(b); m2.append(mb)
    num, den, mnum, mden = [], [], [], []
    for k in range(2 * n + 1):
        sn = sd = smn = smd = Fraction(0)
        for j in range(max(0, k - n), min(n, k) + 1):
            w = Fraction(_binom(n, j) * _binom(n, k - j), _binom(2 * n, k))
            sd += w * (d1[0][j] * d1[0][k - j] + d1[1][j] * d1[1][k - j])
            sn += w * (d2[1][j] * d1[0][k - j] - d2[0][j] * d1[1][k - j])
            smd += w * (m1[0][j] * m1[0][k - j] + m1[1][j] * m1[1][k - j])
            smn += w * (m2[1][j] * m1[0][k - j] + m2[0][j] * m1[1][k - j])
        num.append(sn); den.append(sd); mnum.append(smn); mden.append(smd)
    return num, den, mnum, mden


def coeff_count(n):
    return 2 * n + 24


def point_count(n, depth):
    return coeff_count(n) + 2 * n * depth


def depth_of(t):
    """the bisection depth of a dyadic t in [0, 1]: 0 for an end, else the exponent of its denominator"""
    return Fraction(float(t)).denominator.bit_length() - 1


def _bern(co, t):
    m = len(co) - 1
    return sum(b * c for b, c in zip(basis(m, t), co))


# ------------------------------------------------------------------------------------------------ a point
def derivatives(yv, t):
    """(x', y', x'', y'', w, u, P) at t, exact"""
    P = _ctrl(yv)
    n = len(P[0]) - 1
    t = Fraction(t)
    w, u = basis(n - 1, t), basis(n - 2, t)
    d1 = [n * sum(w[i] * (P[c][i + 1] - P[c][i]) for i in range(n)) for c in range(2)]
    d2 = [n * (n - 1) * sum(u[i] * (P[c][i + 2] - 2 * P[c][i + 1] + P[c][i]) for i in range(n - 1)) for c in range(2)]
    return d1[0], d1[1], d2[0], d2[1], w, u, P


def num_den(yv, t):
    xd, yd, xdd, ydd = derivatives(yv, t)[:4]
    return ydd * xd - xdd * yd, xd * xd + yd * yd


def kappa2(yv, t):
    """(sign of kappa, kappa^2) at t, exact; the speed must not vanish there"""
    num, den = num_den(yv, t)
    return (num > 0) - (num < 0), num * num / den ** 3


def _mp(f):
    return mpmath.mpf(f.numerator) / mpmath.mpf(f.denominator)


def kappa(yv, t):
    """kappa(t) as an mpf: the exact num and den, one 50-digit square root"""
    num, den = num_den(yv, t)
    d = _mp(den)
    return _mp(num) / (d * mpmath.sqrt(d))


def kappa_majorant(yv, t, co=None):
    """(K, M): |the device's sigma kappa(t) - the exact one| <= K UNIT M for the bisection point t (module docstring); M is
    inf where ED <= den / 4 does not hold"""
    num, den, mnum, mden = co or coeffs(yv)
    n = (len(num) - 1) // 2
    t = _F(t)
    K = point_count(n, depth_of(t))
    N, D, MN, MD = _bern(num, t), _bern(den, t), _bern(mnum, t), _bern(mden, t)
    if D <= 0 or K * UNIT * MD > D / 4:
        return K + 5, mpmath.inf
    d = _mp(D)
    d32 = d * mpmath.sqrt(d)
    return K + 5, (mpmath.mpf("1.54") * _mp(MN) + mpmath.mpf("3.08") * _mp(abs(N)) * _mp(MD) / d) / d32 + abs(_mp(N)) / d32


def sample_values(yv, points=4097, co=None):
    """[(num, den)] at the sample points i / (points - 1), as integers on one common positive scale S: [(rn, rd)], S.
    Integer arithmetic on a common denominator (a Horner scheme in i and points - 1 - i)."""
    num, den = (co or coeffs(yv))[:2]
    m = len(num) - 1
    q = 1
    for f in num + den:
        q = q * f.denominator // math.gcd(q, f.denominator)
    an = [int(f * q) * _binom(m, k) for k, f in enumerate(num)]
    ad = [int(f * q) * _binom(m, k) for k, f in enumerate(den)]
    g = points - 1
    out = []
    for i in range(points):
        j = g - i
        rn, rd, pw = an[m], ad[m], 1
        for k in range(m - 1, -1, -1):
            pw *= j
            rn = rn * i + an[k] * pw
            rd = rd * i + ad[k] * pw
        out.append((rn, rd))
    return out, q * g ** m


def sample_exceeds(yv, side, level, points=4097, co=None, values=None):
    """the sample points i / (points - 1) at which sigma kappa > level (a Fraction >= 0), decided in rationals:
    sigma num > 0 and num^2 > level^2 den^3"""
    vals, s = values or sample_values(yv, points, co)
    lvl2 = Fraction(level) ** 2
    a, b = lvl2.numerator, lvl2.denominator
    # (rn / s)^2 > (a / b) (rd / s)^3  <=>  rn^2 b s > a rd^3   (s, b > 0)
    return [i for i, (rn, rd) in enumerate(vals) if rn * SIGMA[side] > 0 and rn * rn * b * s > a * rd ** 3]


# ------------------------------------------------------------------------------------------------ the certified search
def _isqrt_frac(f, up):
    """a rational below (up: above) sqrt(f), f > 0, within 2^-_P relative"""
    f = Fraction(f)
    shift = max(0, 2 * _P + f.denominator.bit_length() - f.numerator.bit_length())
    shift += shift & 1
    r = math.isqrt((f.numerator << shift) // f.denominator)
    return Fraction(r + (1 if up else 0), 1 << (shift // 2))


def _kappa_bounds(N, D, R):
    """rationals (lo, hi) around N R / D^(3/2), D > 0"""
    a, b = Fraction(N * R) / (D * _isqrt_frac(D, True)), Fraction(N * R) / (D * _isqrt_frac(D, False))
    return (a, b) if N >= 0 else (b, a)


def _node_bound(Ns, Ds, R, clamp):
    """an upper bound of N(t) R / D(t)^(3/2) over a sub-curve with integer coefficients Ns, Ds.  With some N_k > 0: the
    tangent of d^(3/2) at s^2, s a rational at or below the square root of the SMALLEST D_k -- g(d) = s (1.5 d - 0.5 s^2) is
    that tangent exactly, whatever s is, so D(t)^(3/2) >= sum g_k B_k(t), and every g_k >= g(s^2) = s^3 > 0 because every
    D_k >= s^2.  lambda = the largest N_k R / g_k over ALL k then has lambda g_k - N_k R >= 0 for every coefficient (checked
    below, coefficient by coefficient) and lambda > 0, hence N(t) R <= lambda sum g_k B_k(t) <= lambda D(t)^(3/2).  (Not
    the device's tangent point -- the mid-range, which is sound only while it stays positive at the smallest D_k -- and
    never infinite while the speed does not vanish on the hull.)  With no N_k > 0: 0 (clamp), else the chord through two
    points above the curve.  None: +inf."""
    dmin, dmax = min(Ds), max(Ds)
    if any(v > 0 for v in Ns):
        if dmin <= 0:
            return None
        s = _isqrt_frac(dmin, False)
        gs = [s * (Fraction(3, 2) * Dk - s * s / 2) for Dk in Ds]
        assert all(g >= s ** 3 > 0 for g in gs)
        lam = max(Nk * R / g for Nk, g in zip(Ns, gs))
        assert lam > 0 and all(lam * g - Nk * R >= 0 for Nk, g in zip(Ns, gs))
        return lam
    if clamp or dmin <= 0:
        return Fraction(0)
    A, B = dmin * _isqrt_frac(dmin, True), dmax * _isqrt_frac(dmax, True)
    best = None
    for Nk, Dk in zip(Ns, Ds):
        h = A if dmax == dmin else A + (B - A) * Fraction(Dk - dmin, dmax - dmin)
        lam = Nk * R / h
        best = lam if best is None or lam > best else best
    return best


def _split(c):
    """integer de Casteljau at 1/2 without a division: (left, right), both scaled by 2^(len - 1)"""
    m = len(c) - 1
    row, left, right = list(c), [c[0] << m], [0] * (m + 1)
    right[m] = c[m] << m
    for r in range(1, m + 1):
        row = [row[i] + row[i + 1] for i in range(m + 1 - r)]
        left.append(row[0] << (m - r))
        right[m - r] = row[-1] << (m - r)
    return left, right


def certified_max(yv, side, max_curv, rel=Fraction(1, 10 ** 9), max_nodes=100000, clamp=True, stack=32, co=None):
    """dict(L, H, t, nodes, waiting, status): L <= m_sigma <= H, L a rational at or below a value met at t (or the clamp's 0),
    H - L <= rel max(max_curv, |L|) with status 'ok'; 'node_cap' / 'depth_cap' as the device names them (more than `stack`
    sub-curves waiting); waiting: the most that waited at once.  Depth-first, the half with the larger bound first."""
    num, den = (co or coeffs(yv))[:2]
    m = len(num) - 1
    q = 1
    for f in num + den:
        q = q * f.denominator // math.gcd(q, f.denominator)
    # num_k = Ns_k / q^2, den_k = Ds_k / q^2: kappa = N R / D^(3/2) with R = q; a split scales by 2^m, m even: R by 2^(m/2)
    Ns = [int(f * q * q) * SIGMA[side] for f in num]
    Ds = [int(f * q * q) for f in den]
    rel, W = Fraction(rel), _F(max_curv)
    out = dict(nodes=1, waiting=0, status='ok')
    if not any(Ns):
        out.update(L=Fraction(0), H=Fraction(0), t=Fraction(0))
        return out
    L, tL = (Fraction(0), Fraction(0)) if clamp else (None, Fraction(0))

    def meet(N, D, R, t):
        nonlocal L, tL
        if D > 0:
            lo = _kappa_bounds(N, D, R)[0]
            if L is None or lo > L:
                L, tL = lo, t
    meet(Ns[0], Ds[0], q, Fraction(0))
    meet(Ns[m], Ds[m], q, Fraction(1))

    def open_(ub):
        return ub is None or L is None or ub - L > rel * max(W, abs(L))
    H = None          # the largest bound of a closed sub-curve
    ub = _node_bound(Ns, Ds, q, clamp)
    todo = []
    cur = (Ns, Ds, q, Fraction(0), Fraction(1), ub) if open_(ub) else None
    if cur is None:
        H = ub
    while cur is not None:
        if out['nodes'] + 2 > max_nodes:
            out['status'] = 'node_cap'
            break
        Nc, Dc, R, t0, w, _ = cur
        (nl, nr), (dl, dr) = _split(Nc), _split(Dc)
        R2, hw = R << (m // 2), w / 2
        out['nodes'] += 2
        meet(nl[m], dl[m], R2, t0 + hw)
        kids = []
        for Nk, Dk, ta in ((nl, dl, t0), (nr, dr, t0 + hw)):
            b = _node_bound(Nk, Dk, R2, clamp)
            if open_(b):
                kids.append((Nk, Dk, R2, ta, hw, b))
            else:
                H = b if H is None or b > H else H
        if len(kids) == 2:
            if len(todo) == stack:
                out['status'] = 'depth_cap'
                break
            first = 0 if (kids[0][5] is None or (kids[1][5] is not None and kids[0][5] >= kids[1][5])) else 1
            todo.append(kids[1 - first])
            out['waiting'] = max(out['waiting'], len(todo))
            cur = kids[first]
        elif kids:
            cur = kids[0]
        else:
            cur = None
            while todo:
                cand = todo.pop()
                if open_(cand[5]):
                    cur = cand
                    break
                H = cand[5] if H is None or cand[5] > H else H
    if L is None:
        L = Fraction(0)
    if out['status'] != 'ok':
        H = None
    else:
        H = L if H is None or H < L else H
    out.update(L=L, H=H, t=tL)
    return out


def curvature_range(yv, rel=Fraction(1, 10 ** 12)):
    """(k_min bracket, k_max bracket) of a free curve, each (lo, hi) Fractions: k_max = m_+ and k_min = -m_- without the clamp"""
    hi = certified_max(yv, 0, 0.0, rel, clamp=False)
    lo = certified_max(yv, 1, 0.0, rel, clamp=False)
    return (-lo['H'], -lo['L']), (hi['L'], hi['H'])


# ------------------------------------------------------------------------------------------------ the envelope block
def _parts(yv, t):
    xd, yd, xdd, ydd, w, u, P = derivatives(yv, t)
    n = len(P[0]) - 1

    def at(b, i):
        return b[i] if 0 <= i < len(b) else Fraction(0)
    A = [n * (at(w, i - 1) - at(w, i)) for i in range(n + 1)]
    Cc = [n * (n - 1) * (at(u, i - 2) - 2 * at(u, i - 1) + at(u, i)) for i in range(n + 1)]
    mA = [n * (at(w, i - 1) + at(w, i)) for i in range(n + 1)]
    mC = [n * (n - 1) * (at(u, i - 2) + 2 * at(u, i - 1) + at(u, i)) for i in range(n + 1)]
    m1 = [n * sum(w[i] * (abs(P[c][i + 1]) + abs(P[c][i])) for i in range(n)) for c in range(2)]
    m2 = [n * (n - 1) * sum(u[i] * (abs(P[c][i + 2]) + 2 * abs(P[c][i + 1]) + abs(P[c][i])) for i in range(n - 1)) for c in range(2)]
    return n, xd, yd, xdd, ydd, A, Cc, mA, mC, m1, m2


def envelope_block(yv, side, t):
    """[2][n + 1] mpf: d row_sigma / d (x_i, y_i) at t (the row is not clamped there and the speed does not vanish)"""
    n, xd, yd, xdd, ydd, A, Cc = _parts(yv, t)[:7]
    den, num = xd * xd + yd * yd, ydd * xd - xdd * yd
    d = _mp(den)
    d32 = d * mpmath.sqrt(d)
    d52 = d * d32
    sg = SIGMA[side]
    bx = [-sg * (_mp(ydd * A[i] - yd * Cc[i]) / d32 - _mp(3 * num * xd * A[i]) / d52) for i in range(n + 1)]
    by = [-sg * (_mp(xd * Cc[i] - xdd * A[i]) / d32 - _mp(3 * num * yd * A[i]) / d52) for i in range(n + 1)]
    return [bx, by]


def block_majorant(yv, t):
    """(K_blk, M_blk[2][n + 1] mpf): |device entry - exact entry| <= 1.05 K_blk UNIT M_blk (module docstring); inf where
    K_blk UNIT rho > 1e-3"""
    n, xd, yd, xdd, ydd, A, Cc, mA, mC, m1, m2 = _parts(yv, t)
    K = 20 * n + 21
    den, num = xd * xd + yd * yd, ydd * xd - xdd * yd
    mden, mnum = m1[0] ** 2 + m1[1] ** 2, m2[1] * m1[0] + m2[0] * m1[1]
    if den <= 0 or K * UNIT * mden > den / 1000:
        return K, [[mpmath.inf] * (n + 1) for _ in range(2)]
    rho = _mp(mden / den)
    d = _mp(den)
    d32 = d * mpmath.sqrt(d)
    d52 = d * d32
    q = abs(_mp(3 * num)) / d52
    out = []
    for c, (G, mG) in enumerate((([ydd * A[i] - yd * Cc[i] for i in range(n + 1)], [m2[1] * mA[i] + m1[1] * mC[i] for i in range(n + 1)]),
                                 ([xd * Cc[i] - xdd * A[i] for i in range(n + 1)], [m1[0] * mC[i] + m2[0] * mA[i] for i in range(n + 1)]))):
        d1 = (xd, yd)[c]
        row = []
        for i in range(n + 1):
            entry = abs(_mp(G[i]) / d32 - _mp(3 * num * d1 * A[i]) / d52)
            row.append((_mp(mG[i]) + rho * abs(_mp(G[i]))) / d32 + 3 * _mp(mnum * m1[c] * mA[i]) / d52
                       + 2 * rho * q * _mp(m1[c] * mA[i]) + entry)
        out.append(row)
    return K, out


# ------------------------------------------------------------------------------------------------ inputs
def seeded(deg, seed):
    """the seeded family: a straight line from (0, 0) to (10, 3), N(0, 0.6) noise on every control point: [2][deg + 1]"""
    rs = np.random.RandomState(seed)
    line = np.stack((np.linspace(0.0, 10.0, deg + 1), np.linspace(0.0, 3.0, deg + 1)))
    return line + 0.6 * rs.randn(2, deg + 1)


PARABOLA = np.array([[-1.0, 0.0, 1.0], [1.0, -1.0, 1.0]])       # max kappa = 2 at t = 1/2, min kappa = 2 / 5^(3/2) at the ends


# A near-stop curve of degree 4: den varies by far more than 5x over [0, 1], and next to t = 0 the coefficients with num_k <= 0
# sit where a tangent of den^(3/2) taken at the mid-range of den is negative.  A bound that looks at the num_k > 0 alone closes
# the node there and reports max(-kappa) = 0.02801 (the value at t = 1); the maximum is 0.034917 near t = 0.0462.
WIDE_SPEED = np.array([[-1.4017902549024934, -1.4000319327142283, -0.8572610010430977, -1.026490504733748, -0.656324904069945],
                       [0.12124707553835466, 0.1113181198446885, -2.3781886614141667, -2.472181568890013, -0.5102682489527195]])


def wild(deg, seed):
    """control points N(0, 1) with no line under them: the speed varies by orders of magnitude along such a curve"""
    return np.random.RandomState(1000 + seed).randn(2, deg + 1)


def elevated(yv, deg):
    """yv degree-elevated to deg, in float64 (the result is the input of whoever uses it: its own curve)"""
    yv = np.asarray(yv, dtype=np.float64)
    while yv.shape[1] - 1 < deg:
        n = yv.shape[1] - 1
        i = np.arange(1, n + 1)
        up = np.empty((2, n + 2))
        up[:, 0], up[:, -1] = yv[:, 0], yv[:, -1]
        up[:, 1:-1] = (i / (n + 1.0)) * yv[:, :-1] + (1.0 - i / (n + 1.0)) * yv[:, 1:]
        yv = up
    return yv


def regular_curves(deg, count, eps_rel, max_nodes, max_curv=1.0):
    """`count` seeded curves of degree deg, seeds in order from 0, on which this file's search ends for both sides with at
    most 32 waiting and within max_nodes -- decided here, before any device sees them -- then the parabola (deg >= 2)"""
    out, seed = [], 0
    while len(out) < count:
        yv = seeded(deg, seed)
        seed += 1
        co = coeffs(yv)
        if all(certified_max(yv, s, max_curv, Fraction(eps_rel), max_nodes, co=co)['status'] == 'ok' for s in range(2)):
            out.append(yv)
    if deg >= 2:
        out.append(elevated(PARABOLA, deg))
    return out
