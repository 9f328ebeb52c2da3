"""The yardstick of the space-curvature rows (obtg_space_curvature_poly, obtg_space_curvature_true_min[_jac],
obtg_bern_space_curvature) in EXACT rationals, with mpmath for the irrational steps (square roots).  No device, no reference
code, and not a re-run of the device's search: the search here has its own arithmetic (integers), its own tangent point, its
own upper bounds of the norms and its own bracket.  It borrows curvature_ref.py's helpers (basis, integer split, rational
square roots) and nothing of its search.

For one curve in space with control points P[c][i] (c < 3, i <= n), derivatives with respect to the parameter (T = 1):

    w(t) = c' x c'' (three polynomials),   den(t) = |c'|^2,   kappa(t) = |w| / den^(3/2) >= 0
    m = max_t kappa(t),    row = max_curv - m            (one row per vehicle: no sides, no clamp)

With A_i, C_i curvature_ref.py's, v = c'(t), a = c''(t), wh = w / |w|:

    d row / d P[d][i] = -[ (A_i (a x wh)_d + C_i (wh x v)_d) / den^(3/2) - 3 |w| v_d A_i / den^(5/2) ]
                      = -[ G_di / (|w| den^(3/2)) - |w| H_di / den^(5/2) ],   G_di = A_i (a x w)_d + C_i (w x v)_d,  H_di = 3 v_d A_i,

G, H, |w|^2 and den exact rationals (block_parts); d kappa^2 / d P[d][i] = 2 (G / den^3 - |w|^2 H / den^4) is rational.

THE CERTIFIED SEARCH (certified_max).  On one common scale the coefficients are integers W_k (three) and D_k.  A node's
bound: s a rational at or BELOW the square root of the smallest D_k, g(d) = s (1.5 d - 0.5 s^2) the tangent of d^(3/2) at
s^2 exactly, so D(t)^(3/2) >= sum g_k B_k(t) with every g_k >= s^3 > 0; NU_k a rational at or ABOVE |W_k|; the norm is
convex, so |W(t)| <= sum NU_k B_k(t); lambda = max NU_k R / g_k, and lambda g_k - NU_k R >= 0 is checked coefficient by
coefficient.  Not the device's tangent point (the mid-range), not its norms (rounded to nearest).

ROUNDING MAJORANTS (unit UNIT = 2^-53; derived from the operations csrc/bern_device.h and csrc/extrema_kernels.hip state and
include/obtg.h repeats, one rounding = one unit on the magnitude it rounds; the counts carry +1 for second-order terms):

  coefficients (coeff_count): a component of w is curvature_row_coeff's num on a pair of coordinates: curvature_ref.py's
    count, 17 for a product u2 u1 + 2 (n + 1) for the chain + 4 for s_k + 1 = 2 n + 24 on mw_k;  den: 12 for a product u1 u1,
    a chain of at most 3 (n + 1) terms, 4, 1: 3 n + 20 on mden_k.  One count serves all four: K_c = 3 n + 24.
  a bisection point at depth d (point_count): 2 n levels of averages per bisection, one rounding each on a convex combination
    of magnitudes: K_pt = 3 n + 24 + 2 n d on MW_c(t) = sum_k B_k(t) mw_c,k and MD(t).
  kappa(t) (kappa_majorant): the components arrive within K_pt UNIT MW_c, so by the triangle inequality |w| moves by at most
    K_pt UNIT |MW| (|MW| the norm of the three magnitudes); the sum of squares is a product and two fmas on non-negative
    partial sums (3 units on the sum: 1.5 on its root) and the root 1: 3 on |w|.  The denominator as in curvature_ref.py
    (ED = K_pt UNIT MD <= den / 4; the mean value theorem on d^(-3/2) over [0.75 den, 1.25 den]; root, product, quotient
    and second order: 5).  So
        |device - exact| <= (K_pt + 8) UNIT M,   M = 1.54 |MW| / den^(3/2) + 3.08 |w| MD / den^(5/2) + kappa,
    and the row max_curv - m is one more rounding on max_curv + kappa.
  the bound of a closed node (bound_majorant): the device closes a node on lambda' = max nu'_k / g'_k computed from rounded
    coefficients.  nu'_k is within (K_pt + 3) units of |MW_k|-magnitudes as above; g'_k: a sum, a root, two products for a,
    three for c, the fma: 8 units on 1.5 sqrt(d0) den_k + 0.5 d0 sqrt(d0) <= 2 dmax^(3/2) (the guard keeps dmax < 5 dmin), and
    the quotient 1.  A node that closes has lambda' <= U + tol, so g'_k >= nu'_k / (U + tol): the absolute error of g'_k
    moves lambda' by at most lambda' (that error) / g'_k.  The test takes R_bound as the largest point majorant over a grid of
    [0, 1] at the depth of t_star with K_pt + 8 + 9 units: the same magnitudes, the bound's own operations counted in.
  a block entry (block_majorant): curvature_ref.py's basis and derivative counts, Kb = 3 n, K1 = 4 n + 2 on mv_c,
    K2 = 4 n + 3 on ma_c, A_i: Kb + 2, C_i: Kb + 3;  a component of w: a product and an fma of two products:
    K1 + K2 + 2 on mw_c = mv_a ma_b + mv_b ma_a;  den: 2 K1 + 3 on mden = sum mv_c^2, rho = mden / den;  |w|: K1 + K2 + 5
    relative to sigma = |mw| / |w|;  wh_c = w_c / |w|: Kh = 2 (K1 + K2) + 8 = 16 n + 18 on sigma (|wh_c| <= 1);  P = a x wh:
    K2 + Kh + 2 on mP_d = sigma (ma_b + ma_c), Q = wh x v: K1 + Kh + 2 on mQ_d = sigma (mv_b + mv_c);  G' = fma(P, A, Q C):
    K2 + Kh + Kb + 7 = 23 n + 28 on mG = mP mA + mQ mC;  r = 1 / (den sqrt(den)): 1.5 (2 K1 + 3) rho + 4 <= (3 K1 + 9) rho
    relative;  q = 3 |w| / (den (den sqrt(den))): K1 + K2 + 7 relative to sigma and (5 K1 + 12) rho relative;  (q v_d) A:
    K1 + Kb + 4 more on |q| mv mA;  the outer fma 1.  The counts are ADDED, not the largest taken:
        K_blk = (23 n + 28) + (20 n + 22) = 43 n + 50,
        M_blk = (mG + rho |G'|) / den^(3/2) + 3 |mw| mv_d mA_i / den^(5/2) + 2 rho |q| mv_d mA_i + |entry|,
    valid to first order; 1.05 covers the second while K_blk UNIT rho sigma <= 1e-3 (else the function answers inf)."""
import math
from fractions import Fraction

import mpmath
import numpy as np

import curvature_ref as C
from curvature_ref import UNIT, _F, _binom, _bern, _mp, _isqrt_frac, _split, basis, depth_of  # noqa: F401

mpmath.mp.dps = 50
PAIRS = ((1, 2), (2, 0), (0, 1))          # component c of w = v x a is v_a a_b - v_b a_a on the pair (a, b)
# an exact rational rotation (rows orthonormal, determinant 1) and a translation: a planar curve lifted into space
ROTATION = [[Fraction(2, 3), Fraction(-1, 3), Fraction(2, 3)],
            [Fraction(2, 3), Fraction(2, 3), Fraction(-1, 3)],
            [Fraction(-1, 3), Fraction(2, 3), Fraction(2, 3)]]
TRANSLATION = [Fraction(1, 2), Fraction(-3, 4), Fraction(2)]


def _ctrl(yv):
    """the control points as [3][n + 1] Fractions: a float64 array, or rows of Fractions handed through as they are"""
    if isinstance(yv, (list, tuple)) and isinstance(yv[0][0], Fraction):
        return [list(r) for r in yv]
    return [[_F(v) for v in row] for row in np.asarray(yv, dtype=np.float64)]


def lift(planar):
    """the planar curve [2][n + 1] (floats or Fractions) rotated by ROTATION and moved by TRANSLATION: [3][n + 1] Fractions, exact"""
    P = C._ctrl(planar)
    return [[ROTATION[r][0] * x + ROTATION[r][1] * y + TRANSLATION[r] for x, y in zip(P[0], P[1])] for r in range(3)]


def snap3(planar, bits=30):
    """the planar float64 curve with every coordinate rounded to a multiple of 3 / 2^bits: its lift is exact in binary64"""
    a = np.asarray(planar, dtype=np.float64)
    return np.round(a * (2.0 ** bits / 3.0)) * (3.0 / 2.0 ** bits)


def as_floats(rows):
    """Fractions that are binary64 numbers, as a float64 array (asserted exact)"""
    out = np.array([[float(v) for v in r] for r in rows])
    assert all(Fraction(float(v)) == v for r in rows for v in r), "not exact in binary64"
    return out


# ------------------------------------------------------------------------------------------------ coefficients
def coeffs(yv):
    """(w[3][2n+1], den[2n+1], mw[3][2n+1], mden[2n+1]): the exact Bernstein coefficients of the components of w = c' x c'' and
    of den = |c'|^2 of the curve yv[3][n+1], and the same sums on magnitudes"""
    P = _ctrl(yv)
    n = len(P[0]) - 1
    d1, m1, d2, m2 = [], [], [], []
    for c in range(3):
        a, ma = C._diff_elev1(P[c], [abs(v) for v in P[c]])
        b, mb = C._diff_elev1(a, ma)
        d1.append(a); m1.append(ma); d2.append(b); m2.append(mb)
    w, mw, den, mden = [[], [], []], [[], [], []], [], []
    for k in range(2 * n + 1):
        sw, smw, sd, smd = [Fraction(0)] * 3, [Fraction(0)] * 3, Fraction(0), Fraction(0)
        for j in range(max(0, k - n), min(n, k) + 1):
            wt = Fraction(_binom(n, j) * _binom(n, k - j), _binom(2 * n, k))
            for c, (a, b) in enumerate(PAIRS):
                sw[c] += wt * (d2[b][j] * d1[a][k - j] - d2[a][j] * d1[b][k - j])
                smw[c] += wt * (m2[b][j] * m1[a][k - j] + m2[a][j] * m1[b][k - j])
            sd += wt * sum(d1[c][j] * d1[c][k - j] for c in range(3))
            smd += wt * sum(m1[c][j] * m1[c][k - j] for c in range(3))
        for c in range(3):
            w[c].append(sw[c]); mw[c].append(smw[c])
        den.append(sd); mden.append(smd)
    return w, den, mw, mden


def coeff_count(n):
    return 3 * n + 24


def point_count(n, depth):
    return coeff_count(n) + 2 * n * depth


# ------------------------------------------------------------------------------------------------ a point
def derivatives(yv, t):
    """(v[3], a[3], w_basis, u_basis, P) at t, exact"""
    P = _ctrl(yv)
    n = len(P[0]) - 1
    t = Fraction(t)
    w, u = basis(n - 1, t), basis(n - 2, t)
    d1 = [n * sum(w[i] * (P[c][i + 1] - P[c][i]) for i in range(n)) for c in range(3)]
    d2 = [n * (n - 1) * sum(u[i] * (P[c][i + 2] - 2 * P[c][i + 1] + P[c][i]) for i in range(n - 1)) for c in range(3)]
    return d1, d2, w, u, P


def cross(p, q):
    return [p[a] * q[b] - p[b] * q[a] for a, b in PAIRS]


def w2_den(yv, t):
    """(|w|^2, den) at t, exact"""
    v, a = derivatives(yv, t)[:2]
    w = cross(v, a)
    return sum(x * x for x in w), sum(x * x for x in v)


def kappa2(yv, t):
    """kappa^2 at t, exact; the speed must not vanish there"""
    w2, den = w2_den(yv, t)
    return w2 / den ** 3


def kappa(yv, t):
    """kappa(t) as an mpf"""
    return mpmath.sqrt(_mp(kappa2(yv, t)))


def kappa_majorant(yv, t, co=None, extra=8):
    """(K, M): |the device's kappa(t) - the exact one| <= K UNIT M for the bisection point t (module docstring); M is inf
    where ED <= den / 4 does not hold"""
    w, den, mw, mden = co or coeffs(yv)
    n = (len(den) - 1) // 2
    t = _F(t)
    K = point_count(n, depth_of(t))
    D, MD = _bern(den, t), _bern(mden, t)
    if D <= 0 or K * UNIT * MD > D / 4:
        return K + extra, mpmath.inf
    W2 = sum(_bern(w[c], t) ** 2 for c in range(3))
    MW = mpmath.sqrt(_mp(sum(_bern(mw[c], t) ** 2 for c in range(3))))
    nw = mpmath.sqrt(_mp(W2))
    d = _mp(D)
    d32 = d * mpmath.sqrt(d)
    return K + extra, (mpmath.mpf("1.54") * MW + mpmath.mpf("3.08") * nw * _mp(MD) / d) / d32 + nw / d32


def bound_majorant(yv, depth, co=None, points=33):
    """R_bound / UNIT-free: the largest (K + 17) UNIT M over the grid i / (points - 1) with the counts of a point at `depth`
    (module docstring, 'the bound of a closed node'); an mpf"""
    co = co or coeffs(yv)
    n = (len(co[1]) - 1) // 2
    K = point_count(n, depth) + 17
    worst = mpmath.mpf(0)
    for i in range(points):
        M = kappa_majorant(yv, Fraction(i, points - 1), co)[1]
        worst = max(worst, M)
    return K * _mp(UNIT) * worst


def sample_max2(yv, points=1025):
    """the largest kappa^2 over the sample points i / (points - 1), exact, and where: (Fraction, Fraction)"""
    best, at = Fraction(-1), None
    w, den = coeffs(yv)[:2]
    for i in range(points):
        t = Fraction(i, points - 1)
        D = _bern(den, t)
        if D > 0:
            k2 = sum(_bern(w[c], t) ** 2 for c in range(3)) / D ** 3
            if k2 > best:
                best, at = k2, t
    return best, at


# ------------------------------------------------------------------------------------------------ the certified search
def _norm_bounds(W3, up):
    """a rational at or above (up) / at or below the norm of the integer vector W3"""
    s = sum(x * x for x in W3)
    return Fraction(0) if s == 0 else _isqrt_frac(Fraction(s), up)


def _node_bound(Ws, Ds, R):
    """an upper bound of |W(t)| R / D(t)^(3/2) over a sub-curve with integer coefficients Ws[3][.], Ds (module docstring);
    None: +inf (the smallest D_k is <= 0); 0 if every W_k is the zero vector"""
    NU = [_norm_bounds([Ws[c][k] for c in range(3)], True) for k in range(len(Ds))]
    if not any(NU):
        return Fraction(0)
    dmin = min(Ds)
    if dmin <= 0:
        return None
    s = _isqrt_frac(dmin, False)
    gs = [s * (Fraction(3, 2) * Dk - s * s / 2) for Dk in Ds]
    assert all(g >= s ** 3 > 0 for g in gs)
    lam = max(nu * R / g for nu, g in zip(NU, gs))
    assert lam > 0 and all(lam * g - nu * R >= 0 for nu, g in zip(NU, gs))
    return lam


def certified_max(yv, max_curv, rel=Fraction(1, 10 ** 9), max_nodes=100000, stack=32, co=None):
    """dict(L, H, t, nodes, waiting, status): L <= m <= H, L a rational at or below a value met at t (or 0), H - L <=
    rel max(max_curv, L) with status 'ok'; 'node_cap' / 'depth_cap' as the device names them (more than `stack` sub-curves
    waiting); waiting: the most that waited at once.  Depth-first, the half with the larger bound first."""
    w, den = (co or coeffs(yv))[:2]
    m = len(den) - 1
    q = 1
    for f in w[0] + w[1] + w[2] + den:
        q = q * f.denominator // math.gcd(q, f.denominator)
    # w_k = Ws_k / q^2, den_k = Ds_k / q^2: kappa = |W| R / D^(3/2) with R = q; a split scales by 2^m, m even: R by 2^(m/2)
    Ws = [[int(f * q * q) for f in w[c]] for c in range(3)]
    Ds = [int(f * q * q) for f in den]
    rel, W = Fraction(rel), _F(max_curv)
    out = dict(nodes=1, waiting=0, status='ok')
    L, tL = Fraction(0), Fraction(0)
    if not any(any(r) for r in Ws):
        out.update(L=L, H=Fraction(0), t=tL)
        return out

    def meet(W3, D, R, t):
        nonlocal L, tL
        if D > 0:
            lo = _norm_bounds(W3, False) * R / (D * _isqrt_frac(D, True))
            if lo > L:
                L, tL = lo, t
    meet([Ws[c][0] for c in range(3)], Ds[0], q, Fraction(0))
    meet([Ws[c][m] for c in range(3)], Ds[m], q, Fraction(1))

    def open_(ub):
        return ub is None or ub - L > rel * max(W, L)
    H = None          # the largest bound of a closed sub-curve
    ub = _node_bound(Ws, Ds, q)
    todo = []
    cur = (Ws, Ds, q, Fraction(0), Fraction(1), ub) if open_(ub) else None
    if cur is None:
        H = ub
    while cur is not None:
        if out['nodes'] + 2 > max_nodes:
            out['status'] = 'node_cap'
            break
        Wc, Dc, R, t0, wd, _ = cur
        halves = [_split(Wc[c]) for c in range(3)]
        dl, dr = _split(Dc)
        wl, wr = [h[0] for h in halves], [h[1] for h in halves]
        R2, hw = R << (m // 2), wd / 2
        out['nodes'] += 2
        meet([wl[c][m] for c in range(3)], dl[m], R2, t0 + hw)
        kids = []
        for Wk, Dk, ta in ((wl, dl, t0), (wr, dr, t0 + hw)):
            b = _node_bound(Wk, Dk, R2)
            if open_(b):
                kids.append((Wk, Dk, R2, ta, hw, b))
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
    if out['status'] != 'ok':
        H = None
    else:
        H = L if H is None or H < L else H
    out.update(L=L, H=H, t=tL)
    return out


# ------------------------------------------------------------------------------------------------ the envelope block
def block_parts(yv, t):
    """dict of the block's exact rational factors at t: n, v, a, w, w2 = |w|^2, den, A, Cc, G[3][n+1], H[3][n+1] and the
    magnitudes mA, mC, mv, ma"""
    v, a, wb, ub, P = derivatives(yv, t)
    n = len(P[0]) - 1

    def at(b, i):
        return b[i] if 0 <= i < len(b) else Fraction(0)
    A = [n * (at(wb, i - 1) - at(wb, i)) for i in range(n + 1)]
    Cc = [n * (n - 1) * (at(ub, i - 2) - 2 * at(ub, i - 1) + at(ub, i)) for i in range(n + 1)]
    mA = [n * (at(wb, i - 1) + at(wb, i)) for i in range(n + 1)]
    mC = [n * (n - 1) * (at(ub, i - 2) + 2 * at(ub, i - 1) + at(ub, i)) for i in range(n + 1)]
    mv = [n * sum(wb[i] * (abs(P[c][i + 1]) + abs(P[c][i])) for i in range(n)) for c in range(3)]
    ma = [n * (n - 1) * sum(ub[i] * (abs(P[c][i + 2]) + 2 * abs(P[c][i + 1]) + abs(P[c][i])) for i in range(n - 1)) for c in range(3)]
    w = cross(v, a)
    axw, wxv = cross(a, w), cross(w, v)
    G = [[A[i] * axw[d] + Cc[i] * wxv[d] for i in range(n + 1)] for d in range(3)]
    H = [[3 * v[d] * A[i] for i in range(n + 1)] for d in range(3)]
    return dict(n=n, v=v, a=a, w=w, w2=sum(x * x for x in w), den=sum(x * x for x in v), A=A, Cc=Cc, G=G, H=H,
                mA=mA, mC=mC, mv=mv, ma=ma)


def kappa2_gradient(yv, t):
    """[3][n + 1] Fractions: d kappa^2 / d P[d][i] at t = 2 (G / den^3 - |w|^2 H / den^4), exact"""
    p = block_parts(yv, t)
    return [[2 * (p['G'][d][i] / p['den'] ** 3 - p['w2'] * p['H'][d][i] / p['den'] ** 4) for i in range(p['n'] + 1)] for d in range(3)]


def envelope_block(yv, t):
    """[3][n + 1] mpf: d row / d P[d][i] at t (w and the speed do not vanish there)"""
    p = block_parts(yv, t)
    nw, d = mpmath.sqrt(_mp(p['w2'])), _mp(p['den'])
    d32 = d * mpmath.sqrt(d)
    d52 = d * d32
    return [[-(_mp(p['G'][c][i]) / (nw * d32) - nw * _mp(p['H'][c][i]) / d52) for i in range(p['n'] + 1)] for c in range(3)]


def block_majorant(yv, t):
    """(K_blk, M_blk[3][n + 1] mpf): |device entry - exact entry| <= 1.05 K_blk UNIT M_blk (module docstring); inf where
    K_blk UNIT rho sigma > 1e-3"""
    p = block_parts(yv, t)
    n = p['n']
    K = 43 * n + 50
    inf = [[mpmath.inf] * (n + 1) for _ in range(3)]
    mv, ma, mA, mC = p['mv'], p['ma'], p['mA'], p['mC']
    mden = sum(x * x for x in mv)
    mw = [mv[a] * ma[b] + mv[b] * ma[a] for a, b in PAIRS]
    if p['den'] <= 0 or p['w2'] <= 0:
        return K, inf
    nw, nmw = mpmath.sqrt(_mp(p['w2'])), mpmath.sqrt(_mp(sum(x * x for x in mw)))
    rho, sigma = _mp(mden / p['den']), nmw / nw
    if K * _mp(UNIT) * rho * sigma > mpmath.mpf("1e-3"):
        return K, inf
    d = _mp(p['den'])
    d32 = d * mpmath.sqrt(d)
    d52 = d * d32
    q = 3 * nw / d52
    exact = envelope_block(yv, t)
    out = []
    for c, (a, b) in enumerate(PAIRS):
        mP, mQ = sigma * _mp(ma[a] + ma[b]), sigma * _mp(mv[a] + mv[b])
        row = []
        for i in range(n + 1):
            mG = mP * _mp(mA[i]) + mQ * _mp(mC[i])
            Gp = abs(_mp(p['G'][c][i])) / nw
            row.append((mG + rho * Gp) / d32 + 3 * nmw * _mp(mv[c] * mA[i]) / d52 + 2 * rho * q * _mp(mv[c] * mA[i]) + abs(exact[c][i]))
        out.append(row)
    return K, out


# ------------------------------------------------------------------------------------------------ inputs
def seeded(deg, seed):
    """the seeded family lifted to space: a straight line from (0, 0, 0) to (10, 3, 2), N(0, 0.6) noise on every control
    point: [3][deg + 1]"""
    rs = np.random.RandomState(seed)
    line = np.stack((np.linspace(0.0, 10.0, deg + 1), np.linspace(0.0, 3.0, deg + 1), np.linspace(0.0, 2.0, deg + 1)))
    return line + 0.6 * rs.randn(3, deg + 1)


# a cusp at t = 1/2 (c' = 0 there) in the plane x = z, w != 0 on both sides of it
CUSP = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]])


def wide_speed():
    """curvature_ref.WIDE_SPEED from t = 1/64 on (a de Casteljau split in float64: the result is its own curve), snapped and
    lifted: [3][5] Fractions, exact in binary64.  The whole curve has its largest curvature at t = 0, an end value no bound
    can miss; from 1/64 on the maximum (53.4 near t = 0.66 of the piece) is inside, the speed varies by far more than 5 x,
    and a tangent taken at the mid-range whatever its sign closes the nodes around it."""
    rows = []
    for row in C.WIDE_SPEED:
        r, right = list(row), [row[-1]]
        while len(r) > 1:
            r = [(1.0 - 0.015625) * r[i] + 0.015625 * r[i + 1] for i in range(len(r) - 1)]
            right.append(r[-1])
        rows.append(right[::-1])
    return lift(snap3(np.array(rows)))


def regular_curves(deg, count, eps_rel, max_nodes, max_curv=0.5):
    """`count` seeded curves of degree deg, seeds in order from 0, on which this file's search ends with at most 32 waiting
    and within max_nodes -- decided here, before any device sees them"""
    out, seed = [], 0
    while len(out) < count:
        yv = seeded(deg, seed)
        seed += 1
        r = certified_max(yv, max_curv, Fraction(eps_rel), max_nodes)
        if r['status'] == 'ok':
            out.append((yv, r))
    return out
