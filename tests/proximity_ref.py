"""The yardstick of the proximity rows (obtg_proximity_poly, obtg_proximity_true[_jac]; include/obtg.h states the contract):
vehicle a against b -- another vehicle or a fixed point -- within the Euclidean radius rho on the window [tau0, tau1],

    g(tau) = (d/2) (rho^2 - |c_a(tau) - c_b(tau)|^2),      `within`: min over the window,  `reach`: max over the window.

Two layers.  No device, no oracle, no reference code.

  float   `rows_float`: the coefficient formation restated operation for operation (csrc/bern_device.h proximity_coeffs on the
          counts with a kernel of their own, csrc/extrema_kernels.hip k_prox_rows on the others): the cuts of the window are
          aligned_ref.restrict on the span (0, 1), a fused multiply-add is `fma` below (one rounding of the exact value).  These
          are the expected BITS of obtg_proximity_poly.  `envelope_float` restates the negated envelope_block likewise.
  exact   `rows_exact`: the same polynomial from the same inputs in Fractions -- the cut parameters are the floats the device
          forms (SpanCut: tau0, and (tau1 - tau0) / (1 - tau0) rounded), everything after them exact -- and `extremum_exact`, a
          certified bracket of its minimum or maximum (extrema_ref's best-first bisection; its front end takes float64 rows,
          and g's coefficients carry 1 / C(2n, k), so `certified_min_exact` here is that search on Fractions over a common
          denominator, splitting with extrema_ref._split).  This is the truth.

The rounding allowance of a device value against the truth (`allowance`): K * 2^-53 * M as tests/bezier_algebra_ref.py grants
it, K the count of rounded operations behind one coefficient and M its majorant, both from the formation as written:
    a windowed factor     per cut n levels of `w p[i] + z p[i+1]`: 3 roundings a level and w = 1 - z once, at the magnitude of the
                          POSITIONS (a convex combination does not grow); two cuts: 2 (3 n + 1); the difference 1; C(n, j) u 1
                                                                                                  Kf = 6 n + 4 per factor
    the product           d (n + 1) terms, fma(2, so, dg), the table entry S_k (2), S_k s (1): d (n + 1) + 4, granted
                          d (n + 1) + 20 as constraint_rows_ref grants the separation rows (one formula for both formations)
    the offset and g_k    rho rho, (0.5 d) ., the final fma: 3
    the search            a de Casteljau level at 1/2 is two exact scalings and one rounded sum; a node is 2n levels and the
                          depth is at most 64 halvings: 2 n * 64 roundings at the magnitude of the largest coefficient
    K = 2 Kf + d (n + 1) + 23 + 128 n,     M = (d/2) (sum_q F_q^2 + rho^2),  F_q = max_i |a_q,i| + max_i |b_q,i|
(every coefficient of the difference's square is a weighted mean of products of two factors, each at most F_q).  A derivation,
not a measurement.
"""
import heapq
import os
import sys
from fractions import Fraction
from math import comb, gcd

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aligned_ref as AL  # noqa: E402
import extrema_ref as R  # noqa: E402

WITHIN, REACH = 0, 1
FUSED_NC = (4, 6, 8, 9, 11, 16, 21)          # csrc/obtg_internal.h OBTG_NC_PROX_LIST
U = Fraction(1, 2 ** 53)


def fma(a, b, c):
    """round(a * b + c): one rounding of the exact value (finite operands)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def curve_t(t_w, tau0, tau1):
    """t_star of a window parameter: fma(t_w, tau1 - tau0, tau0)"""
    return t_w if t_w != t_w else fma(t_w, tau1 - tau0, tau0)


def _cuts(tau0, tau1):
    """(head, zh, tail, zt) of SpanCut(0, 1, tau0, tau1), floats"""
    t0, tf = 0.0, 1.0
    head = t0 < tau0
    zh = (tau0 - t0) / (tf - t0)
    if head:
        t0 = tau0
    tail = tf > tau1
    zt = (tau1 - t0) / (tf - t0)
    return head, zh, tail, zt


def _pair(y, pts, dim, n_veh, a, b):
    """(ya[dim][nc], yb[dim][nc], b is a vehicle) of one evaluation row y[n_veh * dim][nc]"""
    y = np.asarray(y, dtype=np.float64)
    ya = y[a * dim:(a + 1) * dim]
    if b < n_veh:
        return ya, y[b * dim:(b + 1) * dim], True
    p = np.asarray(pts, dtype=np.float64).reshape(-1, dim)[b - n_veh]
    return ya, np.repeat(p.reshape(dim, 1), y.shape[1], axis=1), False


def _offset(dim, rho):
    return (0.5 * dim) * (rho * rho)


def _normsq_separable(a, dim):
    """bern_device.h normsq_coeffs on a[dim][nc]: u = C(n, j) a, the folded chain with fma, S_k s"""
    nc = a.shape[1]
    n, L = nc - 1, 2 * nc - 1
    u = np.array([[float(comb(n, j)) * a[q, j] for j in range(nc)] for q in range(dim)])
    c = np.empty(L)
    for k in range(L):
        jlo = max(k - n, 0)
        so, first = 0.0, True
        j = jlo
        while 2 * j < k:
            for q in range(dim):
                so = u[q, j] * u[q, k - j] if first else fma(u[q, j], u[q, k - j], so)
                first = False
            j += 1
        s = so
        if k % 2 == 0:
            h = k // 2
            dg = u[0, h] * u[0, h]
            for q in range(1, dim):
                dg = fma(u[q, h], u[q, h], dg)
            s = fma(2.0, so, dg) if 2 * jlo < k else dg
        Sk = (1.0 if k & 1 else 0.5) * dim / float(comb(2 * n, k))
        c[k] = Sk * s
    return c


def _normsq_generic(x, yb, dim):
    """k_prox_rows / k_generic_normsq_elev at R = 0: ah = (x - y) C(n, i), (0.5 d) sum_q conv_at(ah_q, ah_q, k) / C(2n, k)"""
    nc = x.shape[1]
    n, L = nc - 1, 2 * nc - 1
    ah = np.array([[(x[q, i] - yb[q, i]) * float(comb(n, i)) for i in range(nc)] for q in range(dim)])
    c = np.empty(L)
    for k in range(L):
        s = 0.0
        for q in range(dim):
            t = 0.0
            for j in range(max(0, k - n), min(n, k) + 1):
                t = fma(ah[q, j], ah[q, k - j], t)
            s += t
        c[k] = (0.5 * dim) * s / float(comb(2 * n, k))
    return c


def item_float(y, pts, dim, n_veh, item, par):
    """One item's 2n+1 coefficients of g, float64: the expected bits of obtg_proximity_poly"""
    a, b, _ = (int(v) for v in item)
    rho, tau0, tau1 = (float(v) for v in par)
    ya, yb, veh = _pair(y, pts, dim, n_veh, a, b)
    x = AL.restrict(ya, (0.0, 1.0), (tau0, tau1))
    yy = AL.restrict(yb, (0.0, 1.0), (tau0, tau1)) if veh else np.array(yb)
    nc = x.shape[1]
    c = _normsq_separable(x - yy, dim) if nc in FUSED_NC else _normsq_generic(x, yy, dim)
    off = _offset(dim, rho)
    return np.array([fma(-1.0, v, off) for v in c])


def rows_float(Y, pts, dim, n_veh, items, params):
    """[B][P][2n+1] for a batch Y[B][n_veh * dim][nc]"""
    return np.array([[item_float(y, pts, dim, n_veh, it, pr) for it, pr in zip(items, params)] for y in Y])


# ---------------------------------------------------------------- exact layer
def _fr(v):
    return [Fraction(float(x)) for x in v]


def _restrict_exact(row, tau0, tau1):
    head, zh, tail, zt = _cuts(tau0, tau1)
    p = list(row)
    n = len(p) - 1
    if head:
        z = Fraction(zh)
        cur, right = p, [None] * (n + 1)
        for lev in range(n):
            right[n - lev] = cur[-1]
            cur = [(1 - z) * cur[i] + z * cur[i + 1] for i in range(len(cur) - 1)]
        right[0] = cur[0]
        p = right
    if tail:
        z = Fraction(zt)
        cur, left = p, [None] * (n + 1)
        for lev in range(n):
            left[lev] = cur[0]
            cur = [(1 - z) * cur[i] + z * cur[i + 1] for i in range(len(cur) - 1)]
        left[n] = cur[0]
        p = left
    return p


def item_exact(y, pts, dim, n_veh, item, par):
    """One item's 2n+1 coefficients of g as Fractions"""
    a, b, _ = (int(v) for v in item)
    rho, tau0, tau1 = (float(v) for v in par)
    ya, yb, veh = _pair(y, pts, dim, n_veh, a, b)
    nc = ya.shape[1]
    n = nc - 1
    d = []
    for q in range(dim):
        x = _restrict_exact(_fr(ya[q]), tau0, tau1)
        w = _restrict_exact(_fr(yb[q]), tau0, tau1) if veh else _fr(yb[q])
        d.append([x[i] - w[i] for i in range(nc)])
    half = Fraction(dim, 2)
    off = half * Fraction(rho) ** 2
    out = []
    for k in range(2 * n + 1):
        s = Fraction(0)
        for j in range(max(0, k - n), min(n, k) + 1):
            wgt = comb(n, j) * comb(n, k - j)
            s += wgt * sum(d[q][j] * d[q][k - j] for q in range(dim))
        out.append(off - half * s / comb(2 * n, k))
    return out


def certified_min_exact(c, rel=R.REL, max_nodes=200000):
    """extrema_ref.certified_min on Fractions: dict(L, H, t, nodes, s), L <= min over [0, 1] <= H = p(t), H - L <= rel * s"""
    c = [Fraction(x) for x in c]
    K = len(c)
    s = max(abs(x) for x in c)
    D = 1
    for x in c:
        D = D * x.denominator // gcd(D, x.denominator)
    v = [int(x * D) for x in c]
    H, tH = (c[0], Fraction(0)) if c[0] <= c[-1] else (c[-1], Fraction(1))
    m = min(c)
    if m == c[0] or m == c[-1] or K <= 2:
        return dict(L=H, H=H, t=tH, nodes=1, s=s)
    heap = [(m, 0, v, 0, Fraction(0), Fraction(1))]
    tie, nodes, L = 1, 1, m
    while heap:
        L = min(H, heap[0][0])
        if H - L <= rel * s:
            break
        if nodes >= max_nodes:
            raise RuntimeError("certified_min_exact: node budget")
        _, _, v, e, t0, w = heapq.heappop(heap)
        left, right = R._split(v)
        e2 = e + K - 1
        mid = Fraction(right[0], D << e2)
        tm = t0 + w / 2
        if mid < H:
            H, tH = mid, tm
        nodes += 2
        for piece, a0 in ((left, t0), (right, tm)):
            lb = Fraction(min(piece), D << e2)
            if lb < H:
                heapq.heappush(heap, (lb, tie, piece, e2, a0, w / 2))
                tie += 1
    else:
        L = H
    return dict(L=L, H=H, t=tH, nodes=nodes, s=s)


def extremum_exact(c, kind, rel=R.REL):
    """dict(L, H, t, s): L <= the item's row <= H -- the minimum of g (`within`) or the maximum (`reach`) -- t the WINDOW's
    parameter of the value that closes the bracket from the attained side"""
    if kind == WITHIN:
        return certified_min_exact(c, rel)
    r = certified_min_exact([-x for x in c], rel)
    return dict(L=-r["H"], H=-r["L"], t=r["t"], nodes=r["nodes"], s=r["s"])


def item_truth(y, pts, dim, n_veh, item, par, rel=R.REL):
    return extremum_exact(item_exact(y, pts, dim, n_veh, item, par), int(item[2]), rel)


def allowance(y, pts, dim, n_veh, item, par):
    """K * 2^-53 * M of one item (module docstring), a Fraction"""
    a, b, _ = (int(v) for v in item)
    rho = float(par[0])
    ya, yb, _ = _pair(y, pts, dim, n_veh, a, b)
    n = ya.shape[1] - 1
    K = 2 * (6 * n + 4) + dim * (n + 1) + 23 + 128 * n
    F2 = sum((Fraction(float(np.abs(ya[q]).max())) + Fraction(float(np.abs(yb[q]).max()))) ** 2 for q in range(dim))
    M = Fraction(dim, 2) * (F2 + Fraction(rho) ** 2)
    return K * U * M


# ---------------------------------------------------------------- the first step of the device's search, and the blocks
def first_step_ends(c, kind, eps_rel):
    """extrema_kernels.hip ex_first on a float row: True when node 1 answers the row (no split)"""
    c = np.asarray(c, dtype=np.float64)
    c = -c if kind == REACH else c
    m, s = c.min(), np.abs(c).max()
    if c[0] == m or c[-1] == m:
        return True
    return min(c[0], c[-1]) - m <= eps_rel * s


def envelope_float(y, pts, dim, n_veh, item, t):
    """bern_device.h envelope_block<.., NEG = true> at the curve's parameter t on the unrestricted control points: float64
    [dim][nc], the expected bits of obtg_proximity_true_jac's block"""
    a, b, _ = (int(v) for v in item)
    ya, yb, _ = _pair(y, pts, dim, n_veh, a, b)
    nc = ya.shape[1]
    if t != t:
        return np.full((dim, nc), np.nan)
    s = 1.0 - t
    w = [1.0] + [0.0] * (nc - 1)
    for r in range(1, nc):
        for i in range(r, 0, -1):
            w[i] = fma(t, w[i - 1], s * w[i])
        w[0] = s * w[0]
    out = np.empty((dim, nc))
    for c in range(dim):
        dl = 0.0
        for i in range(nc):
            dl = fma(w[i], ya[c, i] - yb[c, i], dl)
        kd = -(float(dim) * dl)
        out[c] = [kd * w[i] for i in range(nc)]
    return out


def unique_interior(row, kind, grid=512, gap=1e-3):
    """From a float row of g alone: True when the row's extremum over [0, 1] is attained strictly inside, and every grid point
    farther than 1/8 from the best grid point is worse than it by more than gap * max |c_k| (one basin).  -> (ok, t_best)"""
    c = np.asarray(row, dtype=np.float64)
    c = -c if kind == REACH else c
    t = np.linspace(0.0, 1.0, grid + 1)
    v = np.array(c, dtype=np.float64)[:, None] * np.ones_like(t)[None]
    for _ in range(len(c) - 1):
        v = (1.0 - t) * v[:-1] + t * v[1:]
    v = v[0]
    i = int(np.argmin(v))
    far = np.abs(t - t[i]) > 0.125
    ok = 0.125 < t[i] < 0.875 and (v[far] - v[i] > gap * np.abs(c).max()).all()
    return bool(ok), float(t[i])


def unique_interior_items(bt, rows):
    """[(row, item)] of a batch, in order, whose float row (rows[B][P][2n+1]) passes unique_interior"""
    return [(r, p) for r in range(rows.shape[0]) for p, it in enumerate(bt["items"]) if unique_interior(rows[r, p], int(it[2]))[0]]


def second_derivative_exact(c, t):
    """g''(t) of exact Bernstein coefficients c at the Fraction t (in the polynomial's own parameter)"""
    m = len(c) - 1
    d2 = [c[k + 2] - 2 * c[k + 1] + c[k] for k in range(m - 1)]
    while len(d2) > 1:
        d2 = [(1 - t) * d2[i] + t * d2[i + 1] for i in range(len(d2) - 1)]
    return m * (m - 1) * d2[0]


def scatter(blk, items, n_veh, dim, first, num_cols):
    """Dense [P][n_veh * dim * num_cols] from blocks [P][dim][n + 1]: the free columns first .. first + num_cols of a's
    vehicle, negated for b when b is a vehicle (a point has no variable) -- the layout of BezOptimization's x"""
    J = np.zeros((len(items), n_veh * dim * num_cols))
    for p, (a, b, _) in enumerate(items):
        for own, sg in ((int(a), 1.0), (int(b), -1.0)):
            if own < n_veh:
                J[p, own * dim * num_cols:(own + 1) * dim * num_cols] += sg * blk[p][:, first:first + num_cols].reshape(-1)
    return J


# ---------------------------------------------------------------- the batch of the GPU tests
N_VEH, N_PTS, B_ROWS = 3, 2, 4
EPS_REL = 1e-9
#: every combination of {reach, within} x {point, vehicle target} x {full window, proper window}
ITEMS = np.array([[0, N_VEH + 0, REACH], [1, N_VEH + 1, REACH], [0, 1, REACH], [1, 2, REACH],
                  [2, N_VEH + 0, WITHIN], [0, N_VEH + 1, WITHIN], [1, 2, WITHIN], [2, 0, WITHIN]], dtype=np.int32)
WINDOWS = [(0.0, 1.0), (0.25, 0.75), (0.0, 1.0), (0.5, 1.0), (0.0, 1.0), (0.0, 0.5), (0.0, 1.0), (0.3, 0.8)]
CONFIGS = [(2, 3), (2, 5), (2, 10), (2, 4), (3, 3), (3, 5), (3, 10), (3, 4)]        # (dim, degree); 4: the workspace route
#: chosen so that every configuration's batch holds the cases test_proximity_ref.test_batch_holds_every_case lists
SEEDS = {(2, 3): 2, (2, 5): 0, (2, 10): 1, (2, 4): 2, (3, 3): 0, (3, 5): 0, (3, 10): 0, (3, 4): 1}


def batch(dim, deg, seed=None):
    """dict(Y[B][N * dim][deg + 1], pts[Q][dim], items[P][3], params[P][3]): random control points in [-1, 1]^dim, radii drawn
    around the typical distance so that both signs occur"""
    rng = np.random.RandomState(1000 * dim + 10 * deg + (SEEDS[(dim, deg)] if seed is None else seed) * 7919)
    Y = rng.uniform(-1.0, 1.0, (B_ROWS, N_VEH * dim, deg + 1))
    pts = rng.uniform(-1.0, 1.0, (N_PTS, dim))
    rho = rng.uniform(0.4, 1.6, len(ITEMS))
    params = np.array([[r, w[0], w[1]] for r, w in zip(rho, WINDOWS)])
    return dict(Y=Y, pts=pts, items=ITEMS.copy(), params=params, dim=dim, deg=deg)


def batch_cases(bt, eps_rel=EPS_REL):
    """What a batch holds, from the yardstick alone: dict of counts -- splits, neg/pos rows per kind, extrema at a window end
    interior to the curve, extrema at tau = 0 or 1 -- and the per-(row, item) truth"""
    dim, Y, pts = bt["dim"], bt["Y"], bt["pts"]
    rows = rows_float(Y, pts, dim, N_VEH, bt["items"], bt["params"])
    out = dict(splits=0, neg={WITHIN: 0, REACH: 0}, pos={WITHIN: 0, REACH: 0}, window_end=0, curve_end=0, truth=[])
    for r in range(Y.shape[0]):
        for p, (it, pr) in enumerate(zip(bt["items"], bt["params"])):
            kind = int(it[2])
            tr = item_truth(Y[r], pts, dim, N_VEH, it, pr)
            out["truth"].append(tr)
            out["splits"] += not first_step_ends(rows[r, p], kind, eps_rel)
            if tr["H"] < 0:
                out["neg"][kind] += 1
            if tr["L"] > 0:
                out["pos"][kind] += 1
            if tr["t"] in (0, 1):
                tau = pr[1] if tr["t"] == 0 else pr[2]
                if 0.0 < tau < 1.0:
                    out["window_end"] += 1
                else:
                    out["curve_end"] += 1
    out["rows"] = rows
    return out
