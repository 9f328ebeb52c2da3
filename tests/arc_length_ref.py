"""The yardstick of obtg_bern_arc_length / obtg_arc_length_obj: the length of a Bezier curve, L = int_0^1 |c'(t)| dt, and its
gradient with respect to the control points, at 60 decimal digits.  No device, no oracle, no reference code.

    reference(P, panels, breaks)   composite Gauss-Legendre (GL_POINTS nodes per panel, nodes and weights found here by Newton's
                                   method on the Legendre recurrence in `decimal`) over uniform panels of every stretch between
                                   two break points; a cusp of the curve has to be a break point -- between cusps the integrand
                                   is analytic and the rule converges geometrically.  Control points are taken as the exact
                                   binary64 values they are.  Returns dict(len, grad[d][n+1], S, chord) in `decimal`:
                                   grad[c][i] = int (c'_c / |c'|) n (B_(i-1)^(n-1) - B_i^(n-1)) dt, S the length of the control
                                   polygon (a majorant of L), chord = |P_n - P_0| (a minorant).
    kernel_rule(P, eps_rel, max_nodes)
                                   a NumPy restatement, in binary64, of the rule csrc/arclen_kernels.hip states (adaptive
                                   bisection, 8-point Gauss-Legendre per panel, accept when |G - G_l - G_r| <= eps_rel S w):
                                   what the adaptive rule's own truncation error is, measured on the CPU.

The rounding allowances, in units of 2^-53, against csrc/arclen_kernels.hip (n = degree, d = dimension; u = one rounding):

  K_PANEL = 3 n + d + 9    one panel estimate G: the node t = fma(w, h_k, a) 1; the basis B^(n-1)(t) by the de Casteljau
                           recurrence, per level one product and one fma, n - 1 levels: 2 (n - 1); a difference P_(i+1) - P_i 1;
                           the chain of n fma of a velocity component n, its factor n 1; d squares in one chain d, the square
                           root 1; the weight 1, the 8-term sum in three steps 3, the width 1; G_l + G_r 1        -> 3 n + d + 9
                           relative to the panel's share of n sum_i B_i^(n-1) |P_(i+1) - P_i|, whose integral is S.
  k_len(n, d, nodes)       len: K_PANEL and the (nodes - 1) / 2 additions of accepted pairs, one after the other, on S.
  k_grad(n, d, nodes)      one accumulator of the gradient: K_PANEL (the direction c'_c / |c'| and the weight), the lane's
                           (nodes - 1) / 2 fma, the 4 steps of the row reduction, the difference and its factor n 2.
  k_identity(n, d, nodes)  sum_ci grad[c][i] (P_ci - P_c0) against len, and sum_i grad[c][i] against 0: an entry
                           n (A_(i-1) - A_i) has the absolute error k_grad u n (|A|_(i-1) + |A|_i) with |A|_j <= int B_j^(n-1) =
                           1 / n, so the n + 1 entries of a coordinate carry 2 (n + 1) k_grad u together; each meets a factor
                           |P_ci - P_c0| <= S in the first identity (d coordinates) and 1 in the second.
"""
import decimal
import functools
import math
from decimal import Decimal as D

import numpy as np

DIGITS = 60
GL_POINTS = 30
UNIT = 2.0 ** -53
_CTX = decimal.Context(prec=DIGITS)


def k_panel(n, d):
    return 3 * n + d + 9


def k_len(n, d, nodes):
    return k_panel(n, d) + (int(nodes) - 1) // 2


def k_grad(n, d, nodes):
    return k_panel(n, d) + (int(nodes) - 1) // 2 + 4 + 2


def k_identity(n, d, nodes):
    return 2 * (n + 1) * d * k_grad(n, d, nodes)


def eps_floor(n, d):
    """The smallest eps_rel the kernel works with (include/obtg.h): below it the rounding of one panel's sums alone, 2 K_PANEL u
    times the largest speed a control polygon of length S allows, n S, can fail the acceptance test."""
    return 2.0 * n * k_panel(n, d) * UNIT


# ---------------------------------------------------------------------------------------------------------------------
#  Gauss-Legendre nodes and weights on [-1, 1]
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauss_legendre(m, digits=DIGITS):
    """(nodes, weights), ascending, as Decimals good to about `digits` digits: Newton's method on P_m from the three-term
    recurrence, started at the Chebyshev-like guesses cos(pi (i + 3/4) / (m + 1/2)), in 10 guard digits."""
    ctx = decimal.Context(prec=digits + 10)
    xs, ws = [], []
    for i in range(m):
        x = D(math.cos(math.pi * (i + 0.75) / (m + 0.5)))
        for _ in range(100):
            p0, p1 = D(1), x
            for k in range(2, m + 1):
                p0, p1 = p1, ctx.divide(ctx.subtract(ctx.multiply(ctx.multiply(D(2 * k - 1), x), p1), ctx.multiply(D(k - 1), p0)), D(k))
            dp = ctx.divide(ctx.multiply(D(m), ctx.subtract(ctx.multiply(x, p1), p0)), ctx.subtract(ctx.multiply(x, x), D(1)))
            dx = ctx.divide(p1, dp)
            x = ctx.subtract(x, dx)
            if abs(dx) < D(10) ** -(digits + 5):
                break
        p0, p1 = D(1), x
        for k in range(2, m + 1):
            p0, p1 = p1, ctx.divide(ctx.subtract(ctx.multiply(ctx.multiply(D(2 * k - 1), x), p1), ctx.multiply(D(k - 1), p0)), D(k))
        dp = ctx.divide(ctx.multiply(D(m), ctx.subtract(ctx.multiply(x, p1), p0)), ctx.subtract(ctx.multiply(x, x), D(1)))
        xs.append(x)
        ws.append(ctx.divide(D(2), ctx.multiply(ctx.subtract(D(1), ctx.multiply(x, x)), ctx.multiply(dp, dp))))
    order = sorted(range(m), key=lambda i: xs[i])
    return tuple(xs[i] for i in order), tuple(ws[i] for i in order)


def kernel_constants():
    """The 8-point rule as the kernel holds it: h_k = (1 + x_k) / 2 and g_k = omega_k / 2, so that a panel [a, a + w] has the
    nodes a + w h_k and the estimate w sum_k g_k |c'|; each the binary64 nearest to the 60-digit value."""
    xs, ws = gauss_legendre(8)
    return [float((1 + x) / 2) for x in xs], [float(w / 2) for w in ws]


# ---------------------------------------------------------------------------------------------------------------------
#  the 60-digit reference
# ---------------------------------------------------------------------------------------------------------------------
def _exact(P):
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 1:
        P = P[None]
    return [[D(float(v)) for v in row] for row in P]


def polygon_and_chord(P):
    """(S, chord) in `decimal`: the length of the control polygon and the distance of the two end points."""
    with decimal.localcontext(_CTX):
        E = _exact(P)
        n = len(E[0]) - 1
        S = sum((sum(((row[i + 1] - row[i]) ** 2 for row in E), D(0)).sqrt() for i in range(n)), D(0))
        chord = sum(((row[n] - row[0]) ** 2 for row in E), D(0)).sqrt()
    return S, chord


def reference(P, panels=32, breaks=()):
    with decimal.localcontext(_CTX):
        E = _exact(P)
        d, n = len(E), len(E[0]) - 1
        hod = [[n * (row[i + 1] - row[i]) for i in range(n)] for row in E]            # degree n - 1, n coefficients
        binom = [D(math.comb(n - 1, i)) for i in range(n)]
        xs, ws = gauss_legendre(GL_POINTS)
        total = D(0)
        A = [[D(0)] * n for _ in range(d)]           # A[c][j] = int (c'_c / |c'|) B_j^(n-1)
        cuts = [D(0)] + [D(float(b)) for b in sorted(breaks)] + [D(1)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            w = (hi - lo) / panels
            for p in range(panels):
                a = lo + p * w
                for x, wt in zip(xs, ws):
                    t = a + w * (1 + x) / 2
                    s = 1 - t
                    tp, sp = [D(1)], [D(1)]
                    for _ in range(n - 1):
                        tp.append(tp[-1] * t)
                        sp.append(sp[-1] * s)
                    B = [binom[i] * tp[i] * sp[n - 1 - i] for i in range(n)]
                    v = [sum((B[i] * hod[c][i] for i in range(n)), D(0)) for c in range(d)]
                    speed = sum((vc * vc for vc in v), D(0)).sqrt()
                    q = wt * w / 2
                    total += q * speed
                    if speed != 0:
                        for c in range(d):
                            f = q * v[c] / speed
                            for j in range(n):
                                A[c][j] += f * B[j]
        grad = [[n * ((A[c][i - 1] if i >= 1 else D(0)) - (A[c][i] if i < n else D(0))) for i in range(n + 1)] for c in range(d)]
    S, chord = polygon_and_chord(P)
    return dict(len=total, grad=grad, S=S, chord=chord)


# ---------------------------------------------------------------------------------------------------------------------
#  the kernel's rule, restated in NumPy (binary64; no fused multiply-add, sums in NumPy's order)
# ---------------------------------------------------------------------------------------------------------------------
MD_OK, MD_NODE_CAP, MD_DEPTH_CAP = 0, 1, 2
MAX_DEPTH = 48


def kernel_rule(P, eps_rel, max_nodes=100000):
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    d, n = P.shape[0], P.shape[1] - 1
    dh = np.diff(P, axis=1)                                   # [d][n]
    S = float(np.sqrt((dh * dh).sum(axis=0)).sum())
    tol = max(eps_rel, eps_floor(n, d)) * S
    hk, gk = (np.array(v) for v in kernel_constants())

    def panel(a, w):
        t = a + w * hk
        Bm = np.zeros((8, n))
        Bm[:, 0] = 1.0
        for r in range(1, n):
            Bm[:, 1:r + 1] = t[:, None] * Bm[:, 0:r] + (1 - t)[:, None] * Bm[:, 1:r + 1]
            Bm[:, 0] *= 1 - t
        v = n * (Bm @ dh.T)                                   # [8][d]
        speed = np.sqrt((v * v).sum(axis=1))
        return w * float((gk * speed).sum()), (w * gk, speed, v, Bm)

    A = np.zeros((d, n))

    def add(parts):
        q, speed, v, Bm = parts
        f = np.where(speed > 0, q / np.where(speed > 0, speed, 1.0), 0.0)
        A[...] += np.einsum("k,kc,kj->cj", f, v, Bm)

    G, parts = panel(0.0, 1.0)
    cur, stack = (0.0, 1.0, G), []
    total, err, nodes, status = 0.0, 0.0, 1, MD_OK
    while True:
        a, w, G = cur
        if nodes + 2 > max_nodes:
            status = max(status, MD_NODE_CAP)
            for a, w, G in [cur] + stack[::-1]:
                total += G
                add(panel(a, w)[1])
            break
        hw = 0.5 * w
        GL, pl = panel(a, hw)
        GR, pr = panel(a + hw, hw)
        nodes += 2
        e = abs(G - (GL + GR))
        ok = e <= tol * w
        if ok or w <= 2.0 ** -MAX_DEPTH:
            if not ok:
                status = max(status, MD_DEPTH_CAP)
            total += GL + GR
            err += e
            add(pl)
            add(pr)
            if not stack:
                break
            cur = stack.pop()
        else:
            stack.append((a + hw, hw, GR))
            cur = (a, hw, GL)
    grad = np.zeros((d, n + 1))
    grad[:, :n] -= n * A
    grad[:, 1:] += n * A
    chord = float(np.sqrt(((P[:, -1] - P[:, 0]) ** 2).sum()))
    if total > S:                                             # the bracket chord <= L <= S: an end that is passed is returned, with its gradient
        seg = np.sqrt((dh * dh).sum(axis=0))
        u = np.where(seg > 0, dh / np.where(seg > 0, seg, 1.0), 0.0)
        total, grad = S, np.zeros((d, n + 1))
        grad[:, :n] -= u
        grad[:, 1:] += u
    elif total < chord:
        total, grad = chord, np.zeros((d, n + 1))
        grad[:, 0], grad[:, -1] = -(P[:, -1] - P[:, 0]) / chord, (P[:, -1] - P[:, 0]) / chord
    return dict(len=total, err=err, nodes=nodes, status=status, grad=grad, S=S)


# ---------------------------------------------------------------------------------------------------------------------
#  the cases of tests/test_gpu_arc_length.py
# ---------------------------------------------------------------------------------------------------------------------
DEGREES = (1, 2, 3, 5, 8, 10, 11, 20, 31)
DIMS = (1, 2, 3)
EPS = (1e-6, 1e-10)
MIN_SPEED = 1e-2            # every regular case: min over a 1000-point grid of |c'| > MIN_SPEED * S


def random_curve(deg, dim, seed):
    """A seeded random walk with drift along the first axis: every segment N(0, 1) in the other coordinates and U(1, 2) along
    the first -- in one dimension a monotone curve, the only kind whose speed has no zero; S >= 1 at every degree."""
    rng = np.random.default_rng([deg, dim, seed])
    seg = rng.standard_normal((dim, deg))
    seg[0] = rng.uniform(1.0, 2.0, deg)
    P = np.zeros((dim, deg + 1))
    P[:, 1:] = np.cumsum(seg, axis=1)
    return P + rng.uniform(-0.5, 0.5, (dim, 1))


def min_speed_over_grid(P, points=1000):
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    n = P.shape[1] - 1
    dh = n * np.diff(P, axis=1)
    t = np.linspace(0.0, 1.0, points)
    B = np.array([math.comb(n - 1, i) * t ** i * (1 - t) ** (n - 1 - i) for i in range(n)])
    v = dh @ B
    return float(np.sqrt((v * v).sum(axis=0)).min())


def choose_seed(deg, dim):
    """The first seed whose curve keeps MIN_SPEED (SEEDS below is this function's answer for every case)."""
    for seed in range(1000):
        P = random_curve(deg, dim, seed)
        if min_speed_over_grid(P) > MIN_SPEED * float(polygon_and_chord(P)[0]):
            return seed
    raise RuntimeError("no seed")


# python -c "import arc_length_ref as R; print({(n, d): R.choose_seed(n, d) for n in R.DEGREES for d in R.DIMS})"   (in tests/)
SEEDS = {(n, d): 0 for n in DEGREES for d in DIMS}


def regular_cases():
    return [(n, d, random_curve(n, d, SEEDS[(n, d)])) for n in DEGREES for d in DIMS]


CUSP_HALF = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0]])          # c' = 3 (1 - 2 t) (1 - 2 t, 1): length 2 sqrt 2 - 1


def cusp_at(t0=0.3):
    """The cubic (4 (t - t0)^3, 3 (t - t0)^2): c' = 6 (t - t0) (2 (t - t0), 1), a cusp at t0.  Its Bernstein coefficients are
    the blossom's values, formed here in binary64 -- so the curve that is measured is the one these rounded points define,
    whose speed falls to about 1e-16 within about 1e-16 of t0 (a cusp for every purpose of a 1e-10 rule)."""
    u, v = 1.0 - t0, -t0
    x = [4.0 * v * v * v, 4.0 * u * v * v, 4.0 * u * u * v, 4.0 * u * u * u]
    y = [3.0 * v * v, 3.0 * (2.0 * u * v + v * v) / 3.0, 3.0 * (u * u + 2.0 * u * v) / 3.0, 3.0 * u * u]
    return np.array([x, y])


def elevated_line(p0, p1, deg):
    """The segment p0 -> p1 as a curve of degree `deg` with equally spaced control points (a degree-elevated line)."""
    p0, p1 = np.asarray(p0, dtype=float), np.asarray(p1, dtype=float)
    return p0[:, None] + (p1 - p0)[:, None] * (np.arange(deg + 1) / deg)[None]


# The adaptive rule's own error in the gradient on regular_cases(), by eps_rel: the largest |kernel_rule grad - reference
# grad| over every entry of every case (absolute: an entry of the gradient is bounded by 2), measured on the CPU with
#   python -c "import arc_length_ref as R; print(R.measure_gradient_error())"   (in tests/)
# and the bound the device is held to: 4 x that, for the reduction order and the rounding of the device's recurrence.
GRAD_ERR_MEASURED = {1e-6: 1.8892594347841296e-06, 1e-10: 8.948848606582516e-13}
GRAD_MARGIN = 4.0
GRAD_TOL = {e: GRAD_MARGIN * v for e, v in GRAD_ERR_MEASURED.items()}


@functools.lru_cache(maxsize=None)
def _reference_cached(key, panels, breaks):
    return reference(np.frombuffer(key[0], dtype=np.float64).reshape(key[1]), panels=panels, breaks=breaks)


def reference_of(P, panels=32, breaks=()):
    """reference(), computed once per curve and shared among the tests that need it."""
    P = np.ascontiguousarray(np.atleast_2d(np.asarray(P, dtype=np.float64)))
    return _reference_cached((P.tobytes(), P.shape), panels, tuple(breaks))


def measure_gradient_error():
    out = {}
    for eps in EPS:
        worst = 0.0
        for n, d, P in regular_cases():
            ref = np.array([[float(v) for v in row] for row in reference_of(P)["grad"]])
            worst = max(worst, float(np.abs(kernel_rule(P, eps)["grad"] - ref).max()))
        out[eps] = worst
    return out
