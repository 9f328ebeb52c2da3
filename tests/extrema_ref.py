"""The yardstick of the true-extrema tests: a certified bracket [L, H] of the minimum of a Bernstein polynomial over [0, 1]
in EXACT arithmetic.  No device, no reference code.

A float64 coefficient is a dyadic rational, so a row is a list of integers over a common power of two, and de Casteljau
at 1/2 is additions alone: level r holds the level's values times 2^r.  Best-first bisection: the sub-curve with the
smallest coefficient is split next, the end-point values met bound the minimum from above (H), the smallest coefficient
over the sub-curves still alive bounds it from below (L); a sub-curve whose smallest coefficient is not below H is dropped.
Stops with H - L <= rel * s, s = the largest coefficient magnitude.  Everything returned is a Fraction."""
import heapq
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

REL = Fraction(1, 10 ** 13)


def _split(v):
    """ints v (values x 2^e) -> (left, right), both x 2^(e + K - 1)"""
    K = len(v)
    b = list(v)
    left = [b[0] << (K - 1)]
    right = [0] * K
    right[K - 1] = b[K - 1] << (K - 1)
    for r in range(1, K):
        b = [b[i] + b[i + 1] for i in range(K - r)]          # level r, times 2^r
        left.append(b[0] << (K - 1 - r))
        right[K - 1 - r] = b[K - 1 - r] << (K - 1 - r)
    return left, right


def certified_min(coeffs, rel=REL, max_nodes=200000):
    """dict(L, H, t, nodes, s): L <= min over [0, 1] <= H = p(t), H - L <= rel * s, all exact."""
    c = [Fraction(float(x)) for x in np.asarray(coeffs, dtype=np.float64).reshape(-1)]
    K = len(c)
    s = max(abs(x) for x in c)
    den = 1
    for x in c:
        den = max(den, x.denominator)
    e = den.bit_length() - 1                                  # denominators are powers of two
    v = [int(x * den) for x in c]
    H, tH = (c[0], Fraction(0)) if c[0] <= c[-1] else (c[-1], Fraction(1))
    m = min(c)
    nodes = 1
    if m == c[0] or m == c[-1] or K <= 2:
        return dict(L=H, H=H, t=tH, nodes=1, s=s)
    heap = [(m, 0, v, e, Fraction(0), Fraction(1))]
    tie = 1
    L = m
    while heap:
        L = min(H, heap[0][0])
        if H - L <= rel * s:
            break
        if nodes >= max_nodes:
            raise RuntimeError("certified_min: node budget")
        _, _, v, e, t0, w = heapq.heappop(heap)
        left, right = _split(v)
        e2 = e + K - 1
        mid = Fraction(right[0], 1 << e2)
        tm = t0 + w / 2
        if mid < H:
            H, tH = mid, tm
        nodes += 2
        for piece, a in ((left, t0), (right, tm)):
            lb = Fraction(min(piece), 1 << e2)
            if lb < H:
                heapq.heappush(heap, (lb, tie, piece, e2, a, w / 2))
                tie += 1
    else:
        L = H
    return dict(L=L, H=H, t=tH, nodes=nodes, s=s)


def certified_max(coeffs, rel=REL):
    """dict(L, H, t, ...) of the MAXIMUM: L <= max <= H (the negated bracket of the minimum of the negated row)"""
    r = certified_min(-np.asarray(coeffs, dtype=np.float64), rel)
    return dict(L=-r["H"], H=-r["L"], t=r["t"], nodes=r["nodes"], s=r["s"])


def separation_coeffs(y, n_obj, dim, max_sep):
    """The pair polynomials of one evaluation row y[n_obj * dim][n + 1] (point obstacles as constant curves behind the
    vehicles): oracle.temporal_sep at R = 0, [P][2n + 1]."""
    from oracle import oracle as O
    y = np.ascontiguousarray(y, dtype=np.float64)
    n = y.shape[1] - 1
    return O.temporal_sep(y, n_obj, dim, 0, max_sep).reshape(-1, 2 * n + 1)
