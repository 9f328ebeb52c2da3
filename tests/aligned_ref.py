"""NumPy restatement of the reference's arithmetic on curves with different time spans: `_temporalAlignment`
(bezier.py:903-941) through `Bezier.split` (533-572) and `deCasteljauSplit` (985-1027), then `sub`, `normSquare` with its
(d/2) factor (869-889, 1724-1756), `elev` (469-495, 1127-1147) and the minimum of the control points (the sequential
planner's constraint, Examples/SequentialSwarm.py:43-70).  Test infrastructure: tests/test_aligned_ref.py holds every
function here to tests/golden/aligned.npz, which the reference itself wrote (tests/golden/gen_aligned.py); the GPU tests and
tools/aligned_time.py then use it where the fixture has no value (whole B x K tables, CPU pairs per second).
"""
import numpy as np
from scipy.special import binom


def de_casteljau(row, z):
    """-> (left, right) of one coordinate row split at z; `right` in the curve's own orientation (bezier.py:563)."""
    cur = np.array(row, dtype=np.float64)
    n = cur.size - 1
    left, right = np.empty(n + 1), np.empty(n + 1)
    for lev in range(n):
        left[lev], right[n - lev] = cur[0], cur[-1]
        cur = (1 - z) * cur[:-1] + z * cur[1:]
    left[n] = right[0] = cur[0]
    return left, right


def restrict(cpts, span, target):
    """One curve's share of `_temporalAlignment`: cpts[dim][n+1] on span = (t0, tf) cut down to target = (a, e), first what
    lies before a (the right piece of a split at (a - t0)/(tf - t0)), then what lies after e (the left piece of a split of
    THAT piece, which starts at a).  An end that already is the target's is left alone."""
    c = np.array(cpts, dtype=np.float64, ndmin=2)
    t0, tf = float(span[0]), float(span[1])
    a, e = float(target[0]), float(target[1])
    if t0 < a:
        c = np.stack([de_casteljau(r, (a - t0) / (tf - t0))[1] for r in c])
        t0 = a
    if tf > e:
        c = np.stack([de_casteljau(r, (e - t0) / (tf - t0))[0] for r in c])
    return c


def align(c1, s1, c2, s2):
    """-> (aligned c1, aligned c2, (t0, tf)) or None where the spans do not overlap (t0 >= tf: `add` / `sub` return None)."""
    t0, tf = max(s1[0], s2[0]), min(s1[1], s2[1])
    if t0 >= tf:
        return None
    return restrict(c1, s1, (t0, tf)), restrict(c2, s2, (t0, tf)), (t0, tf)


def norm_square(x):
    """(d/2) |x|^2 as the 2n+1 Bernstein coefficients."""
    x = np.atleast_2d(x)
    d, nc = x.shape
    n = nc - 1
    bn = binom(n, np.arange(nc))
    out = np.zeros(2 * n + 1)
    for q in range(d):
        out += np.convolve(bn * x[q], bn * x[q])
    return (d / 2.0) * out / binom(2 * n, np.arange(2 * n + 1))


def elev(c, R):
    if R == 0:
        return np.array(c, dtype=np.float64)
    n = c.size - 1
    return np.convolve(binom(n, np.arange(n + 1)) * c, binom(R, np.arange(R + 1))) / binom(n + R, np.arange(n + R + 1))


def sep_rows(c1, s1, c2, s2, R):
    """`c1.sub(c2).normSquare().elev(R).cpts` as a vector, or None."""
    al = align(c1, s1, c2, s2)
    return None if al is None else elev(norm_square(al[0] - al[1]), R)


def sep_min(c1, s1, c2, s2, R, max_sep, no_overlap=np.inf):
    rows = sep_rows(c1, s1, c2, s2, R)
    return no_overlap if rows is None else rows.min() - max_sep ** 2


def one_vs_many(one, one_span, many, many_span, R, max_sep, no_overlap=np.inf):
    """out[B][K] of obtg_one_vs_many_min_spans."""
    return np.array([[sep_min(o, so, m, sm, R, max_sep, no_overlap) for m, sm in zip(many, many_span)]
                     for o, so in zip(one, one_span)])
