#!/usr/bin/env python3
"""Generate tests/golden/aligned.npz by RUNNING THE REFERENCE's arithmetic on curves with different time spans.

    python -B tests/golden/gen_aligned.py

`Bezier.sub` / `Bezier.add` (bezier.py:318-374) with `_temporalAlignment` (903-941) on seeded pairs of ours: per group the
file holds the curves and their spans, where the reference returned None, the control points of both aligned curves, the
span of the result, `sub(...).normSquare().elev(R).cpts` and its minimum less maxSep**2 for R in (0, 10), and the control
points of `add(...)`.  gen_golden.py is imported for its injections (it makes the reference importable); nothing of the
reference is copied.  Exits cleanly where the reference is absent (gen_golden does).

Spans are sorted uniform pairs in [0, 10]; in some pairs the starts, the ends or both are forced equal (the branches of
the alignment that do not split) and a few pairs touch exactly (tf of one == t0 of the other: None).  Two random intervals
are disjoint with probability 1/3: the script fails unless every group has between 20 % and 45 % pairs without overlap and
at least 100 with.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.argv = [sys.argv[0], "none"]
import gen_golden as GG  # noqa: E402  (exits when the reference is absent)

import numpy as np  # noqa: E402

bez = GG.bez
MAX_SEP = 0.9
ELEVS = (0, 10)
PAIRS = 180
GROUPS = (("d2_deg5", 2, 5, 501), ("d3_deg5", 3, 5, 502), ("d3_deg3", 3, 3, 503), ("d2_deg10", 2, 10, 504),
          ("d3_deg4", 3, 4, 505))          # (degree 4 has no specialised kernel)


def spans_for(rng, n):
    s1 = np.sort(rng.uniform(0.0, 10.0, size=(n, 2)), axis=1)
    s2 = np.sort(rng.uniform(0.0, 10.0, size=(n, 2)), axis=1)
    for i in range(n):
        k = i % 12
        if k in (1, 3):
            s2[i, 0] = s1[i, 0]                      # equal starts
        if k in (2, 3):
            s2[i, 1] = s1[i, 1]                      # equal ends (3: the same span, no alignment at all)
        if i % 30 == 5:
            s2[i, 0] = s1[i, 1]                      # touching: one ends exactly where the other starts
        if i % 30 == 17:
            s1[i, 0] = s2[i, 1]
        for s in (s1, s2):
            if not s[i, 0] < s[i, 1]:
                s[i, 1] = s[i, 0] + rng.uniform(0.5, 3.0)
    return s1, s2


def group(d, name, dim, deg, seed):
    rng = np.random.default_rng(seed)
    nc = deg + 1
    c1 = rng.uniform(-5.0, 5.0, size=(PAIRS, dim, nc))
    c2 = rng.uniform(-5.0, 5.0, size=(PAIRS, dim, nc))
    s1, s2 = spans_for(rng, PAIRS)
    none = np.zeros(PAIRS, dtype=bool)
    a1, a2, add = (np.full((PAIRS, dim, nc), np.nan) for _ in range(3))
    ends = np.full((PAIRS, 2), np.nan)
    rows = {R: np.full((PAIRS, 2 * deg + R + 1), np.nan) for R in ELEVS}
    mins = {R: np.full(PAIRS, np.nan) for R in ELEVS}
    for i in range(PAIRS):
        b1 = bez.Bezier(c1[i].copy(), t0=s1[i, 0], tf=s1[i, 1])
        b2 = bez.Bezier(c2[i].copy(), t0=s2[i, 0], tf=s2[i, 1])
        dv, sm = b1.sub(b2), b1.add(b2)
        assert (dv is None) == (sm is None)
        if dv is None:
            none[i] = True
            continue
        if (s1[i] == s2[i]).all():
            n1, n2 = b1, b2                          # (Bezier.sub does not call the alignment on equal spans)
        else:
            n1, n2 = bez._temporalAlignment(b1, b2)
        a1[i], a2[i], add[i] = n1.cpts, n2.cpts, sm.cpts
        ends[i] = dv.t0, dv.tf
        assert np.array_equal(dv.cpts, n1.cpts - n2.cpts) and (sm.t0, sm.tf) == (dv.t0, dv.tf)
        ns = dv.normSquare()
        for R in ELEVS:
            e = ns.elev(R).cpts if R else ns.cpts
            rows[R][i] = np.asarray(e, dtype=float).reshape(-1)
            mins[R][i] = rows[R][i].min() - MAX_SEP ** 2
    share = float(none.mean())
    print("  %-9s %d pairs, %d overlap, %.1f %% without" % (name, PAIRS, int((~none).sum()), 100 * share), flush=True)
    if not (0.20 <= share <= 0.45) or int((~none).sum()) < 100:
        raise SystemExit("group %s: %.1f %% of the pairs without overlap (20..45 %% wanted), %d with (>= 100 wanted)"
                         % (name, 100 * share, int((~none).sum())))
    d[name + "_c1"], d[name + "_c2"], d[name + "_s1"], d[name + "_s2"] = c1, c2, s1, s2
    d[name + "_none"], d[name + "_a1"], d[name + "_a2"], d[name + "_add"], d[name + "_ends"] = none, a1, a2, add, ends
    for R in ELEVS:
        d["%s_rows%d" % (name, R)], d["%s_min%d" % (name, R)] = rows[R], mins[R]


def main():
    d = {"groups": np.array([g[0] for g in GROUPS]), "dims": np.array([g[1] for g in GROUPS], np.int32),
         "degs": np.array([g[2] for g in GROUPS], np.int32), "max_sep": np.float64(MAX_SEP), "elevs": np.array(ELEVS, np.int32)}
    for name, dim, deg, seed in GROUPS:
        group(d, name, dim, deg, seed)
    path = os.path.join(HERE, "aligned.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    if os.path.getsize(path) >= 1000000:
        raise SystemExit("aligned.npz must stay under 1 MB")


if __name__ == "__main__":
    main()
