#!/usr/bin/env python3
"""Generate tests/golden/mixed_degree.npz by RUNNING THE REFERENCE's `_minDist` on curves of different degree.

    python -B tests/golden/gen_mixed_degree.py

`_minDist` (bezier.py:1283-1408) builds poly1 / poly2 from each curve's own control points, takes t1 = p1idx[0] / c1.deg
and t2 = p2idx[0] / c2.deg and splits each curve with its own de Casteljau: nothing in it asks for one degree.  It does
pad a 2-D SECOND curve with `[0] * x1.size` (bezier.py:1302), the first curve's length, so of the planar cases only a
2-D first curve against a 3-D second one is accepted; the groups here are 3-D against 3-D and 2-D against 3-D, degrees
from {2, 4, 5, 10, 15}, every ordered pair of different degrees twice.  The file holds the inputs (one array of control
points with the curves' offsets, as obtg_min_dist_mixed takes them, and the dimension each curve was handed over with),
the triple each call returned, the number of gjkNew calls it made and whether the reference finished (0), ran out of its
time budget (1) or overflowed its stack (2).  A case the reference does not return from within the alarm is recorded as
such and not retried.  gen_golden.py is imported for its injections (it makes the reference importable and counts gjkNew
calls) and for `run_mindist` with its per-call alarm; nothing of the reference is copied.  Exits cleanly where the
reference is absent (gen_golden does).
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
BUDGET = 8.0           # seconds per case
DEGREES = (2, 4, 5, 10, 15)


def random_curve(rng, K, dim, shift):
    """K control points: a random walk from a random start (the same extent at every degree), moved by `shift`"""
    c = rng.uniform(0.0, 3.0, size=(dim, 1)) + np.cumsum(rng.normal(0.0, 4.0 / np.sqrt(K), size=(dim, K)), axis=1)
    c[0] += shift
    return c


def main():
    sys.setrecursionlimit(1000)
    rng = np.random.default_rng(20261)
    cpts, off, dims, pa, pb, res, fin, calls = [], [0], [], [], [], [], [], []
    for dim1 in (3, 2):                                        # (the second curve is 3-D: see above)
        for d1 in DEGREES:
            for d2 in DEGREES:
                if d1 == d2:
                    continue
                for rep in range(1 if dim1 == 2 else 2):      # 40 pairs 3-D against 3-D, 20 pairs 2-D against 3-D
                    c1 = random_curve(rng, d1 + 1, dim1, 0.0)
                    c2 = random_curve(rng, d2 + 1, 3, 2.0 * rep)     # rep 1: further apart, so fewer of them cross
                    st, v, nc = GG.run_mindist(bez.Bezier(c1.copy()), bez.Bezier(c2.copy()), budget=BUDGET)
                    for c, dim in ((c1, dim1), (c2, 3)):
                        p = np.zeros((3, c.shape[1]))
                        p[:dim] = c
                        cpts.append(p.ravel())
                        off.append(off[-1] + c.shape[1])
                        dims.append(dim)
                    pa.append(len(dims) - 2)
                    pb.append(len(dims) - 1)
                    res.append(v)
                    fin.append(st)
                    calls.append(nc if st == 0 else -1)
    fin = np.array(fin, np.int32)
    d = dict(cpts=np.concatenate(cpts), off=np.array(off, np.int32), dims=np.array(dims, np.int32), pa=np.array(pa, np.int32),
             pb=np.array(pb, np.int32), res=np.array(res), fin=fin, calls=np.array(calls, np.int32))
    print("  %d pairs: finished %d, out of time %d, stack overflow %d; most gjkNew calls %d" % (
        fin.size, int((fin == 0).sum()), int((fin == 1).sum()), int((fin == 2).sum()), int(d["calls"].max())))
    path = os.path.join(HERE, "mixed_degree.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
