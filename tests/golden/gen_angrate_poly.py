#!/usr/bin/env python3
"""Generate tests/golden/angrate_poly.npz by RUNNING THE REFERENCE's `_angularRate` (optimization.py:543-574).

    python -B tests/golden/gen_angrate_poly.py

`_angularRate` returns a rational curve whose weights are the Bernstein coefficients of den = x'^2 + y'^2 and whose control
points are num / den coefficient by coefficient, num = y'' x' - x'' y' -- the two polynomials the true angular-rate rows are
made of (obtg_ang_rate_poly: W den -+ num).  For 8 random-walk trajectories at each of the degrees 3, 5, 10 and 15, with
tf = 2.5, the file holds the inputs and what the call returned: `Y<deg>` [8][2][deg + 1], `weights<deg>` [8][2 deg + 1] and
`cw<deg>` = control points x weights [8][2 deg + 1].  gen_golden.py is imported for its injections (it makes the reference
importable); nothing of the reference is copied.  Exits cleanly where the reference is absent (gen_golden does).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.argv = [sys.argv[0], "none"]
import gen_golden as GG  # noqa: E402  (exits when the reference is absent)

import numpy as np  # noqa: E402

DEGREES = (3, 5, 10, 15)
TF = 2.5
COUNT = 8


def random_walk(rng, K):
    """K planar control points: a random walk from a random start (the same extent at every degree)"""
    return rng.uniform(0.0, 3.0, size=(2, 1)) + np.cumsum(rng.normal(0.0, 4.0 / np.sqrt(K), size=(2, K)), axis=1)


def main():
    rng = np.random.default_rng(20262)
    d = dict(tf=np.array(TF), degrees=np.array(DEGREES, np.int32))
    for deg in DEGREES:
        Y = np.stack([random_walk(rng, deg + 1) for _ in range(COUNT)])
        w, cw = [], []
        for y in Y:
            r = GG.opt._angularRate(GG.bez.Bezier(y.copy(), tf=TF))
            wt = np.asarray(r._weights, dtype=np.float64).reshape(-1)
            w.append(wt)
            cw.append(np.asarray(r.cpts, dtype=np.float64).reshape(-1) * wt)
        d["Y%d" % deg], d["weights%d" % deg], d["cw%d" % deg] = Y, np.array(w), np.array(cw)
        print("  degree %d: %d trajectories, %d coefficients each" % (deg, COUNT, 2 * deg + 1))
    path = os.path.join(HERE, "angrate_poly.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
