#!/usr/bin/env python3
"""Generate tests/golden/jerk_rows.npz by RUNNING THE REFERENCE's jerk curve (optimization.py:522-539).

    python -B tests/golden/gen_jerk_rows.py

`_minJerkObjective` sums the control points of `pos.diff().diff().diff().normSquare().elev(DEG_ELEV)` per vehicle; the jerk
bound's rows (obtg_jerk) are that curve under a bound: bound**2 - c_k.  For 4 vehicles at each of the degrees 3, 4, 5, 6, 10,
in 2-D and 3-D, at R = 0 and 3 and tf = 1.0 and 2.5, the file holds the inputs `Y<deg>_<dim>` [4 * dim][deg + 1] and what the
reference's chain returned, `c<deg>_<dim>_<R>_<tf index>` [4][2 deg + R + 1].  Degree 2 is left out: the third derivative of a
parabola is zero, the reference's output there is rounding residue and has no scale to compare on.  gen_golden.py is imported
for its injections (it makes the reference importable); nothing of the reference is copied.  Exits cleanly where the reference
is absent (gen_golden does).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.argv = [sys.argv[0], "none"]
import gen_golden as GG  # noqa: E402  (exits when the reference is absent)

import numpy as np  # noqa: E402

DEGREES = (3, 4, 5, 6, 10)
DIMS = (2, 3)
ELEVS = (0, 3)
TFS = (1.0, 2.5)
COUNT = 4


def main():
    rng = np.random.default_rng(20418)
    d = dict(tfs=np.array(TFS), degrees=np.array(DEGREES, np.int32), dims=np.array(DIMS, np.int32), elevs=np.array(ELEVS, np.int32))
    for deg in DEGREES:
        for dim in DIMS:
            Y = rng.uniform(-10.0, 10.0, (COUNT * dim, deg + 1))
            d["Y%d_%d" % (deg, dim)] = Y
            for R in ELEVS:
                for it, tf in enumerate(TFS):
                    rows = [np.asarray(GG.bez.Bezier(Y[v * dim:(v + 1) * dim].copy(), tf=tf).diff().diff().diff().normSquare().elev(R).cpts,
                                       dtype=np.float64).reshape(-1) for v in range(COUNT)]
                    d["c%d_%d_%d_%d" % (deg, dim, R, it)] = np.array(rows)
            print("  degree %d, %d-D: %d vehicles" % (deg, dim, COUNT))
    path = os.path.join(HERE, "jerk_rows.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
