#!/usr/bin/env python3
"""True extrema of Bezier curves and the tight continuous-time separation constraint.

(a) The reference's own lines (Examples/3D_Plots.py:167-172, Examples/PlotGenerationForPaper.py:183-188):
    c6.min(dim=1), c6.max(dim=1).  Here they are the curve's true extrema within `tol` (obtg_bern_extrema); the
    reference's recursion returns 1.7744000000000004 for the minimum (true: 2.26066686...) and does not return for the
    maximum.
(b) A small swarm solved at DEG_ELEV = 0 twice: with one control-point row per pair (separationRows='min', a LOWER
    BOUND of the squared separation) and with the true minimum per pair (separationRows='true_min').  For both results
    every pair's true minimum separation and the time it is reached, from obtg_temporal_sep_true_min.

    python examples/example10_true_separation.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd import bezier as bez  # noqa: E402
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402


def extrema_lines():
    c6 = bez.Bezier(np.array([(0, 1, 2, 3, 4, 5), (5, 0, 2, 5, 7, 5)], dtype=float))
    print("c6.min(dim=1) = %.12f" % c6.min(dim=1))
    print("c6.max(dim=1) = %.12f" % c6.max(dim=1))


def solve(rows, max_sep=1.0, tf=10.0):
    bo = BezOptimization(numVeh=3, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=max_sep, tf=tf,
                         initPoints=[(0.0, 0.0), (0.0, 4.0), (3.0, -1.0)], finalPoints=[(6.0, 4.0), (6.0, 0.0), (3.0, 5.0)],
                         separationRows=rows)
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints, 'jac': bo.temporalSeparationJacobian}]
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0.3, seed=2), method='SLSQP', constraints=cons,
                       options={'maxiter': 300, 'ftol': 1e-10, 'disp': False})
    val, t_star = bo.trueMinSeparation(res.x)
    print("separationRows=%r: path length %.6f after %d iterations (SLSQP status %d)" % (rows, res.fun, res.nit, res.status))
    pairs = [(i, j) for i in range(3) for j in range(i + 1, 3)]
    for (i, j), v, t in zip(pairs, val, t_star):
        # the rows carry normSquare's (d/2) factor (1 in the plane): v = min |p_i - p_j|^2 - maxSep^2
        print("   vehicles %d and %d: closest at t = %6.3f s, separation %.6f (bound %.1f)"
              % (i, j, t * tf, np.sqrt(max(v + max_sep ** 2, 0.0)), max_sep))
    return res


if __name__ == "__main__":
    extrema_lines()
    a = solve('min')
    b = solve('true_min')
    print("path length with the control-point bound %.6f, with the true minimum %.6f" % (a.fun, b.fun))
