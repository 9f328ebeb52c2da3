#!/usr/bin/env python3
"""Four multirotors in 3-D crossing through one point, separated by a sphere (`maxSep`) and then by a DOWNWASH BOX
(BezOptimization(separationRegion=...)).

A multirotor must not fly through another's downwash, and the accepted model of that is a region tall in z and narrow in x
and y.  With `maxSep` alone -- the reference's |c_i - c_j|^2 >= maxSep^2 -- the cheapest way through a crossing is to stack
the vehicles vertically, a radius apart: exactly what the downwash forbids.  `separationRegion` keeps the RELATIVE curve
c_i - c_j of every pair out of one convex region around the origin, here the box |dx|, |dy| <= r, |dz| <= 3 r: side by side
at r is allowed, one above the other only at 3 r.

  1. `maxSep` = r alone (exact Jacobian), from the straight lines plus noise;
  2. the box beside it, separationRegionJacobian(method='fd'), from solve 1's solution (which violates the box);
  3. the same with method='envelope': one call at x, the first vehicle's block scattered with +1 and -1.

Degree 5, fixed tf.  It prints the objective, the iterations and the box rows (separationRegionConstraints, one per pair in the
order of np.triu_indices) at all three solutions.  SLSQP is a local method on a min-max constraint: the two box solves are
expected to end feasible; that they end at the same objective is printed, not promised.  On the MI355X: solve 1
stops at its 400-iteration limit (status 9) at 45.437463 with four of the six box rows negative, the least -0.527; solve 2 ends
at 45.493547 in 185 iterations, solve 3 at 45.493502 in 172, both with status 0 and every box row >= -4.1e-10.

    python examples/example25_downwash_boxes.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

R = 0.6
INIT = [(-4.0, -4.0, 0.0), (4.0, -4.0, 0.3), (4.0, 4.0, -0.3), (-4.0, 4.0, 0.15)]
FINAL = [(4.0, 4.0, 0.0), (-4.0, 4.0, 0.3), (-4.0, -4.0, -0.3), (4.0, -4.0, 0.15)]


def box(r=R):
    """(A, b) of |dx| <= r, |dy| <= r, |dz| <= 3 r"""
    A = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    return A, np.array([r, r, r, r, 3 * r, 3 * r])


def problem(region=True, degree=5):
    return BezOptimization(numVeh=4, dimension=3, degree=degree, minimizeGoal='Euclidean', maxSep=R, tf=10.0, initPoints=INIT,
                           finalPoints=FINAL, separationRegion=box() if region else None)


def solve(region, method, x0, degree=5, ftol=1e-9, maxiter=400):
    """(BezOptimization, SciPy result): `maxSep` alone (region False) or with the box under the Jacobian `method`"""
    bo = problem(region, degree)
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints, 'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')}]
    if region:
        cons.append({'type': 'ineq', 'fun': bo.separationRegionConstraints,
                     'jac': lambda x: bo.separationRegionJacobian(x, method=method)})
    res = sop.minimize(bo.objectiveFunction, x0=x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def region_rows(x, degree=5):
    """the box rows at x, whatever the solve was"""
    return problem(True, degree).separationRegionConstraints(x)


def run(degree=5):
    """(sphere result, box result under 'fd', box result under 'envelope')"""
    x0 = problem(False, degree).generateGuess(std=0.3, seed=4)
    _, sphere = solve(False, None, x0, degree)
    _, fd = solve(True, 'fd', sphere.x, degree)
    _, env = solve(True, 'envelope', sphere.x, degree)
    return sphere, fd, env


def report(name, res):
    rows = region_rows(res.x)
    print("%-22s objective %.6f (%d iterations, SLSQP status %d); box rows %s" % (name, res.fun, res.nit, res.status,
                                                                                 np.array2string(rows, precision=4)))


if __name__ == "__main__":
    sphere, fd, env = run()
    report("maxSep alone", sphere)
    report("box, 'fd'", fd)
    report("box, 'envelope'", env)
    print("objective under 'envelope' - under 'fd' = %.3e" % (env.fun - fd.fun))
