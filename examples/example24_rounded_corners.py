#!/usr/bin/env python3
"""Example22's cars and square with a MARGIN -- a round vehicle of radius 0.3 -- under both keep-out metrics
(BezOptimization(keepOutMetric='faces' | 'euclidean')).

The faces metric measures the square by G = max_f (a_f . c - b_f), which is the distance only where the nearest feature is a
face: beside a corner it is smaller, by up to sqrt(2).  With keepOutMargin = r it keeps the vehicle out of the square inflated
with SHARP corners, where a disc only needs ROUNDED ones -- and a time-optimal path turns round a corner.  The Euclidean
metric is the signed distance itself: the same rows on faces, the true distance beside corners, minus the
depth inside, and C^1 outside, so its envelope Jacobian needs no co-activity rule.

  1. 'faces', envelope Jacobian, from example22's unconstrained optimum (which drives through the square);
  2. 'euclidean', envelope Jacobian, started from solve 1's solution (feasible for it: D >= G).

For both it prints tf, the iterations and, per car, BOTH true clearances of the result: the faces row and the Euclidean row
(each minus the margin).  SLSQP is a local method: the Euclidean tf is expected to be the smaller one, and is printed, not
promised.

    python examples/example24_rounded_corners.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import example22_keep_out_obstacles as ex22  # noqa: E402
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

MARGIN = 0.3


def problem(metric, degree=5, margin=MARGIN):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=degree, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5,
                           maxAngRate=1, initPoints=ex22.INIT, finalPoints=ex22.FINAL, initSpeeds=[1] * numVeh,
                           finalSpeeds=[1] * numVeh, initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], keepOut=ex22.obstacles(),
                           keepOutMargin=margin, keepOutMetric=metric)


def solve(metric, x0, degree=5, ftol=1e-10, maxiter=1000):
    """(BezOptimization, SciPy result) under `metric`, the envelope Jacobian of its rows, from x0"""
    bo = problem(metric, degree)
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)},
            {'type': 'ineq', 'fun': bo.keepOutConstraints, 'jac': lambda x: bo.keepOutJacobian(x, method='envelope')}]
    res = sop.minimize(bo.objectiveFunction, x0=x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def clearances(x, metric, degree=5):
    """trueKeepOutClearances of the square at x under `metric` (the margin taken off), whatever the solve was"""
    return problem(metric, degree).trueKeepOutClearances(x)


def run(degree=5):
    """(faces result, euclidean result): example22's unconstrained optimum, then the two solves"""
    _, free = ex22.solve(None, degree)
    _, faces = solve('faces', free.x, degree)
    _, euclid = solve('euclidean', faces.x, degree)
    return free, faces, euclid


def report(name, res, degree=5):
    cf, ce = clearances(res.x, 'faces', degree), clearances(res.x, 'euclidean', degree)
    print("%-12s tf* = %.9f (%d iterations, SLSQP status %d)" % (name, res.fun, res.nit, res.status))
    for v in range(2):
        print("   car %d: faces row %.6f at t = %.4f; Euclidean row %.6f at t = %.4f (active set %s)"
              % (v, cf['val'][v], cf['t_star'][v], ce['val'][v], ce['t_star'][v], [int(f) for f in ce['faces'][v] if f >= 0]))


if __name__ == "__main__":
    free, faces, euclid = run()
    print("margin %.2f; without the obstacle tf* = %.9f" % (MARGIN, free.fun))
    report("'faces'", faces)
    report("'euclidean'", euclid)
    print("tf under 'euclidean' - tf under 'faces' = %.3e" % (euclid.fun - faces.fun))
