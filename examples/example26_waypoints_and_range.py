#!/usr/bin/env python3
"""Example1's two cars on a FIXED time span, with WAYPOINTS and a RANGE LIMIT (BezOptimization(waypoints=.., stayWithin=..),
proximityConstraints): every distance constraint before these was a keep-apart constraint; these say "come close" and "stay
close".

A waypoint (vehicle, point, radius, (tau0, tau1)) asks the vehicle to pass within `radius` of the point at SOME time of the
window (tau0, tau1) of the normalised parameter; its row is the maximum over the window of (d/2)(radius^2 - distance^2).  Two
gates per car with the windows (0, 0.5) and (0.5, 1) are visited in that order.  A range limit (vehicle, other vehicle, R) asks
the pair to stay within R of each other at ALL times; its row is the minimum of the same polynomial.  Solved three ways, at
degree 7, minimising the path's control polygon length (minimizeGoal='Euclidean'):

  1. without waypoints: the cars drive straight -- the example prints how far each passes from its gates;
  2. with the gates and the range limit and the finite-difference Jacobian (one batched call per Jacobian), from solve 1;
  3. with the envelope Jacobian (obtg_proximity_true_jac: the row's polynomial differentiated at the parameter its search
     returns -- DESIGN.md 4.28), from the same start.

For every solve it prints the objective, the iterations and every row's margin from trueProximityMargins, as a distance:
sqrt(radius^2 - 2 val / d) is the closest approach of a waypoint row, the largest separation of a range row.

Measured on the MI355X at ftol = 1e-10: without waypoints objective 18.832587363 (19 iterations); the cars pass 2.357 and 1.736
(car 0), 3.343 and 2.507 (car 1) from their gates and are at most 6.083 apart.  With the lists, from that point: 'fd' 31.228999895
in 199 iterations (SLSQP status 8, smallest row -1.7e-07), 'envelope' 31.228979062 in 222 (status 0, smallest row 2.5e-10); every
gate is passed at distance 0.500000, in order (tau 0.395 and 0.844 for car 0, 0.210 and 0.813 for car 1); the range limit is
not active.

    python examples/example26_waypoints_and_range.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

INIT, FINAL = [(0, 5), (3, 0)], [(8, 4), (7, 10)]
TF = 10.0
RADIUS = 0.5
GATES = [(0, (3.0, 7.0), RADIUS, (0.0, 0.5)), (0, (6.0, 2.5), RADIUS, (0.5, 1.0)),
         (1, (1.0, 4.0), RADIUS, (0.0, 0.5)), (1, (8.5, 7.0), RADIUS, (0.5, 1.0))]
RANGE = [(0, 1, 7.0)]


def problem(degree=7, waypoints=None, stay_within=None):
    return BezOptimization(numVeh=2, dimension=2, degree=degree, minimizeGoal='Euclidean', maxSep=1, maxSpeed=5, tf=TF,
                           initPoints=INIT, finalPoints=FINAL, waypoints=waypoints, stayWithin=stay_within)


def solve(method=None, degree=7, x0=None, waypoints=GATES, stay_within=RANGE, ftol=1e-10, maxiter=500):
    """(BezOptimization, SciPy result): method None -- no proximity rows; 'fd' / 'envelope' -- with the lists and that Jacobian
    of their rows, from x0 (None: the straight-line guess); the other constraints are the same in every solve"""
    bo = problem(degree, None if method is None else waypoints, None if method is None else stay_within)
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')}]
    if method is not None:
        cons.append({'type': 'ineq', 'fun': bo.proximityConstraints, 'jac': lambda x: bo.proximityJacobian(x, method=method)})
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0) if x0 is None else x0, method='SLSQP', constraints=cons,
                       options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def margins(x, degree=7, waypoints=GATES, stay_within=RANGE):
    """(val[P], t_star[P], distance[P]) of the lists at x, whatever the solve was: distance is the closest approach of a
    waypoint row and the largest separation of a range row"""
    bo = problem(degree, waypoints, stay_within)
    val, t = bo.trueProximityMargins(x)
    rho = np.array([e[2] for e in (waypoints or [])] + [e[2] for e in (stay_within or [])], dtype=float)
    return val, t, np.sqrt(np.maximum(rho * rho - 2.0 * val / bo.model['dim'], 0.0))


def report(name, res, degree=7):
    val, t, dist = margins(res.x, degree)
    print("%-22s objective %.9f (%d iterations, SLSQP status %d); smallest row %.3e" % (name, res.fun, res.nit, res.status, val.min()))
    for p, e in enumerate(GATES + RANGE):
        what = "gate %s of car %d, window %s: closest approach" % (e[1], e[0], e[3]) if p < len(GATES) else \
               "cars %d and %d: largest separation" % (e[0], e[1])
        print("   %s %.6f at tau = %.4f (radius %.2f, row %.3e)" % (what, dist[p], t[p], e[2], val[p]))


if __name__ == "__main__":
    _, free = solve(None)
    _, fd = solve('fd', x0=free.x)
    _, env = solve('envelope', x0=free.x)
    report("no waypoints", free)
    report("lists, 'fd'", fd)
    report("lists, 'envelope'", env)
