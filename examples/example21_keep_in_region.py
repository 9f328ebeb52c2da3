#!/usr/bin/env python3
"""Example1's time-optimal problem (two Dubins cars, maxSpeed 5, start and end speed 1, maxAngRate 1, maxSep 1) with a
KEEP-IN region: each car has to stay inside a box of its own, 0.6 wide, laid along the chord between its two end points
(BezOptimization(keepIn=..), keepInConstraints).  Without it the cars swing out of their boxes on the way -- the example
prints by how much -- because nothing tells them where the road ends.

A keep-in face a . p <= b is b - a . c(t) >= 0 on the whole trajectory: a polynomial of the curve's own degree whose
Bernstein coefficients are LINEAR in the control points.  Solved three ways:

  1. without the region (Example1 as it is);
  2. on the control-point rows (keepInRows='all': every control point inside every face -- exact linear constraints, but
     only sufficient: a control polygon bulges further than its curve);
  3. on the true rows (keepInRows='true_min': per (vehicle, face) the true margin over the trajectory,
     obtg_keep_in_true_min, with the envelope Jacobian of DESIGN.md 4.23), started from solve 2's solution: the true margin
     is piecewise smooth in x, and from the straight-line guess SLSQP has nothing to hold on to.

Measured on the MI355X at ftol = 1e-10: without the region tf = 2.427643190 (25 iterations), car 1 0.0308 outside its box
at t = 0.23.  The control-point rows end at tf = 2.848797402 (16 iterations) with the smallest TRUE margin still 0.091: the
room between the curve and its control polygon is left unused.  The true rows take that room back: tf = 2.428177166 (13
iterations), 0.0005 above the unconstrained time, both of car 1's lateral margins at 1e-15 (t = 0.229 and 0.784).

    python examples/example21_keep_in_region.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

INIT, FINAL = [(0, 5), (3, 0)], [(8, 4), (7, 10)]
WIDTH = 0.3          # half-width of a car's box, across its chord
PAD = 0.1            # what a box extends beyond the car's end points, along its chord


def boxes(width=WIDTH, pad=PAD):
    """per car a box along the chord between its own two end points, 2 width across and pad longer at either end: (A[4][2],
    b[4]) with unit normals -- the margins are distances -- and the faces in the order left of the chord, right of it, ahead
    of the final point, behind the initial one"""
    out = []
    for p0, p1 in zip(np.array(INIT, dtype=float), np.array(FINAL, dtype=float)):
        d = (p1 - p0) / np.linalg.norm(p1 - p0)
        n = np.array([-d[1], d[0]])
        out.append((np.array([n, -n, d, -d]), np.array([n @ p0 + width, -(n @ p0) + width, d @ p1 + pad, -(d @ p0) + pad])))
    return out


def problem(keep_in_rows='all', degree=10, keep_in=None):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=degree, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5,
                           maxAngRate=1, initPoints=INIT, finalPoints=FINAL, initSpeeds=[1] * numVeh, finalSpeeds=[1] * numVeh,
                           initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], keepIn=keep_in, keepInRows=keep_in_rows)


def solve(keep_in_rows=None, degree=10, x0=None, ftol=1e-10, maxiter=1000, width=WIDTH):
    """(BezOptimization, SciPy result): keep_in_rows None -- no region; 'all' / 'true_min' -- with boxes(width) on those rows,
    from x0 (None: the straight-line guess); the other constraints are the same in every solve"""
    bo = problem(keep_in_rows or 'all', degree, None if keep_in_rows is None else boxes(width))
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
    if keep_in_rows is not None:
        method = 'envelope' if keep_in_rows == 'true_min' else 'fd'
        cons.append({'type': 'ineq', 'fun': bo.keepInConstraints, 'jac': lambda x: bo.keepInJacobian(x, method=method)})
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0) if x0 is None else x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def margins(x, degree=10, width=WIDTH):
    """(val[8], t_star[8]) of boxes(width) at x, whatever the solve was: car-major, faces left, right, ahead, behind"""
    return problem('true_min', degree, boxes(width)).trueKeepInMargins(x)


def report(name, res, degree=10):
    val, t = margins(res.x, degree)
    print("%-28s tf* = %.9f (%d iterations, SLSQP status %d); smallest true margin %.6f"
          % (name, res.fun, res.nit, res.status, val.min()))
    for v in range(2):
        print("   car %d: margins (left, right, ahead, behind) %s at t = %s"
              % (v, np.array2string(val[4 * v:4 * v + 4], precision=6), np.array2string(t[4 * v:4 * v + 4], precision=3)))


if __name__ == "__main__":
    _, free = solve(None)
    _, all_rows = solve('all')
    _, true_rows = solve('true_min', x0=all_rows.x)
    report("no region", free)
    report("control-point rows", all_rows)
    report("true rows, from those", true_rows)
