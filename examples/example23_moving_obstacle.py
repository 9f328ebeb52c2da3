#!/usr/bin/env python3
"""Example22's problem (two Dubins cars, time-optimal; a square, 1 wide, on the straight line between car 0's end points) with
a square that MOVES (BezOptimization(keepOut=.., keepOutMotion=..)).

A moving obstacle keeps its faces and is translated by a Bezier offset q(time) on the absolute span [0, T].  A car's row is
the static keep-out row of the RELATIVE curve c(s) - q(s tf): positive while the car stays outside the body wherever the body
is at that moment, minus the depth inside.  In a time-optimal problem the row depends on tf itself -- leaving later meets the
obstacle elsewhere -- and the envelope Jacobian carries that in its tf column (obtg_keep_out_moving_true_min_jac; DESIGN.md
4.25).  Two scenes:

  parked    the square stands on car 0's chord for the whole span (keepOutMotion=[None]: example22's rows);
  crossing  the square starts 1.5 above that place and comes down along a straight line at unit speed, T = 6: it is on the
            chord when the unconstrained car 0 gets there.

Each scene is solved with the finite-difference Jacobian and with the envelope Jacobian of the keep-out rows, from the
solution without an obstacle.  For every solve it prints tf, the iterations and per car the clearance and the parameter
where it is reached.

    python examples/example23_moving_obstacle.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import example22_keep_out_obstacles as ex22  # noqa: E402
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

SPAN = 6.0                                                   # the motion's span T
OFFSET = np.array([[0.0, 0.0], [1.5, 1.5 - SPAN]])           # q(time) = (0, 1.5 - time): straight down, unit speed
SCENES = {"parked": [None], "crossing": [(OFFSET, SPAN)]}


def problem(scene, degree=5):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=degree, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5,
                           maxAngRate=1, initPoints=ex22.INIT, finalPoints=ex22.FINAL, initSpeeds=[1] * numVeh,
                           finalSpeeds=[1] * numVeh, initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], keepOut=ex22.obstacles(),
                           keepOutMotion=SCENES[scene])


def solve(scene, method, x0, degree=5, ftol=1e-10, maxiter=1000):
    """(BezOptimization, SciPy result) of the scene under the keep-out rows' Jacobian `method` ('fd' / 'envelope'), from x0"""
    bo = problem(scene, degree)
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)},
            {'type': 'ineq', 'fun': bo.keepOutConstraints, 'jac': lambda x: bo.keepOutJacobian(x, method=method)}]
    res = sop.minimize(bo.objectiveFunction, x0=x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def clearances(scene, x, degree=5):
    """dict(val[2], t_star[2], face[2][2], lam[2], status[2]) of the scene's square at x: one row per car"""
    return problem(scene, degree).trueKeepOutClearances(x)


def report(name, scene, res, degree=5):
    c = clearances(scene, res.x, degree)
    print("%-22s tf* = %.9f (%d iterations, SLSQP status %d); smallest clearance %.6f" % (name, res.fun, res.nit, res.status, c['val'].min()))
    for v in range(2):
        print("   car %d: clearance %.6f at s = %.4f (time %.4f; faces %s, weight %.4f)"
              % (v, c['val'][v], c['t_star'][v], c['t_star'][v] * res.x[-1], c['face'][v].tolist(), c['lam'][v]))


if __name__ == "__main__":
    _, free = ex22.solve(None)
    for scene in SCENES:
        print("%s: without the obstacle (tf %.9f) the clearances are %s" % (scene, free.fun, clearances(scene, free.x)['val'].tolist()))
        for method in ('fd', 'envelope'):
            _, res = solve(scene, method, free.x)
            report("%s, %r" % (scene, method), scene, res)
