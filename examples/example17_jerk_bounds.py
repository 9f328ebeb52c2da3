#!/usr/bin/env python3
"""Example16's time-optimal problem (two Dubins cars, degree 10, maxSpeed 5, start and end speed 1) with a bound on the JERK
in place of the acceleration, maxJerk = 10.  Without it the problem ends at tf = 2.427643190 on a trajectory whose jerk
reaches |j| ~ 34 and ~ 121.  The bound is the curve of the reference's jerk objective
(pos.diff().diff().diff().normSquare(), optimization.py:522-539) held under maxJerk^2: maxJerkConstraints, in any dimension.

Solved twice: with the control-point rows (jerkRows='all': the 2n+1 coefficients of maxJerk^2 - (d/2)|j|^2 per vehicle, from
the straight-line guess, Jacobian by one batched finite-difference call) and with the true rows (jerkRows='true_min': per
vehicle the true minimum over the trajectory, obtg_jerk_true_min, with the envelope Jacobian of DESIGN.md 4.18), started from
the first solve's solution.

The bound was chosen in a CPU rehearsal on the control-point rows (the oracle's rows, SciPy's own differences, ftol 1e-10):
maxJerk = 10 converges with status 0 in 22 iterations at tf = 2.772558152, both vehicles' largest control point at the cap
(0.9998 and 1.0000 of it).  Tried and not used: 200 (status 0, but no row binds: tf stays 2.427643190), 100, 50, 30 and 20
(status 0; tf 2.447877161, 2.514473291, 2.563879425, 2.633436246; only vehicle 1 binds), 15 (status 0, tf 2.688127147, 50
iterations), 5 and 3 (status 0; tf 3.000477310 and 3.314607205; both bind, further from the unbounded problem).  None of the
rehearsed values failed to converge.

Measured on the MI355X at ftol = 1e-10: the control-point rows end at tf = 2.772558152 (19 iterations), the rehearsal's
figure.  There vehicle 1's largest jerk is the END coefficient at t = 0, which IS the polynomial's value -- that row is tight,
10.000000 --, and vehicle 0's true maximum is 9.831 (t = 1).  The true rows release the slack the control points leave inside
the span: tf = 2.755968758 (236 iterations), vehicle 1's active maximum now inside the span (10.000000 at t = 0.870),
vehicle 0's at 9.284 (t = 0.826) -- tf is lowered by 0.017 of 2.77, as example16's true acceleration rows lower theirs by 0.026
of 3.12.

    python examples/example17_jerk_bounds.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

MAX_SPEED = 5.0
MAX_JERK = 10.0
TF_UNBOUNDED = 2.427643190        # the same problem without maxJerk (example14's first solve)


def problem(jerk_rows, max_jerk=MAX_JERK):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=MAX_SPEED,
                           maxAngRate=1, initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)],
                           initSpeeds=[1] * numVeh, finalSpeeds=[1] * numVeh, initAngs=[0, np.pi / 2],
                           finalAngs=[0, np.pi / 2], maxJerk=max_jerk, jerkRows=jerk_rows)


def solve(jerk_rows, ftol=1e-10, x0=None, maxiter=1000, max_jerk=MAX_JERK):
    """(BezOptimization, SciPy result) of the solve with `jerk_rows` from x0 (None: the straight-line guess); the other
    constraints are the same in both solves"""
    bo = problem(jerk_rows, max_jerk)
    jerk_method = 'envelope' if jerk_rows == 'true_min' else 'fd'
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxJerkConstraints, 'jac': lambda x: bo.maxJerkJacobian(x, method=jerk_method)},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0) if x0 is None else x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def report(jerk_rows, bo, res):
    hi, t_hi = bo.trueJerkMax(res.x)
    d = bo.model['dim']
    print("jerkRows=%-10r tf* = %.9f (%d iterations, SLSQP status %d, %d jerk rows)"
          % (jerk_rows, res.fun, res.nit, res.status, bo.maxJerkConstraints(res.x).size))
    for v in range(bo.model['numVeh']):
        print("   vehicle %d: largest jerk %.6f (t = %.3f), bound %.1f" % (v, np.sqrt(hi[v] * 2.0 / d), t_hi[v], MAX_JERK))


if __name__ == "__main__":
    out = {}
    out['all'] = solve('all')
    out['true_min'] = solve('true_min', x0=out['all'][1].x)
    for rows in ('all', 'true_min'):
        report(rows, *out[rows])
    print("final time without the bound %.9f, with the control-point rows %.9f, with the true rows %.9f"
          % (TF_UNBOUNDED, out['all'][1].fun, out['true_min'][1].fun))
