#!/usr/bin/env python3
"""Example14's time-optimal problem (two Dubins cars, degree 10, maxSpeed 5, start and end speed 1) with a bound on the
ACCELERATION, maxAccel = 4.  Without it the problem ends at tf = 2.427643190 on a trajectory whose acceleration reaches
|a| ~ 23 -- on vehicles whose speed is capped at 5.  The bound is the curve of the reference's acceleration objective
(pos.diff().diff().normSquare(), optimization.py:503-519) held under maxAccel^2: maxAccelConstraints, in any dimension.

Solved twice: with the control-point rows (accelRows='all': the 2n+1 coefficients of maxAccel^2 - (d/2)|a|^2 per vehicle, from
the straight-line guess, Jacobian by one batched finite-difference call) and with the true rows (accelRows='true_min': per
vehicle the true minimum over the trajectory, obtg_accel_true_min, with the envelope Jacobian of DESIGN.md 4.17), started from
the first solve's solution.

Measured on the MI355X at ftol = 1e-10: the control-point rows end at tf = 3.120132305 (32 iterations).  There vehicle 1's
largest acceleration is the END coefficient at t = 0, which IS the polynomial's value -- that row is tight, 4.000000 --, and
vehicle 0's true maximum is 3.964 (t = 1).  Inside the span the control points only bound the rows from one side; the true
rows release that slack: tf = 3.093995027 (300 iterations), vehicle 1's active maximum now inside the span (4.000000 at
t = 0.125), vehicle 0's at 3.894 (t = 0.933).  A CPU rehearsal on the control-point rows had suggested that tf would be kept
because the binding maximum is an end coefficient; it is lowered, but by little -- 0.026 of 3.12 -- where example14's true
speed rows, whose maxima are all inside, gain 0.10 of 2.43.

    python examples/example16_acceleration_bounds.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

MAX_SPEED = 5.0
MAX_ACCEL = 4.0
TF_UNBOUNDED = 2.427643190        # the same problem without maxAccel (example14's first solve)


def problem(accel_rows, max_accel=MAX_ACCEL):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=MAX_SPEED,
                           maxAngRate=1, initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)],
                           initSpeeds=[1] * numVeh, finalSpeeds=[1] * numVeh, initAngs=[0, np.pi / 2],
                           finalAngs=[0, np.pi / 2], maxAccel=max_accel, accelRows=accel_rows)


def solve(accel_rows, ftol=1e-10, x0=None, maxiter=1000, max_accel=MAX_ACCEL):
    """(BezOptimization, SciPy result) of the solve with `accel_rows` from x0 (None: the straight-line guess); the other
    constraints are the same in both solves"""
    bo = problem(accel_rows, max_accel)
    accel_method = 'envelope' if accel_rows == 'true_min' else 'fd'
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAccelConstraints, 'jac': lambda x: bo.maxAccelJacobian(x, method=accel_method)},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0) if x0 is None else x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def report(accel_rows, bo, res):
    hi, t_hi = bo.trueAccelMax(res.x)
    d = bo.model['dim']
    print("accelRows=%-10r tf* = %.9f (%d iterations, SLSQP status %d, %d acceleration rows)"
          % (accel_rows, res.fun, res.nit, res.status, bo.maxAccelConstraints(res.x).size))
    for v in range(bo.model['numVeh']):
        print("   vehicle %d: largest acceleration %.6f (t = %.3f), bound %.1f" % (v, np.sqrt(hi[v] * 2.0 / d), t_hi[v], MAX_ACCEL))


if __name__ == "__main__":
    out = {}
    out['all'] = solve('all')
    out['true_min'] = solve('true_min', x0=out['all'][1].x)
    for rows in ('all', 'true_min'):
        report(rows, *out[rows])
    print("final time without the bound %.9f, with the control-point rows %.9f, with the true rows %.9f"
          % (TF_UNBOUNDED, out['all'][1].fun, out['true_min'][1].fun))
