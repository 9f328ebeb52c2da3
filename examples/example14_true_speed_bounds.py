#!/usr/bin/env python3
"""Example1's time-optimal problem (two Dubins cars, degree 10) at DEG_ELEV = 0, solved twice: with the
reference's speed rows (speedRows='all': the 2n+1 control points of (d/2)|v|^2 per vehicle, which bound the speed from one
side only -- the gap DEG_ELEV = 100 exists to squeeze) and with the true speed rows (speedRows='true_min': per vehicle the
true maximum over the trajectory, obtg_speed_true_min, with the envelope Jacobian of DESIGN.md 4.15).  The speed bound fixes
tf in this problem, so the second final time is the smaller one and its true maximum speed sits on the bound.

The second solve starts from the first one's solution.  A time-optimal trajectory rides the bound: at the solution the second
vehicle's speed has THREE maxima on it, and the maximum over t is not differentiable where maxima tie -- the envelope
Jacobian is then the derivative of one of them.  From the conservative solution SLSQP settles on the three peaks (some 200
iterations, most of them spent trading the peaks against each other); from the straight-line guess it wanders among them
and does not finish in 250.

    python examples/example14_true_speed_bounds.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

MAX_SPEED = 5.0


def problem(speed_rows):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=MAX_SPEED,
                           maxAngRate=1, initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)],
                           initSpeeds=[1] * numVeh, finalSpeeds=[1] * numVeh, initAngs=[0, np.pi / 2],
                           finalAngs=[0, np.pi / 2], speedRows=speed_rows)


def solve(speed_rows, ftol=1e-10, x0=None, maxiter=1000):
    """(BezOptimization, SciPy result) of the solve with `speed_rows` from x0 (None: the straight-line guess); the other
    constraints are the same in both solves"""
    bo = problem(speed_rows)
    speed_method = 'envelope' if speed_rows == 'true_min' else 'exact'
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method=speed_method)},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0) if x0 is None else x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def report(speed_rows, bo, res):
    lo, t_lo, hi, t_hi = bo.trueSpeedRange(res.x)
    d = bo.model['dim']
    print("speedRows=%-10r tf* = %.9f (%d iterations, SLSQP status %d, %d speed rows)"
          % (speed_rows, res.fun, res.nit, res.status, bo.maxSpeedConstraints(res.x).size))
    for v in range(bo.model['numVeh']):
        print("   vehicle %d: speed between %.6f (t = %.3f) and %.6f (t = %.3f), bound %.1f"
              % (v, np.sqrt(max(lo[v], 0.0) * 2.0 / d), t_lo[v], np.sqrt(hi[v] * 2.0 / d), t_hi[v], MAX_SPEED))


if __name__ == "__main__":
    out = {}
    out['all'] = solve('all')
    out['true_min'] = solve('true_min', x0=out['all'][1].x)
    for rows in ('all', 'true_min'):
        report(rows, *out[rows])
    print("final time with the control-point rows %.9f, with the true rows %.9f" % (out['all'][1].fun, out['true_min'][1].fun))
