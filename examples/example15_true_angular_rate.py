#!/usr/bin/env python3
"""example14's time-optimal problem (two Dubins cars, degree 10) at DEG_ELEV = 0, solved twice: with the reference's
angular-rate rows (angRateRows='all': the 4n+1 quotients maxAngRate^2 - num_k/den_k of Bernstein coefficients per vehicle,
which bound omega^2 from one side only and are what the time-optimal drivers set DEG_ELEV = 100 to squeeze) and with the true
angular-rate rows (angRateRows='true_min': per vehicle the true minima over the trajectory of W den - num and W den + num,
obtg_ang_rate_true_min, with the envelope Jacobian of DESIGN.md 4.16).  The other rows and their Jacobians are the same in both
solves.  The true rows are a relaxation of the control-point rows, so the second solve starts from the first one's solution,
which is feasible for it, and can only end with a final time that is not larger.  On THIS problem it ends where it starts
(tf 2.427643190 both ways, the second solve in one iteration): the angular-rate bound is active at the two end points of the
second vehicle, where the control-point rows are already tight, and the speed bound fixes tf beyond that (example14).  What the
true rows change here is the row count, 82 to 4.

Per vehicle and side the report gives the true row, the parameter t_star where it is reached and the angular rate there,
formed with the package's own Bezier arithmetic (diff, mul, evaluation).

    python examples/example15_true_angular_rate.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd import bezier as bez  # noqa: E402
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

MAX_ANG_RATE = 1.0


def problem(ang_rows):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5,
                           maxAngRate=MAX_ANG_RATE, initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)],
                           initSpeeds=[1] * numVeh, finalSpeeds=[1] * numVeh, initAngs=[0, np.pi / 2],
                           finalAngs=[0, np.pi / 2], angRateRows=ang_rows)


def solve(ang_rows, ftol=1e-10, x0=None, maxiter=1000):
    """(BezOptimization, SciPy result) of the solve with `ang_rows` from x0 (None: the straight-line guess); the other
    constraints are the same in both solves"""
    bo = problem(ang_rows)
    ang_method = 'envelope' if ang_rows == 'true_min' else 'exact'
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method=ang_method)},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0) if x0 is None else x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def angular_rate(bo, x, s):
    """[N][len(s)]: every vehicle's angular rate at the parameters s in [0, 1] of the trajectory x, from the package's Bezier
    arithmetic: (y'' x' - x'' y') / (x'^2 + y'^2) with x' = x.diff(), x'' = x'.diff()"""
    y, tf = bo.reshapeVector(x), float(bo._tf_of(x))
    tt = np.atleast_1d(np.asarray(s, dtype=float)) * tf
    out = []
    for v in range(bo.model['numVeh']):
        c = bez.Bezier(y[2 * v:2 * v + 2], tf=tf)
        xd, yd = c.x.diff(), c.y.diff()
        xdd, ydd = xd.diff(), yd.diff()
        num, den = ydd * xd - xdd * yd, xd * xd + yd * yd
        out.append(np.asarray(num(tt)).ravel() / np.asarray(den(tt)).ravel())
    return np.array(out)


def report(ang_rows, bo, res):
    val, t_star = bo.trueAngularRateRows(res.x)
    print("angRateRows=%-10r tf* = %.9f (%d iterations, SLSQP status %d, %d angular-rate rows)"
          % (ang_rows, res.fun, res.nit, res.status, bo.maxAngularRateConstraints(res.x).size))
    for v in range(bo.model['numVeh']):
        for side, name in enumerate(("left ", "right")):
            w = angular_rate(bo, res.x, [t_star[v, side]])[v, 0]
            print("   vehicle %d %s: true row %+.6e at t_star = %.6f, angular rate there %+.6f (bound %.1f)"
                  % (v, name, val[v, side], t_star[v, side], w, MAX_ANG_RATE))


if __name__ == "__main__":
    out = {}
    out['all'] = solve('all')
    out['true_min'] = solve('true_min', x0=out['all'][1].x)
    for rows in ('all', 'true_min'):
        report(rows, *out[rows])
    print("final time with the control-point rows %.9f, with the true rows %.9f" % (out['all'][1].fun, out['true_min'][1].fun))
