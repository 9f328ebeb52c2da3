#!/usr/bin/env python3
"""Example1's time-optimal problem (two Dubins cars, degree 10) at DEG_ELEV = 0, solved with the angular-rate bound alone and
with a curvature bound added -- the limit that defines a Dubins car, a minimum turning radius of 1 / maxCurvature.

The angular-rate rows are in units of maxAngRate * speed^2: as tf moves they tighten or loosen, and a slow car may turn on the
spot.  The curvature rows (maxCurvature=..., obtg_curvature_true_min: per vehicle and side maxCurvature minus the true maximum
over the path of +-kappa, kappa = (y'' x' - x'' y') / |v|^3) do not move with tf.  The curvature run is done twice, with the
forward-difference Jacobian of the rows ('fd': the search differenced, one batched call) and with their envelope Jacobian
('envelope': the derivative of kappa at the parameter the search returns, obtg_curvature_true_min_jac); the other rows and
their Jacobians are the same in all three solves.  Printed: tf, iterations and trueCurvatureRange at each solution.

    python examples/example19_curvature_bound.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

MAX_CURVATURE = 0.4          # a turning radius of 2.5


def problem(max_curvature=None):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=10, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5, maxAngRate=1,
                           initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)], initSpeeds=[1] * numVeh,
                           finalSpeeds=[1] * numVeh, initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2],
                           angRateRows='true_min', maxCurvature=max_curvature)


def solve(max_curvature=None, method='envelope', x0=None, ftol=1e-9, maxiter=500):
    """(BezOptimization, SciPy result): the solve with the angular-rate rows and, with max_curvature, the curvature rows under
    their `method` Jacobian, from x0 (None: the straight-line guess)"""
    bo = problem(max_curvature)
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method='envelope')},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
    if max_curvature is not None:
        cons.append({'type': 'ineq', 'fun': bo.maxCurvatureConstraints,
                     'jac': lambda x: bo.maxCurvatureJacobian(x, method=method)})
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0) if x0 is None else x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def report(name, bo, res):
    k_min, t_min, k_max, t_max = bo.trueCurvatureRange(res.x)
    print("%-34s tf* = %.9f (%d iterations, SLSQP status %d)" % (name, res.fun, res.nit, res.status))
    for v in range(bo.model['numVeh']):
        print("   vehicle %d: curvature in [%+.6f at t = %.4f, %+.6f at t = %.4f]" % (v, k_min[v], t_min[v], k_max[v], t_max[v]))


if __name__ == "__main__":
    bo, res = solve()
    report("maxAngRate alone:", bo, res)
    for method in ('fd', 'envelope'):
        report("maxCurvature = %.2f, %r:" % (MAX_CURVATURE, method), *solve(MAX_CURVATURE, method, x0=res.x))
