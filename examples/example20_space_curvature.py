#!/usr/bin/env python3
"""Example2's crossing swarm in space at a small size (3 vehicles, degree 5), time-optimal under a speed bound, solved without
a turning limit and with maxSpaceCurvature -- a fixed-wing vehicle's minimum turn radius of 1 / maxSpaceCurvature, which
neither the speed nor the acceleration rows express and which does not move with tf.

The space-curvature rows (maxSpaceCurvature=..., obtg_space_curvature_true_min: per vehicle maxSpaceCurvature minus the true
maximum over the path of |c' x c''| / |c'|^3) are solved twice, with the forward-difference Jacobian of the rows ('fd': the
search differenced, one batched call) and with their envelope Jacobian ('envelope': the derivative of kappa at the parameter
the search returns, obtg_space_curvature_true_min_jac); the other rows and their Jacobians are the same in all three solves.
The bound is 3/4 of the unbounded solution's largest curvature, so it is active (on this swarm the tighter turn costs no
time: the vehicle that turns hardest reshapes its path at the same tf).  Printed: tf, iterations and
trueSpaceCurvatureMax at each solution.

    python examples/example20_space_curvature.py [numVeh]
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402
from example2_swarm_3d import crossing_swarm  # noqa: E402


def problem(numVeh, max_curvature=None):
    init, final = crossing_swarm(numVeh)
    return BezOptimization(numVeh=numVeh, dimension=3, degree=5, minimizeGoal='TimeOpt', maxSep=0.9, maxSpeed=3.0,
                           initPoints=init, finalPoints=final, tf=8.0, maxSpaceCurvature=max_curvature)


def solve(numVeh=3, max_curvature=None, method='envelope', x0=None, ftol=1e-9, maxiter=400):
    """(BezOptimization, SciPy result): the solve with the separation and speed rows and, with max_curvature, the
    space-curvature rows under their `method` Jacobian, from x0 (None: the straight lines plus N(0, 0.2) noise, seed 2)"""
    bo = problem(numVeh, max_curvature)
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints, 'jac': bo.temporalSeparationJacobian},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': bo.maxSpeedJacobian},
            {'type': 'ineq', 'fun': lambda x: x[-1:] - 0.1, 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
    if max_curvature is not None:
        cons.append({'type': 'ineq', 'fun': bo.maxSpaceCurvatureConstraints,
                     'jac': lambda x: bo.maxSpaceCurvatureJacobian(x, method=method)})
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0.2, seed=2) if x0 is None else x0, method='SLSQP',
                       constraints=cons, options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def report(name, bo, res):
    k_max, t_max = bo.trueSpaceCurvatureMax(res.x)
    print("%-40s tf* = %.9f (%d iterations, SLSQP status %d)" % (name, res.fun, res.nit, res.status))
    for v in range(bo.model['numVeh']):
        print("   vehicle %d: largest curvature %.6f at t = %.4f" % (v, k_max[v], t_max[v]))
    return k_max.max()


if __name__ == "__main__":
    numVeh = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    bo, res = solve(numVeh)
    bound = round(0.75 * report("no turning limit:", bo, res), 3)
    for method in ('fd', 'envelope'):
        report("maxSpaceCurvature = %.3f, %r:" % (bound, method), *solve(numVeh, bound, method, x0=res.x))
