#!/usr/bin/env python3
"""Example1's two Dubins cars (Examples/Example1_DubinsCarTimeOptimal.py:94-148) on a fixed final time, solved twice: once
minimising the length of the control polygon (`minGoal='euclidean'`, the reference's goal, optimization.py:462-489) and once
minimising the length of the curves themselves (`minGoal='arcLength'`, obtg_arc_length_obj) with the exact gradient from the
device as SLSQP's `jac`.  For both solutions it prints the control-polygon length and the true length.

    python examples/example18_arc_length.py

The polygon bounds the curve from above, so the first number of a row is never below the second.  Forward differences of
the arc-length goal would divide the quadrature's tolerance by SciPy's step of 1.5e-8: the goal is meant to be used with
`objectiveGradient(method='exact')`.
"""
import os
import sys
import time

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization


def solve(goal):
    numVeh, dim, deg = 2, 2, 10
    bezopt = BezOptimization(numVeh=numVeh, dimension=dim, degree=deg, minimizeGoal=goal, maxSep=1, maxSpeed=5, maxAngRate=1,
                             tf=12.0, initPoints=[(0, 5), (3, 0)], finalPoints=[(8, 4), (7, 10)], initSpeeds=[1] * numVeh,
                             finalSpeeds=[1] * numVeh, initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2])
    cons = [{'type': 'ineq', 'fun': bezopt.temporalSeparationConstraints, 'jac': bezopt.temporalSeparationJacobian},
            {'type': 'ineq', 'fun': bezopt.maxSpeedConstraints, 'jac': bezopt.maxSpeedJacobian},
            {'type': 'ineq', 'fun': bezopt.maxAngularRateConstraints, 'jac': bezopt.maxAngularRateJacobian}]
    t0 = time.time()
    res = sop.minimize(bezopt.objectiveFunction, x0=bezopt.generateGuess(std=0), method='SLSQP', constraints=cons,
                       jac=lambda x: bezopt.objectiveGradient(x, method='exact'), options={'maxiter': 250, 'disp': False})
    polygon = float(bezopt._ctx(False).euclidean_obj(bezopt.reshapeVector(res.x))[0])
    true = bezopt.trueArcLengths(res.x)
    print("minGoal=%-10s status %d, nit %3d, %.2f s:  control polygon %.9f   true length %.9f  (per vehicle %s)"
          % (goal, res.status, res.nit, time.time() - t0, polygon, float(true.sum()), np.array2string(true, precision=6)))
    return polygon, float(true.sum())


def main():
    poly_e, true_e = solve('euclidean')
    poly_a, true_a = solve('arcLength')
    print("true length: %.9f (euclidean goal)  ->  %.9f (arcLength goal)" % (true_e, true_a))


if __name__ == '__main__':
    main()
