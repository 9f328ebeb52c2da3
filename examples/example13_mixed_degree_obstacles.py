#!/usr/bin/env python3
"""The flow of Examples/ComplexObstacles.py:19-63 with a vehicle whose degree is NOT the tracks': one Dubins-like vehicle of
degree 5, time optimal, against the two degree-10 Bezier "tracks" as shapeObstacles -- the ordinary case of a low-order
vehicle steered past boundaries drawn in detail.  `_minDist` (bezier.py:1283-1408) takes any two degrees; on the device that
is obtg_min_dist_mixed (one launch for the constraint, one for its Jacobian).

    python examples/example13_mixed_degree_obstacles.py [--robust]

As in example4_complex_obstacles.py: the distance column of spatialSeparationConstraints goes to SLSQP with
spatialSeparationJacobian(column=0) as its `jac`; only tf is bounded below; a pair on which the reference's search does not
end raises from the closure, and the script then goes on with the robust search (--robust takes it from the start), which on
unequal degrees elevates the lower curve to the other's degree first.  It ends with the vehicle's minDist to each track.
"""
import os
import sys
import time

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optimalbeziertrajectorygeneration_amd.bezier as bez  # was: import bezier as bez
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # was: from optimization import ...


def solve(robust):
    track1 = bez.Bezier(np.array([[8, 9, 10, 11, 12, 13, 12, 11, 10, 9, 8],
                                  [8, 10, 12, 14, 20, 14, 12, 10, 10, 9, 8]], dtype=float))
    track2 = bez.Bezier(np.array([[18, 13, 9, 6, 4, 3, 4, 6, 9, 13, 18],
                                  [3, 3, 4, 4, 4, 5, 5, 5, 7, 8, 3]], dtype=float))
    bezopt = BezOptimization(numVeh=1, dimension=2, degree=5, minimizeGoal='TimeOpt', maxSep=0.5, maxSpeed=5,
                             maxAngRate=0.5, initPoints=(2, 1), finalPoints=(15, 15), initSpeeds=1, finalSpeeds=1,
                             initAngs=np.pi / 2, finalAngs=np.pi / 2, shapeObstacles=[track1, track2])
    xGuess = bezopt.generateGuess()
    xGuess[-1] = 10
    lb = np.full(xGuess.size, -np.inf)
    lb[-1] = 1e-3
    bounds = sop.Bounds(lb, np.inf)
    ineqCons = [{'type': 'ineq', 'fun': bezopt.maxSpeedConstraints, 'jac': bezopt.maxSpeedJacobian},
                {'type': 'ineq', 'fun': bezopt.maxAngularRateConstraints, 'jac': bezopt.maxAngularRateJacobian},
                {'type': 'ineq', 'fun': lambda x: bezopt.spatialSeparationConstraints(x, robust=robust)[:, 0],
                 'jac': lambda x: bezopt.spatialSeparationJacobian(x, robust=robust, column=0)}]
    t0 = time.time()
    res = sop.minimize(bezopt.objectiveFunction, x0=xGuess, method='SLSQP', constraints=ineqCons, bounds=bounds,
                       options={'maxiter': 250, 'disp': False})
    dt = time.time() - t0
    print('%s search: tf* = %.6f, %d iterations, success %s, %.2f s'
          % ('robust' if robust else "reference's", res.x[-1], res.nit, res.success, dt))
    vehicle = bez.Bezier(bezopt.reshapeVector(res.x)[:2])
    for name, track in (('track1', track1), ('track2', track2)):
        d, t1, t2 = vehicle.minDist(track, robust=robust)
        print('  degree-%d vehicle to degree-%d %s: minDist %.6f at t1 = %.4f, t2 = %.4f' % (vehicle.deg, track.deg, name, d, t1, t2))


def main():
    if "--robust" not in sys.argv:
        try:
            return solve(False)
        except (RuntimeError, RecursionError) as e:
            print("reference's search: %s -> switching to the robust search" % e)
    solve(True)


if __name__ == '__main__':
    main()
