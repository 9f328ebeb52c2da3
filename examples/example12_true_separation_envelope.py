#!/usr/bin/env python3
"""example10's swarm with the true-minimum separation rows, solved twice from the same start: with the finite-difference
Jacobian (method='fd': n_x + 1 rows of branch-and-bound searches per iteration) and with the envelope Jacobian
(method='envelope': the derivative of each pair's squared-separation polynomial at the minimiser the search returns,
values and Jacobian from ONE launch at x).

    python examples/example12_true_separation_envelope.py
"""
import os
import sys
import time

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402


def solve(method, max_sep=1.0, tf=10.0):
    bo = BezOptimization(numVeh=3, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=max_sep, tf=tf,
                         initPoints=[(0.0, 0.0), (0.0, 4.0), (3.0, -1.0)], finalPoints=[(6.0, 4.0), (6.0, 0.0), (3.0, 5.0)],
                         separationRows='true_min')
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method=method)}]
    x0 = bo.generateGuess(std=0.3, seed=2)
    bo.temporalSeparationJacobian(x0, method=method)          # the first call loads the kernels: not part of the solve
    ctx = bo._ctx(False)
    ctx.set_profiling(True)
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    res = sop.minimize(bo.objectiveFunction, x0=x0, method='SLSQP', constraints=cons,
                       options={'maxiter': 300, 'ftol': 1e-10, 'disp': False})
    wall = time.perf_counter() - t0
    launches = sum(n for _, n in ctx.kernel_stats().values())
    ctx.set_profiling(False)
    val, t_star = bo.trueMinSeparation(res.x)
    print("method=%r: path length %.9f, %d iterations (SLSQP status %d), %d launches, %.1f ms"
          % (method, res.fun, res.nit, res.status, launches, 1e3 * wall))
    for (i, j), v, t in zip([(0, 1), (0, 2), (1, 2)], val, t_star):
        print("   vehicles %d and %d: closest at t = %6.3f s, separation %.6f (bound %.1f)"
              % (i, j, t * tf, np.sqrt(max(v + max_sep ** 2, 0.0)), max_sep))
    return res


if __name__ == "__main__":
    a = solve('fd')
    b = solve('envelope')
    print("path length with the finite-difference Jacobian %.9f, with the envelope Jacobian %.9f (relative gap %.2e)"
          % (a.fun, b.fun, abs(a.fun - b.fun) / abs(a.fun)))
