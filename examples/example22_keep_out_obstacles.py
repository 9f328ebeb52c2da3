#!/usr/bin/env python3
"""Example1's time-optimal problem (two Dubins cars, maxSpeed 5, start and end speed 1, maxAngRate 1, maxSep 1) with a
KEEP-OUT obstacle: a square, 1 wide, that sits on the straight line between car 0's two end points
(BezOptimization(keepOut=..), keepOutConstraints).  Without it car 0 drives through the square -- the example prints how
deep.

A convex obstacle is the set {p : a_f . p <= b_f}; a car's row is the least over its trajectory of
G(t) = max_f (a_f . c(t) - b_f): positive outside (with unit normals at most the true distance: equal where the nearest
feature is a face, smaller near a corner), minus the penetration depth inside -- so a start that drives through the square
still has a gradient that pushes it out, which the Euclidean distance (0 inside) has not.  Solved three ways, at degree 5:

  1. without the obstacle (Example1 as it is);
  2. with keepOut and the finite-difference Jacobian (one batched call per Jacobian), from solve 1's solution;
  3. with keepOut and the envelope Jacobian (obtg_keep_out_true_min_jac: one face at an end or a smooth minimum, the
     weighted pair of faces at a kink -- DESIGN.md 4.24), from the same start.

For every solve it prints tf, the iterations, the smallest clearance and, beside it, Bezier.minDist2Poly (the true distance
to the square; 0 inside) of car 0's final curve.

Measured on the MI355X at ftol = 1e-10: without the obstacle tf = 2.896326733 (15 iterations), car 0 0.370 deep in the
square (car 1 0.142).  With keepOut, from that infeasible point: 'fd' tf = 4.134170344 in 11 iterations, 'envelope' the same tf
in 10; car 0's clearance 0 at t = 0.635 on a kink (two faces, weights 0.957 and 0.043), minDist2Poly 0.000000 beside it.

    python examples/example22_keep_out_obstacles.py
"""
import os
import sys

import numpy as np
import scipy.optimize as sop

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd import bezier  # noqa: E402
from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization  # noqa: E402

INIT, FINAL = [(0, 5), (3, 0)], [(8, 4), (7, 10)]
CENTRE = (4.0, 4.3)          # car 0's chord passes y = 4.5 at x = 4: through the square, 0.2 off its centre
HALF = 0.5


def square(centre=CENTRE, half=HALF):
    """the square's vertices, counter-clockwise"""
    cx, cy = centre
    return [(cx - half, cy - half), (cx + half, cy - half), (cx + half, cy + half), (cx - half, cy + half)]


def obstacles():
    return [bezier.halfspacesOfPolygon(square())]


def problem(degree=5, keep_out=None, margin=0.0):
    numVeh = 2
    return BezOptimization(numVeh=numVeh, dimension=2, degree=degree, minimizeGoal='TimeOpt', maxSep=1, maxSpeed=5,
                           maxAngRate=1, initPoints=INIT, finalPoints=FINAL, initSpeeds=[1] * numVeh, finalSpeeds=[1] * numVeh,
                           initAngs=[0, np.pi / 2], finalAngs=[0, np.pi / 2], keepOut=keep_out, keepOutMargin=margin)


def solve(method=None, degree=5, x0=None, ftol=1e-10, maxiter=1000):
    """(BezOptimization, SciPy result): method None -- no obstacle; 'fd' / 'envelope' -- with the square and that Jacobian of
    its rows, from x0 (None: the straight-line guess); the other constraints are the same in every solve"""
    bo = problem(degree, None if method is None else obstacles())
    cons = [{'type': 'ineq', 'fun': bo.temporalSeparationConstraints,
             'jac': lambda x: bo.temporalSeparationJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxSpeedConstraints, 'jac': lambda x: bo.maxSpeedJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': bo.maxAngularRateConstraints, 'jac': lambda x: bo.maxAngularRateJacobian(x, method='exact')},
            {'type': 'ineq', 'fun': lambda x: x[-1:], 'jac': lambda x: np.eye(1, x.size, x.size - 1)}]
    if method is not None:
        cons.append({'type': 'ineq', 'fun': bo.keepOutConstraints, 'jac': lambda x: bo.keepOutJacobian(x, method=method)})
    res = sop.minimize(bo.objectiveFunction, x0=bo.generateGuess(std=0) if x0 is None else x0, method='SLSQP', constraints=cons,
                       jac=lambda x: bo.objectiveGradient(x, method='exact'), options={'maxiter': maxiter, 'ftol': ftol, 'disp': False})
    return bo, res


def clearances(x, degree=5):
    """dict(val[2], t_star[2], face[2][2], lam[2], status[2]) of the square at x, whatever the solve was: one row per car"""
    return problem(degree, obstacles()).trueKeepOutClearances(x)


def distances(x, degree=5):
    """[2]: per car the true distance of its curve to the square (Bezier.minDist2Poly, robust; 0 inside)"""
    bo = problem(degree)
    Y = bo.reshapeVector(np.asarray(x, dtype=float))
    poly = np.array([(px, py, 0.0) for px, py in square()])
    return np.array([bezier.Bezier(Y[2 * v:2 * v + 2]).minDist2Poly(poly, robust=True)[0] for v in range(2)])


def report(name, res, degree=5):
    c = clearances(res.x, degree)
    d = distances(res.x, degree)
    print("%-26s tf* = %.9f (%d iterations, SLSQP status %d); smallest clearance %.6f" % (name, res.fun, res.nit, res.status, c['val'].min()))
    for v in range(2):
        print("   car %d: clearance %.6f at t = %.4f (faces %s, weight %.4f); minDist2Poly %.6f"
              % (v, c['val'][v], c['t_star'][v], c['face'][v].tolist(), c['lam'][v], d[v]))


if __name__ == "__main__":
    _, free = solve(None)
    print("without the obstacle car 0 is %.6f deep in the square" % -clearances(free.x)['val'][0])
    _, fd = solve('fd', x0=free.x)
    _, env = solve('envelope', x0=free.x)
    report("no obstacle", free)
    report("keepOut, 'fd'", fd)
    report("keepOut, 'envelope'", env)
