#!/usr/bin/env python3
"""Staggered departures in the sequential planner: the same crowded volume planned twice, once with every vehicle in the
air over the same interval and once with one departure every few seconds.

    python examples/example11_staggered_departures.py [numVeh] [seconds between departures]

The vehicles start within a 30 x 30 patch of the z = 0 face and climb to targets within the same patch of the z = volume
face (3-D, degree 3, dsafe 2.5: the crowded case of the planner's test).  Each is planned by SLSQP against ALL
trajectories fixed so far (`pairing='new_vs_all'`, one-call Jacobian).  With `Parameters(..., t0s=, tfs=)` a pair is
held apart only while both vehicles fly: the constraint runs on the overlap of their two spans, as the reference's
`Bezier.sub` does through `_temporalAlignment` (bezier.py:347-374, 903-941) -- obtg_one_vs_many_min_spans on the device --
and two vehicles that are never in the air together do not constrain each other at all.  Printed: how many vehicles
converge with and without the stagger, the worst margin of the converged ones, and the time.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalbeziertrajectorygeneration_amd import sequential as SS  # noqa: E402


def main():
    nveh = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    gap = float(sys.argv[2]) if len(sys.argv) > 2 else 2.5
    NDIM, DEG, VOLUME, DSAFE, FLIGHT = 3, 3, 100.0, 2.5, 10.0
    rng = np.random.default_rng(2)
    fin = VOLUME * np.concatenate([0.35 + 0.3 * rng.random((nveh, 2)), np.ones((nveh, 1))], axis=1)
    ini = 35.0 + 30.0 * rng.random((nveh, 2))
    t0s = gap * np.arange(nveh)
    for label, spans in (("one interval for all", {}), ("a departure every %g s" % gap, dict(t0s=t0s, tfs=t0s + FLIGHT))):
        params = SS.Parameters(nveh, NDIM, DEG, VOLUME, DSAFE, finalpts=fin, seed=4, **spans)
        params.inipts[:, :2] = ini
        traj, results, dt = SS.plan(params, pairing='new_vs_all', with_jac=True)
        ok = np.array([r.success for r in results])
        sp = None if params.t0s is None else np.stack([params.t0s, params.tfs], axis=1)
        worst, together = np.inf, 0
        for i in range(1, nveh):
            kw = {} if sp is None else dict(spans=sp[:i], new_span=sp[i])
            c = SS.new_vs_all(traj[NDIM * i:NDIM * (i + 1)], traj[:NDIM * i], NDIM, DSAFE, **kw)[0]
            together += int((c != SS.NO_OVERLAP).sum()) if sp is not None else i
            if ok[i]:
                worst = min(worst, float(c.min()))
        print('%-26s %3d of %3d vehicles converged in %6.2f s (%d SLSQP iterations); %d of %d pairs share the air; worst '
              'margin of a converged vehicle %+.3e' % (label, int(ok.sum()), nveh, dt, sum(r.nit for r in results), together,
                                                       nveh * (nveh - 1) // 2, worst))


if __name__ == '__main__':
    main()
