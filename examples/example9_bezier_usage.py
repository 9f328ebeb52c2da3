#!/usr/bin/env python3
"""The four sections of Examples/BezierUsageExamples.py on the MI355X path, printing instead of plotting:
minimum distance between two curves, between a curve and a polygon, collision check between two curves
(`Bezier.collCheck`, bezier.py:859-862 -> `_collCheckBez2Bez`, :1561-1614) and between a curve and a polygon
(`Bezier.collCheck2Poly`, bezier.py:864-867 -> `_collCheckBez2Poly`, :1617-1651).

    python examples/example9_bezier_usage.py

Section 4 (`c1.collCheck2Poly(poly2)`) is a call the reference itself does not come back from: the method raises once its
node budget is spent, the batched call reports the status, and `robust=True` answers the question from the true minimum
distance (NOT the reference's value).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optimalbeziertrajectorygeneration_amd.bezier as bez  # was: import bezier as bez
from optimalbeziertrajectorygeneration_amd import _capi


def curves_and_polys():
    cpts1 = np.array([(0, 1, 2, 3, 4, 5), (1, 2, 0, 0, 2, 1), (0, 1, 2, 3, 4, 5)], dtype=float)
    cpts2 = np.array([(0, 1, 2, 3, 4, 5), (3, 2, 0, 0, 2, 3), (5, 4, 3, 2, 1, 0)], dtype=float)
    cpts3 = np.array([(0, 1, 2, 3, 4, 5), (0, 1, 2, 3, 4, 5), (0, 0, 0, 0, 0, 0)], dtype=float)
    cpts4 = np.array([(5, 4, 3, 2, 1, 0), (0, 1, 2, 3, 4, 5), (0, 0, 0, 0, 0, 0)], dtype=float)
    poly1 = np.array([(1, 1, 3), (1, 1, 2), (1, 2, 1), (3, 1, 3), (1, 3, 1)], dtype=float)
    poly2 = np.array([(1, 1, 3), (1, 1, 2), (1, 2, 1), (3, -1, 3), (1, 3, 1)], dtype=float)
    return [cpts1, cpts2, cpts3, cpts4], [poly1, poly2]


def verdict(v, what):
    return ('No collision detected between ' if v == 1 else 'Collision detected between ') + what


def main(budget=20000):
    cpts, (poly1, poly2) = curves_and_polys()
    c1, c2, c3, c4 = [bez.Bezier(c) for c in cpts]
    out = {}
    # 1 - minimum distance between curves
    out['dist12'], t1, t2 = c1.minDist(c2)
    print('The minimum distance between C1 and C2 is {}'.format(out['dist12']))
    # 2 - minimum distance between a curve and a polygon
    out['dist1p1'], t1p, pt1 = c1.minDist2Poly(poly1)
    print('The minimum distance between C1 and Poly1 is {}'.format(out['dist1p1']))
    # 3 - collision detection between two curves
    out['collCheck34'] = c3.collCheck(c4)
    print(verdict(out['collCheck34'], 'C3 and C4') + ' (collCheck returned {!r})'.format(out['collCheck34']))
    # 4 - collision detection between a curve and a polygon
    try:
        out['collCheck1p2'] = c1.collCheck2Poly(poly2, max_nodes=budget)
        print(verdict(out['collCheck1p2'], 'C1 and Poly2'))
    except RuntimeError as e:
        out['collCheck1p2'] = None
        print('C1 and Poly2: {}'.format(e))
    r = _capi.scratch_context().coll_check2poly(c1._padded()[None], poly2, [0, len(poly2)], [0], [0], max_nodes=budget)
    out['status1p2'] = int(r['status'][0])
    print('  batched call: status {} (1 = node budget) after {} gjkNew calls, depth {}'.format(
        out['status1p2'], int(r['gjk_calls'][0]), int(r['depth'][0])))
    out['robust'] = dict(c3c4=c3.collCheck(c4, robust=True), c1c2=c1.collCheck(c2, robust=True),
                         c1p1=c1.collCheck2Poly(poly1, robust=True), c1p2=c1.collCheck2Poly(poly2, robust=True))
    print('  robust=True: ' + verdict(out['robust']['c1p2'], 'C1 and Poly2') +
          ' (true distance to the polygon\'s hull {:.6g})'.format(c1.minDist2Poly(poly2, robust=True)[0]))
    print('  robust=True, the other three: C3/C4 {c3c4}, C1/C2 {c1c2}, C1/Poly1 {c1p1} (1 = no collision)'.format(**out['robust']))
    return out


if __name__ == '__main__':
    main()
