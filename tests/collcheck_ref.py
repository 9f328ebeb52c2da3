"""The reference's two collision checks restated over the CPU oracle's primitives.

`_collCheckBez2Bez` (bezier.py:1561-1614) and `_collCheckBez2Poly` (bezier.py:1617-1651) as explicit recursions on
`oracle.gjk` (gjkNew's flag) and `oracle.split` (deCasteljauSplit at 0.5), with what the device entry points add: a node
budget and a status.  A search stops with MD_GJK_CAP at the first gjkNew call that does not return (the oracle's
ST_MD_CAP / ST_CYCLE: the reference loops forever there; ST_MAXITER is a return, flag -1, as in the reference) and with
MD_NODE_CAP when `max_nodes` nodes have been visited.  A node is a call that passes the reference's `cnt > 100` test;
every node makes exactly one gjkNew call.  tests/test_collcheck_ref.py holds this file to the reference's recorded
values and call counts (tests/test_collcheck_cases_ref.py: on non-finite input, 13 control points and deep 3-D walks too);
tests/test_gpu_collcheck.py and tests/test_gpu_collcheck_forms.py hold the device to this file.

-> dict(res, nodes, gjk_calls, depth, status); res is 0.0 beside a status other than MD_OK.
"""
import math
import sys

import numpy as np

from oracle import oracle

MD_OK, MD_NODE_CAP, MD_GJK_CAP = oracle.MD_OK, oracle.MD_NODE_CAP, oracle.MD_GJK_CAP


class _Stop(Exception):
    pass


class _Search:
    def __init__(self, max_iter, md_cap, max_nodes):
        self.max_iter, self.md_cap, self.max_nodes = max_iter, md_cap, max_nodes
        self.nodes = self.calls = self.depth = 0
        self.status = MD_OK

    def enter(self, cnt):
        if self.nodes >= self.max_nodes:
            self.status = MD_NODE_CAP
            raise _Stop()
        self.nodes += 1
        self.depth = max(self.depth, cnt)

    def flag(self, p1, p2):
        self.calls += 1
        g = oracle.gjk(p1, p2, max_iter=self.max_iter, md_cap=self.md_cap, trace_cap=0)
        if g["status"] in (oracle.ST_MD_CAP, oracle.ST_CYCLE):
            self.status = MD_GJK_CAP
            raise _Stop()
        return g["flag"]

    def result(self, fn):
        limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(limit, 1000))
        try:
            res = float(fn())
        except _Stop:
            res = 0.0
        finally:
            sys.setrecursionlimit(limit)
        return dict(res=res, nodes=self.nodes, gjk_calls=self.calls, depth=self.depth, status=self.status)


def pad3(cpts):
    """[dim][K] -> [3][K] with a zero z row (bezier.py:1567-1580)."""
    cpts = np.atleast_2d(np.asarray(cpts, dtype=np.float64))
    out = np.zeros((3, cpts.shape[1]))
    out[:cpts.shape[0]] = cpts
    return out


def upperbound(c1, c2):
    """_upperbound (bezier.py:1499-1541): the smallest of the four end-point distances, `norm` summed left to right."""
    def norm(a, b):
        s = 0.0
        with np.errstate(invalid="ignore"):          # inf - inf of a non-finite control point: NaN, as in the reference
            for v in a - b:
                s += v * v
        return math.sqrt(s)
    d = np.array([norm(c1[:, 0], c2[:, 0]), norm(c1[:, 0], c2[:, -1]), norm(c1[:, -1], c2[:, 0]), norm(c1[:, -1], c2[:, -1])])
    return float(d[int(np.argmin(d))])


def _py_min(a, b):
    """Python's min(a, b): b only when b < a."""
    return b if b < a else a


def coll_check(c1, c2, eps=1e-9, max_iter=128, md_cap=4096, max_nodes=200000):
    s = _Search(max_iter, md_cap, max_nodes)

    def rec(a, b, cnt, alpha):
        cnt += 1
        if cnt > 100:
            return -1.0
        s.enter(cnt)
        ub = upperbound(a, b)
        if s.flag(a.T, b.T) > 0:
            return 1.0
        if ub <= alpha:
            alpha = ub
        if 0.0 >= alpha * (1 - eps):
            return alpha
        a3, a4 = oracle.split(a, 0.5)
        b5, b6 = oracle.split(b, 0.5)
        for x, y in ((a3, b5), (a3, b6), (a4, b5), (a4, b6)):
            alpha = _py_min(alpha, rec(x, y, cnt, alpha))
        return alpha

    return s.result(lambda: rec(pad3(c1), pad3(c2), 0, math.inf))


def coll_check2poly(c1, poly, max_iter=128, md_cap=4096, max_nodes=200000):
    s = _Search(max_iter, md_cap, max_nodes)
    poly = np.ascontiguousarray(poly, dtype=np.float64).reshape(-1, 3)

    def rec(a, cnt):
        cnt += 1
        if cnt > 100:
            return -1.0
        s.enter(cnt)
        if s.flag(a.T, poly) > 0:
            return 1.0
        a3, a4 = oracle.split(a, 0.5)
        if rec(a3, cnt) == 1 and rec(a4, cnt) == 1:
            return 1.0
        return 0.0

    return s.result(lambda: rec(pad3(c1), 0))


def coll_check_pairs(curves, pair_a, pair_b, **kw):
    """Every pair of curves[n][3][K]: arrays res, nodes, gjk_calls, depth, status."""
    rs = [coll_check(curves[a], curves[b], **kw) for a, b in zip(pair_a, pair_b)]
    return _stack(rs)


def coll_check2poly_pairs(curves, pts, off, pair_curve, pair_poly, **kw):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    rs = [coll_check2poly(curves[c], pts[off[p]:off[p + 1]], **kw) for c, p in zip(pair_curve, pair_poly)]
    return _stack(rs)


def _stack(rs):
    return dict(res=np.array([r["res"] for r in rs], dtype=np.float64),
                nodes=np.array([r["nodes"] for r in rs], dtype=np.int32),
                gjk_calls=np.array([r["gjk_calls"] for r in rs], dtype=np.int32),
                depth=np.array([r["depth"] for r in rs], dtype=np.int32),
                status=np.array([r["status"] for r in rs], dtype=np.int32))
