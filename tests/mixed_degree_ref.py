"""Seeded inputs of the mixed-degree `_minDist` tests and the oracle's answers on them (test infrastructure, no test in here).

A group is N pairs of curves with (KA, KB) control points: curve k of the first set against curve k of the second.  The curves
are random walks of one extent at every degree, so that pairs cross now and then: a crossing pair runs the reference's search
into its budgets (about 18 % of the reference's sampled pairs do not terminate), and such a pair is compared by
status and counts only.  `apart` moves the second set away so that every search ends.

    python tests/mixed_degree_ref.py        prints the share of MD_OK pairs of every group (how the seeds were chosen)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_PAIRS = 200
EPS, MAX_DEPTH, MAX_NODES = 1e-9, 40, 3000        # one budget on both sides, small enough that the oracle takes a second or two

# (name, KA, KB, dim of the first set, dim of the second set, apart, seed)
GROUPS = [(("%s_%d_%d" % (kind, ka, kb)), ka, kb, dim, dim, 0.0, seed)
          for kind, dim, seeds in (("planar", 2, (11, 12, 13, 14, 15, 16, 17)), ("space", 3, (21, 22, 23, 24, 25, 26, 27)))
          for (ka, kb), seed in zip(((3, 11), (11, 3), (6, 11), (11, 16), (2, 32), (17, 5), (32, 31)), seeds)]
GROUPS.append(("planar_vs_space_6_11", 6, 11, 2, 3, 0.0, 31))
GROUPS.append(("apart_6_11", 6, 11, 3, 3, 40.0, 32))          # hulls apart: every search ends (the all-OK group)
GROUP_NAMES = [g[0] for g in GROUPS]


def walk(rng, n, K, dim, shift):
    c = np.zeros((n, 3, K))
    c[:, :dim] = rng.uniform(0.0, 6.0, size=(n, dim, 1)) + np.cumsum(rng.normal(0.0, 4.0 / np.sqrt(K), size=(n, dim, K)), axis=2)
    c[:, 0] += shift
    return c


def group(name):
    """-> (curves: list of 2 N padded [3][K] arrays, pa, pb)"""
    _, ka, kb, da, db, apart, seed = GROUPS[GROUP_NAMES.index(name)]
    rng = np.random.default_rng(seed)
    a, b = walk(rng, N_PAIRS, ka, da, 0.0), walk(rng, N_PAIRS, kb, db, apart)
    return list(a) + list(b), np.arange(N_PAIRS, dtype=np.int32), np.arange(N_PAIRS, 2 * N_PAIRS, dtype=np.int32)


def oracle_pairs(O, curves, pa, pb, eps=EPS, max_depth=MAX_DEPTH, max_nodes=MAX_NODES):
    """oracle.min_dist on every pair -> dict of arrays, as Context.min_dist_mixed returns them"""
    out = [O.min_dist(curves[a], curves[b], eps=eps, max_depth=max_depth, max_nodes=max_nodes) for a, b in zip(pa, pb)]
    return dict(res=np.array([o["res"] for o in out]), nodes=np.array([o["nodes"] for o in out]),
                gjk_calls=np.array([o["gjk_calls"] for o in out]), depth=np.array([o["depth"] for o in out]),
                status=np.array([o["status"] for o in out], np.int32))


_memo = {}


def oracle_group(O, name):
    """The oracle's answers on a group, computed once per session and shared (callers must not write into them)."""
    if name not in _memo:
        _memo[name] = oracle_pairs(O, *group(name))
    return _memo[name]


if __name__ == "__main__":
    import time
    from oracle import oracle as O
    O.build()
    for g in GROUPS:
        t0 = time.time()
        o = oracle_group(O, g[0])
        print("%-22s seed %3d: MD_OK %5.1f %%, statuses %s, most nodes %d, %.2f s" % (
            g[0], g[6], 100.0 * (o["status"] == 0).mean(), np.bincount(o["status"], minlength=4), o["nodes"].max(), time.time() - t0))
