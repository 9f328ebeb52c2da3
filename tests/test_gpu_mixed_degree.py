"""obtg_min_dist_mixed (`_minDist`, bezier.py:1283-1408, on curves of different degree) on the MI355X: against the CPU oracle
bit for bit, against the reference's own results (tests/golden/mixed_degree.npz), and through Bezier.minDist and
BezOptimization's spatial-separation calls."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixed_degree_ref as R  # noqa: E402
from util import assert_identical  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUDGET = dict(eps=R.EPS, max_depth=R.MAX_DEPTH, max_nodes=R.MAX_NODES)


@pytest.fixture(scope="module")
def capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    return _capi


def _compare(r, o, what):
    """Per pair: status, node and gjkNew-call counts and the depth always; the result triple, bit for bit, where the search ended."""
    assert np.array_equal(r["status"], o["status"]), what
    assert np.array_equal(r["nodes"], o["nodes"]), what
    assert np.array_equal(r["gjk_calls"], o["gjk_calls"]), what
    assert np.array_equal(r["depth"], o["depth"]), what
    ok = o["status"] == 0
    assert_identical(r["res"][ok], o["res"][ok], what)
    return ok


@pytest.mark.parametrize("name", R.GROUP_NAMES)
def test_mixed_degree_is_the_oracle(capi, oracle, name):
    """200 seeded pairs per group, (KA, KB) = (3, 11), (11, 3), (6, 11), (11, 16), (2, 32), (17, 5), (32, 31), each planar and
    3-D, one group planar against 3-D and one with the hulls apart: the device's result triple equals the oracle's bit for bit,
    and its node count, gjkNew-call count, depth and status are the oracle's, under one budget (eps 1e-9, depth 40, 3000 nodes).
    A pair the oracle ends with a budget status is compared by status and counts only; such pairs may be at most half of a
    group.  Share of MD_OK pairs (python tests/mixed_degree_ref.py; the seeds are the first tried): planar 69.0, 65.5, 71.0,
    68.0, 85.0, 76.0, 65.0 %; 3-D 76.0, 75.0, 81.0, 83.5, 95.5, 85.5, 77.0 %; planar against 3-D 81.5 %; apart 100 % (up to
    2045 nodes a pair).  Every budget status (node cap, depth cap, an inner gjkNew that does not converge) occurs."""
    curves, pa, pb = R.group(name)
    o = R.oracle_group(oracle, name)
    r = capi.scratch_context().min_dist_mixed(curves, pa, pb, **BUDGET)
    ok = _compare(r, o, name)
    assert ok.mean() >= 0.5, "%s: only %.1f %% of the pairs are compared by value" % (name, 100 * ok.mean())
    if name.startswith("apart"):
        assert ok.all()


def test_one_call_with_several_degree_pairs(capi, oracle):
    """Pairs of different (KA, KB) in ONE call -- workers take them from one queue, with LDS and frame stack laid out for the
    largest KA + KB -- give per pair what a call with that pair alone gives (and what the oracle gives).  A second call of the
    same list hands the pairs out in the order of the first call's node counts: the same answers."""
    ctx = capi.scratch_context()
    curves, pa, pb, ref = [], [], [], []
    for name in ("planar_3_11", "space_32_31", "space_2_32", "planar_vs_space_6_11", "space_17_5", "apart_6_11"):
        c, a, b = R.group(name)
        o = R.oracle_group(oracle, name)
        for k in range(0, R.N_PAIRS, 8):
            pa.append(len(curves)); pb.append(len(curves) + 1)
            curves += [c[a[k]], c[b[k]]]
            ref.append({key: o[key][k] for key in o})
    o = {key: np.array([e[key] for e in ref]) for key in ref[0]}
    perm = np.random.default_rng(3).permutation(len(pa))                 # sizes interleaved in the queue
    pa, pb = np.array(pa)[perm], np.array(pb)[perm]
    o = {key: o[key][perm] for key in o}
    r = ctx.min_dist_mixed(curves, pa, pb, **BUDGET)
    _compare(r, o, "one call, several (KA, KB)")
    again = ctx.min_dist_mixed(curves, pa, pb, **BUDGET)                 # (ordered by the history of the first)
    for key in r:
        assert np.array_equal(r[key], again[key], equal_nan=(key == "res")), key
    for k in range(0, len(pa), 7):
        one = ctx.min_dist_mixed([curves[pa[k]], curves[pb[k]]], [0], [1], **BUDGET)
        for key in r:
            assert np.array_equal(one[key][0], r[key][k], equal_nan=(key == "res")), (key, k)


def test_equal_degrees_forward_to_min_dist(capi):
    """obtg_min_dist_mixed with every K_i equal is obtg_min_dist: the same res / info / status, planar and 3-D."""
    ctx = capi.scratch_context()
    for dim, K in ((2, 6), (3, 11), (3, 20)):
        rng = np.random.default_rng(40 + K)
        curves = R.walk(rng, 64, K, dim, 0.0)
        pa, pb = np.arange(0, 64, 2), np.arange(1, 64, 2)
        a = ctx.min_dist(curves, pa, pb, **BUDGET)
        b = ctx.min_dist_mixed(list(curves), pa, pb, **BUDGET)
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=(key == "res")), (K, key)


@pytest.mark.parametrize("dim,K", [(2, 6), (3, 20), (3, 22)])
def test_equal_degree_pairs_on_the_mixed_kernel(capi, monkeypatch, dim, K):
    """A call of equal-degree curves is forwarded to obtg_min_dist (above), so k_min_dist_mixed never sees KA == KB through it.
    Here one curve of another length (K = 3) that no pair names keeps the call on k_min_dist_mixed: all 28 pairs of 8 curves
    give what obtg_min_dist gives on the same curves in its one-wavefront and its one-lane form -- res (NaN equal to NaN),
    node and gjkNew-call counts, depth and status, no pair left out -- when the searches end, under a depth cap, and under a
    one-node budget.  K = 6 planar (hulls without a z row in the mixed kernel, with one in the others), K = 20 in 3-D (3 K <= 64:
    the level-parallel split), K = 22 in 3-D (3 K > 64: a lane per row)."""
    ctx = capi.scratch_context()
    rng = np.random.default_rng(600 + K)
    curves = R.walk(rng, 8, K, dim, 0.0)
    spare = R.walk(rng, 1, 3, dim, 0.0)[0]
    pa, pb = np.triu_indices(8, 1)
    for kw in (dict(max_depth=32, max_nodes=300), dict(max_depth=5, max_nodes=300), dict(max_depth=32, max_nodes=1)):
        mixed = ctx.min_dist_mixed(list(curves) + [spare], pa, pb, **kw)
        for form in ("wave", "lane"):
            monkeypatch.setenv("OBTG_MD_FORM", form)
            same = ctx.min_dist(curves, pa, pb, **kw)
            monkeypatch.delenv("OBTG_MD_FORM")
            for key in ("res", "nodes", "gjk_calls", "depth", "status"):
                assert np.array_equal(mixed[key], same[key], equal_nan=(key == "res")), (K, kw, form, key)


def test_mixed_degree_reference_fixture(capi, oracle, golden_dir):
    """The reference's own `_minDist` on curves of different degree (tests/golden/mixed_degree.npz: 3-D against 3-D and a 2-D
    first curve against a 3-D second one, degrees from {2, 4, 5, 10, 15}): the same triple, bit for bit, and the same number of
    gjkNew calls on every pair the reference returned from.  A pair it did not return from says nothing about the answer when
    the alarm ended it (fin 1: the reference may just be slow -- pair 50 ends after 23 373 gjkNew calls): there the device is
    held to the oracle's status and counts.  Where the reference overflowed its stack (fin 2: its recursion limit is 1000 and a
    level of `_minDist` is one frame of it, so the search went deeper than 64) the device reports a budget status."""
    m = np.load(os.path.join(golden_dir, "mixed_degree.npz"))
    off = m["off"]
    curves = [m["cpts"][3 * off[i]:3 * off[i + 1]].reshape(3, -1) for i in range(off.size - 1)]
    r = capi.scratch_context().min_dist_mixed(curves, m["pa"], m["pb"], max_depth=64, max_nodes=300000)
    fin = m["fin"] == 0
    assert fin.sum() >= 40
    for k in range(fin.size):
        if fin[k]:
            assert r["status"][k] == capi.MD_OK, k
            assert r["gjk_calls"][k] == m["calls"][k], k
            assert_identical(r["res"][k], m["res"][k], "fixture pair %d" % k)
        else:
            o = oracle.min_dist(curves[m["pa"][k]], curves[m["pb"][k]], max_depth=64, max_nodes=300000)
            assert (r["status"][k], r["nodes"][k], r["gjk_calls"][k], r["depth"][k]) == (o["status"], o["nodes"], o["gjk_calls"], o["depth"]), k
            if m["fin"][k] == 2:
                assert r["status"][k] != capi.MD_OK, k


def _deg5_deg10():
    from optimalbeziertrajectorygeneration_amd.bezier import Bezier
    c5 = Bezier(np.array([[0, 1, 2.5, 3, 4, 5.5], [1, 2.5, 0, 0.5, 2, 1]], dtype=float))
    c10 = Bezier(np.array([[8, 9, 10, 11, 12, 13, 12, 11, 10, 9, 8], [8, 10, 12, 14, 20, 14, 12, 10, 10, 9, 8]], dtype=float))
    return c5, c10


def test_bezier_min_dist_on_degree_5_and_10(oracle):
    """Bezier.minDist on a degree-5 and a degree-10 curve (it used to raise ValueError) returns the oracle's triple, in either
    order, 2-D against 2-D (each padded by its own length) and 2-D against 3-D."""
    from optimalbeziertrajectorygeneration_amd.bezier import Bezier
    c5, c10 = _deg5_deg10()
    c10s = Bezier(np.vstack((c10.cpts, np.linspace(0.0, 2.0, 11)[None])))
    for a, b in ((c5, c10), (c10, c5), (c5, c10s), (c10s, c5)):
        o = oracle.min_dist(a._padded(), b._padded(), max_depth=128, max_nodes=4000000)
        assert o["status"] == oracle.MD_OK
        got = a.minDist(b)
        assert isinstance(got, tuple) and len(got) == 3
        assert_identical(np.array(got), o["res"], "Bezier.minDist, degrees %d and %d" % (a.deg, b.deg))


def test_robust_calls_elevate_the_lower_curve():
    """minDist(robust=True) / collCheck(robust=True) on degrees 5 and 10 are the calls on the pair with the lower curve
    elevated by hand; collCheck without robust still refuses unequal degrees, and says where to go."""
    c5, c10 = _deg5_deg10()
    up = c5.elev(5)
    assert up.deg == 10
    assert c5.minDist(c10, robust=True) == up.minDist(c10, robust=True)
    assert c10.minDist(c5, robust=True) == c10.minDist(up, robust=True)
    assert c5.collCheck(c10, robust=True) == up.collCheck(c10, robust=True) == 1
    with pytest.raises(ValueError, match="robust=True"):
        c5.collCheck(c10)


def _mixed_problem(fdBatching):
    from optimalbeziertrajectorygeneration_amd.bezier import Bezier
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    rng = np.random.default_rng(77)
    obs = [Bezier(R.walk(rng, 1, 11, 2, s)[0, :2]) for s in (12.0, -12.0)]
    bo = BezOptimization(numVeh=3, dimension=2, degree=5, minimizeGoal='Euclidean', maxSep=0.5,
                         initPoints=[(0, 0), (0, 3), (0, 6)], finalPoints=[(6, 1), (6, 4), (6, 7)],
                         shapeObstacles=obs, fdBatching=fdBatching)
    # (seed 7: with the oracle alone, every pair's search ends at x and at every x + h e_k -- at seed 5 two vehicle pairs run into
    # the depth cap, where the closure raises as the reference's recursion would)
    return bo, bo.generateGuess(std=0.3, seed=7)


@pytest.fixture(scope="module")
def mixed_closure_rows():
    """spatialSeparationConstraints at x and at x + h e_k for every k, one call of the closure each (shared, read only)."""
    from optimalbeziertrajectorygeneration_amd.optimization import FD_STEP
    bo, x = _mixed_problem(False)
    rows = [bo.spatialSeparationConstraints(x)]
    for k in range(x.size):
        xk = x.copy()
        xk[k] += FD_STEP
        rows.append(bo.spatialSeparationConstraints(xk))
    return rows


def test_spatial_separation_constraints_mixed(oracle, mixed_closure_rows):
    """3 degree-5 vehicles and 2 degree-10 curve obstacles: the closure equals the oracle's pair loop (optimization.py:109-133)."""
    from optimalbeziertrajectorygeneration_amd.bezier import Bezier
    bo, x = _mixed_problem(False)
    y = bo.reshapeVector(x)
    curves = [Bezier(y[2 * i:2 * i + 2])._padded() for i in range(3)] + [c._padded() for c in bo.shapeObstacles]
    assert sorted(set(c.shape[1] for c in curves)) == [6, 11]
    pa, pb = np.triu_indices(5, 1)
    o = R.oracle_pairs(oracle, curves, pa, pb, max_depth=128, max_nodes=4000000)
    assert (o["status"] == 0).all()
    F = mixed_closure_rows[0]
    assert F.shape == (10, 3)
    assert_identical(F, o["res"] - 0.5, "spatialSeparationConstraints, degrees 5 and 10")


def test_spatial_separation_jacobian_mixed(mixed_closure_rows):
    """spatialSeparationJacobian on the same problem: entry for entry the n_x + 1 calls of the closure, the column=0 form its
    distance rows, and SciPy's approx_derivative through the served closure (one device call for the n_x rows) the same."""
    from scipy.optimize._numdiff import approx_derivative
    from optimalbeziertrajectorygeneration_amd.optimization import FD_STEP
    bo, x = _mixed_problem(False)
    J = bo.spatialSeparationJacobian(x)
    F0 = mixed_closure_rows[0]
    assert J.shape == (30, x.size)
    for k in range(x.size):
        dxk = (x[k] + FD_STEP) - x[k]
        assert np.array_equal(J[:, k], ((mixed_closure_rows[k + 1] - F0) / dxk).ravel()), k
    assert np.array_equal(bo.spatialSeparationJacobian(x, column=0), J.reshape(10, 3, -1)[:, 0, :])
    served, _ = _mixed_problem(True)
    Js = approx_derivative(lambda v: served.spatialSeparationConstraints(v).ravel(), x, method='2-point', abs_step=FD_STEP)
    assert served.fdBatchingStats['batches'] == 1 and served.fdBatchingStats['served'] == x.size
    assert np.array_equal(Js, J)


def test_min_dist_mixed_error_codes(capi):
    """Raw C ABI: the host's argument checks, all before any launch."""
    ctx = capi.scratch_context()
    lib, h = ctx._lib, ctx._h
    OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, capi.ERR_UNSUPPORTED           # (include/obtg.h: OBTG_ERR_ARG = -1)

    def call(off, pa=(0,), pb=(1,), cpts=True, res=True, offp=True):
        off = np.asarray(off, np.int32)
        pts = np.random.default_rng(1).normal(size=3 * max(int(off.max()), 1))
        pa, pb = np.asarray(pa, np.int32), np.asarray(pb, np.int32)
        out = np.zeros((max(pa.size, 1), 3))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        return lib.obtg_min_dist_mixed(h, p(pts) if cpts else None, p(off) if offp else None, off.size - 1, p(pa), p(pb), pa.size,
                                       1e-9, 128, 4096, 16, 100, p(out) if res else None, None, None)

    assert call([0, 3, 8]) == OK
    assert call([0, 3, 8], pa=(), pb=()) == OK                          # an empty pair list
    assert call([0, 3, 8], cpts=False) == ERR_ARG
    assert call([0, 3, 8], offp=False) == ERR_ARG
    assert call([0, 3, 8], res=False) == ERR_ARG
    assert call([0, 3, 2]) == ERR_ARG                                   # offsets that do not ascend
    assert call([0, 1, 8]) == ERR_ARG                                   # a curve of one point
    assert call([1, 4, 9]) == ERR_ARG                                   # offsets start at 0
    assert call([0, 3, 36]) == ERR_UNSUPPORTED                          # 33 control points
    assert call([0, 32, 35]) == OK                                      # 32 are taken
    assert call([0, 3, 8], pb=(2,)) == ERR_ARG                          # a pair index out of range
    assert call([0, 3, 8], pa=(-1,)) == ERR_ARG
