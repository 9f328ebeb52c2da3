"""Non-finite control points in the REDUCED separation forms (include/obtg.h, "Non-finite control points"): the seeded
cases, the function that plants the non-finite values, and the expectation, stated in NumPy from full rows.  No test here:
tests/test_nonfinite_rows_ref.py holds this file to the reference on the CPU (tests/golden/nonfinite_rows.npz), and
tests/test_gpu_nonfinite_rows.py holds every reduced entry point to it on the device.

The contract.  A pair's full row is what obtg_temporal_sep returns for it on the same context, at the same elevation R.
A row whose elements are all finite is CLEAN and reduces to the bits of its minimum; a row with any NaN or +-inf element is
DIRTY and reduces to NaN -- what `dv.normSquare().elev(10).cpts.min()` of Examples/SequentialSwarm.py:65 returns, because
the reference's elev is a dense np.dot with the elevation matrix (bezier.py:469-495: one non-finite coefficient makes the
whole elevated row NaN) and ndarray.min() keeps a NaN.  The active form (the k smallest with their positions) returns k
NaNs at the positions 0 .. k-1 for a dirty row.

Batches have two rows: row 0 stays as it was drawn, row 1 is planted, so every comparison also shows that clean rows keep
their bits next to dirty ones.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_rows_ref as C  # noqa: E402

MAX_SEP = C.SEP_MAX_SEP
B = 2
HUGE = 1e200                # finite, and HUGE * HUGE overflows: a dirty row from finite control points

# (name, n_veh, dim, deg, R, point obstacles): the shapes with a specialised kernel (k_normsq_elev<MINONLY[, ELEV]>; 66 pairs
# of the first are two waves) and those of the any-degree kernel (k_generic_normsq_elev, min_only)
FAST_SHAPES = (("nc 11, R = 0, 66 pairs", 12, 2, 10, 0, 1), ("nc 6, R = 0", 4, 2, 5, 0, 0), ("nc 6, R = 6", 9, 2, 5, 6, 0),
               ("nc 21, R = 30, 3-D", 6, 3, 20, 30, 1))
GENERIC_SHAPES = (("any degree: deg 12, R = 7", 5, 3, 12, 7, 1), ("any degree: deg 2", 6, 2, 2, 0, 0),
                  ("any degree: dim 1", 4, 1, 5, 0, 0))
# the reduced launch staged by slots and in row-window tiles: the smallest entries of constraint_rows_ref.SEP_CASES whose
# plan says so with min_only (name in SEP_CASES, the staging sep_form must answer)
STAGED = (("elevated, slot staging", "slots"), ("tiled", "tiled"))
FD_SHAPES = ((4, 2, 5, 0), (4, 2, 5, 6))                   # (n_veh, dim, deg, R): temporal_sep_fd_min_rows_dev and the FD view
# (dim, deg, R, candidates, others): one_vs_many_min[_spans]; the last is k_generic_one_vs_many_spans
ONE_MANY = ((3, 5, 0, 3, 5), (3, 5, 10, 3, 5))
ONE_MANY_GENERIC = (2, 12, 3, 3, 5)

PLANTINGS = ("nan at control point 0", "nan at a middle control point", "+inf at the last control point",
             "-inf at a middle control point", "whole vehicle nan", "two control points of +-1e200")
OBSTACLE_PLANTING = "nan in a point obstacle"


def plant_rows(Y, what, dim, veh=1):
    """A copy of the rows Y[..][n_veh * dim][deg + 1] (any leading shape) with `what` planted in vehicle `veh`."""
    Y = np.array(Y, dtype=np.float64, copy=True)
    nc = Y.shape[-1]
    r0, r1, mid = veh * dim, (veh + 1) * dim, nc // 2
    if what == "nan at control point 0":
        Y[..., r0, 0] = np.nan
    elif what == "nan at a middle control point":
        Y[..., r1 - 1, mid] = np.nan
    elif what == "+inf at the last control point":
        Y[..., r0, nc - 1] = np.inf
    elif what == "-inf at a middle control point":
        Y[..., r1 - 1, mid] = -np.inf
    elif what == "whole vehicle nan":
        Y[..., r0:r1, :] = np.nan
    elif what == "two control points of +-1e200":
        Y[..., r0, 0] = HUGE
        Y[..., r1 - 1, nc - 1] = -HUGE
    else:
        raise ValueError(what)
    return Y


def plant(Yb, what, dim, veh=1):
    """The batch Yb[B][n_veh * dim][deg + 1] with `what` planted in vehicle `veh` of batch row 1; every other row as it was."""
    out = np.array(Yb, dtype=np.float64, copy=True)
    out[1] = plant_rows(Yb[1], what, dim, veh)
    return out


def plant_obstacle(obs):
    """The point obstacles obs[M][dim] with a NaN coordinate in the first (obstacles belong to the context: both batch rows
    see it, and only the pairs with that obstacle are dirty)."""
    obs = np.array(obs, dtype=np.float64, copy=True)
    obs[0, -1] = np.nan
    return obs


def batch(seed, n_veh, dim, deg):
    return C.rows_batch(seed, B, n_veh, dim, deg, "full")


# ---------------------------------------------------------------------------------------------------------------------
#  the expectation, from full rows [..][L]
# ---------------------------------------------------------------------------------------------------------------------
def clean(rows):
    return np.isfinite(rows).all(-1)


def reduced_min(rows):
    rows = np.asarray(rows, dtype=np.float64)
    return np.where(clean(rows), rows.min(-1), np.nan)


def reduced_active(rows, k):
    """-> (values[..][k], positions[..][k]): the k smallest of each clean row in ascending POSITION (ties: the earlier position
    is the smaller, numpy's stable argsort); a dirty row: k NaNs at the positions 0 .. k-1."""
    rows = np.asarray(rows, dtype=np.float64)
    ok = clean(rows)
    order = np.argsort(np.where(ok[..., None], rows, 0.0), axis=-1, kind="stable")
    idx = np.sort(order[..., :k], axis=-1)
    val = np.take_along_axis(rows, idx, axis=-1)
    val[~ok] = np.nan
    idx[~ok] = np.arange(k)
    return val, idx.astype(np.int32)


def same(got, want):
    """bit for bit, NaN for NaN"""
    return np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
#  the fixture's inputs (tests/golden/gen_nonfinite_rows.py evaluates the reference on them)
# ---------------------------------------------------------------------------------------------------------------------
FIX_ROWS = dict(n_veh=4, dim=2, deg=5, elevs=(0, 6), seed=7300)            # optimization.py:311-346, DEG_ELEV 0 and 6
FIX_SEQ = dict(n_traj=6, candidates=3, dim=3, deg=5, elev=10, max_sep=1.0, seed=7301)   # Examples/SequentialSwarm.py:43-70


def fixture_rows_input(what):
    """Y[B][n_veh * dim][deg + 1] of the full-row part, planted (what = None: as drawn)"""
    f = FIX_ROWS
    Yb = batch(f["seed"], f["n_veh"], f["dim"], f["deg"])
    return Yb if what is None else plant(Yb, what, f["dim"])


def fixture_seq_input(what):
    """(one[3][dim][deg + 1], many[K][dim][deg + 1]) of the sequential part: trajectory 0 of draw b is candidate b, the
    others' trajectories are draw 0's (they are fixed in the planner).  Planted: candidate 1 and many[2]; candidates 0 and 2
    and the other trajectories stay as drawn."""
    f = FIX_SEQ
    Yb = C.rows_batch(f["seed"], f["candidates"], f["n_traj"], f["dim"], f["deg"], "full") * 0.25   # (separations of the order of max_sep)
    nc = f["deg"] + 1
    one = Yb[:, :f["dim"]].copy()
    many = Yb[0, f["dim"]:].reshape(f["n_traj"] - 1, f["dim"], nc).copy()
    if what is not None:
        one = plant(one, what, f["dim"], veh=0)
        many[2] = plant_rows(many[2], what, f["dim"], veh=0)
    return np.ascontiguousarray(one), many
