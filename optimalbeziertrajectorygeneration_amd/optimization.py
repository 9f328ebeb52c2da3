"""`optimization.BezOptimization` look-alike: same constructor, attributes and callback
signatures as the reference (optimization.py:20-308), with every constraint / cost
evaluation dispatched to the MI355X through libobtg_hip.so.

A driver script changes only its import lines:

    import optimalbeziertrajectorygeneration_amd.bezier as bez
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization

and hands the same closures to `scipy.optimize.minimize(method='SLSQP')`.  Beyond the
reference, each constraint has a `...Jacobian` provider that evaluates SciPy's whole
2-point finite-difference batch (n_x + 1 rows) in ONE launch; pass it as the 'jac' entry of
the constraint dict to remove the n_x + 1 serial callbacks per iteration.
"""
import numpy as np

from . import _capi
from . import bezier as bez

DEG_ELEV = 0   # module constant read at call time, like optimization.py:17

FD_STEP = 1.4901161193847656e-08   # SciPy '2-point' abs_step (sqrt of machine epsilon)


# ---------------------------------------------------------------------------------------------
# module-level evaluators with the reference's private signatures (optimization.py:311-459).
# Drivers copy / call these directly (Examples/Example1_DubinsCarTimeOptimal.py:19-52 re-implements
# the first one with a `degElev` argument), so they exist here too; contexts are cached per shape.
# ---------------------------------------------------------------------------------------------
import collections
import os

_CTX_CACHE_MAX = 8              # device contexts kept; the least recently used one is closed beyond that
_ctx_cache = collections.OrderedDict()


def _shape_ctx(nVeh, dim, deg, R, device=None):
    """A device context per (shape, DEG_ELEV): least-recently-used eviction, so that a driver sweeping degElev or the
    degree (Examples/Example1_DubinsCarTimeOptimal.py:19-52 takes degElev as an argument) does not pile up contexts.
    device None: this process's GPU (_capi.default_device: OBTG_DEVICE, else the launcher's LOCAL_RANK, else 0)."""
    if device is None:
        device = _capi.default_device()
    key = (int(nVeh), int(dim), int(deg), int(R), int(device))
    c = _ctx_cache.get(key)
    if c is None:
        c = _capi.Context(key[0], key[1], key[2], key[3], device=key[4])
        _ctx_cache[key] = c
        while len(_ctx_cache) > _CTX_CACHE_MAX:
            _, old = _ctx_cache.popitem(last=False)
            old.close()
    else:
        _ctx_cache.move_to_end(key)
    return c


# The private separation evaluator under SciPy's finite differences (round 6).  Examples/Example1_DubinsCarTimeOptimal.py:124-125
# hands SLSQP `lambda x: _temporalSeparationConstraints(bezopt.reshapeVector(x), ...)`: the function sees y, not x, and SciPy
# differences the lambda with n_x one-row calls per iteration.  As BezOptimization._serve does for the class closures: a call
# whose y differs from the last base in ONE element by exactly SciPy's step is taken for a row of that sweep -- the rows for
# every element of y are evaluated in one launch, kept, and this and the following calls are answered from them (a variable
# that moves several elements -- tf with prescribed speeds -- and any other point are evaluated directly and become the new
# base).  Values are those of the one-row call (the batch kernels' rows are its bits: tests/test_gpu_dropin.py).
_ysep_state = {}


def _temporalSeparationConstraints(y, nVeh, dim, maxSep, degElev=None):
    if nVeh <= 1:
        return None
    y = np.ascontiguousarray(y, dtype=np.float64)
    R = DEG_ELEV if degElev is None else degElev
    ctx = _shape_ctx(nVeh, dim, y.shape[1] - 1, R)
    if os.environ.get("OBTG_FD_BATCHING", "1") == "0":
        return ctx.temporal_sep(y, maxSep)[0]
    key = (int(nVeh), int(dim), y.shape, int(R), float(maxSep))
    st = _ysep_state.get(key)
    if st is not None and st['ctx'] is ctx:
        d = np.flatnonzero(y.ravel() != st['y0'].ravel())
        if d.size == 0:
            return st['base'].copy()
        if d.size == 1 and y.ravel()[d[0]] == st['y0'].ravel()[d[0]] + FD_STEP:
            if st['rows'] is None:
                E = y.size
                limit = float(os.environ.get("OBTG_FD_BATCH_MB", "512")) * 2.0 ** 20
                if 8.0 * E * st['base'].size > limit:
                    st['rows'] = False
                else:
                    Yb = np.repeat(st['y0'][None], E, axis=0)
                    Yb.reshape(E, E)[np.arange(E), np.arange(E)] += FD_STEP
                    st['rows'] = ctx.temporal_sep(Yb, maxSep)
            if st['rows'] is not False:
                return st['rows'][d[0]].copy()
            return ctx.temporal_sep(y, maxSep)[0]
    v = ctx.temporal_sep(y, maxSep)[0]
    if len(_ysep_state) > 8:
        _ysep_state.clear()
    _ysep_state[key] = {'ctx': ctx, 'y0': y.copy(), 'base': v.copy(), 'rows': None}
    return v


def _minSpeedConstraints(y, nVeh, dim, tf, minSpeed):
    y = np.ascontiguousarray(y, dtype=np.float64)
    return _shape_ctx(nVeh, dim, y.shape[1] - 1, DEG_ELEV).speed(y, tf, minSpeed, False)[0]


def _maxSpeedConstraints(y, nVeh, dim, tf, maxSpeed):
    y = np.ascontiguousarray(y, dtype=np.float64)
    return _shape_ctx(nVeh, dim, y.shape[1] - 1, DEG_ELEV).speed(y, tf, maxSpeed, True)[0]


def _maxAccelConstraints(y, nVeh, dim, tf, maxAccel):
    """The acceleration-bound rows, maxAccel**2 - (pos.diff().diff().normSquare().elev(DEG_ELEV)) per vehicle (obtg_accel):
    the curve of the reference's acceleration objective (optimization.py:503-519) as a constraint, any dimension."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    return _shape_ctx(nVeh, dim, y.shape[1] - 1, DEG_ELEV).accel(y, tf, maxAccel)[0]


def _maxJerkConstraints(y, nVeh, dim, tf, maxJerk):
    """The jerk-bound rows, maxJerk**2 - (pos.diff().diff().diff().normSquare().elev(DEG_ELEV)) per vehicle (obtg_jerk):
    the curve of the reference's jerk objective (optimization.py:522-539) as a constraint, any dimension."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    return _shape_ctx(nVeh, dim, y.shape[1] - 1, DEG_ELEV).jerk(y, tf, maxJerk)[0]


def _maxAngularRateConstraints(y, nVeh, dim, tf, maxAngRate):
    if dim != 2:
        raise ValueError('The input curve must be two dimensional,\n'
                         'instead it is {} dimensional'.format(dim))
    y = np.ascontiguousarray(y, dtype=np.float64)
    return _shape_ctx(nVeh, dim, y.shape[1] - 1, DEG_ELEV).ang_rate(y, tf, maxAngRate)[0]


def _euclideanObjective(y, nVeh, dim):
    """optimization.py:463-490: summed distances between neighbouring control points, every vehicle (obtg_euclidean_obj)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    return float(_shape_ctx(nVeh, dim, y.shape[1] - 1, 0).euclidean_obj(y)[0])


def _minAccelObjective(y, nVeh, dim, tf):
    """optimization.py:503-520: sum of the elevated control points of |acceleration|^2 (obtg_accel_obj)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    return float(_shape_ctx(nVeh, dim, y.shape[1] - 1, DEG_ELEV).deriv_energy_obj(y, tf, 2)[0])


def _minJerkObjective(y, nVeh, dim, tf):
    """optimization.py:523-540: the same for the jerk (obtg_jerk_obj)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    return float(_shape_ctx(nVeh, dim, y.shape[1] - 1, DEG_ELEV).deriv_energy_obj(y, tf, 3)[0])


def _angularRateSqr(bezTraj):
    """optimization.py:578-611: the squared angular rate of ONE planar trajectory as a rational curve -- control points
    num / den (inf / nan kept), weights den = (|v|^2)^2.  The quotient is obtg_ang_rate's (bound 0: the kernel returns
    0 - num/den), the weights two device products of the speed curve; the trajectory is taken at the degree it has."""
    if bezTraj.dim != 2:
        raise ValueError('The input curve must be two dimensional,\n'
                         'instead it is {} dimensional'.format(bezTraj.dim))
    cpts = np.ascontiguousarray(bezTraj.cpts, dtype=np.float64)
    ctx = _capi.Context(1, 2, bezTraj.deg, 0)
    try:
        quotient = 0.0 - ctx.ang_rate(cpts, bezTraj.tf - bezTraj.t0, 0.0)[0]
    finally:
        ctx.close()
    speed2 = bezTraj.diff().normSquare()              # (d / 2) |v|^2 with d = 2
    return bez.RationalBezier(quotient[None, :], (speed2 * speed2).cpts)


def _check_method(method):
    if method not in ('fd', 'exact'):
        raise ValueError("method must be 'fd' or 'exact', not {!r}".format(method))


# (key of BezOptimization.model, constructor keyword, container) -- optimization.py:49-63 defines the keys
_MODEL_FIELDS = (
    ('numVeh', 'numVeh', None), ('dim', 'dimension', None), ('deg', 'degree', None), ('minGoal', 'minimizeGoal', None),
    ('maxSep', 'maxSep', None), ('minSpeed', 'minSpeed', None), ('maxSpeed', 'maxSpeed', None),
    ('maxAngRate', 'maxAngRate', None), ('maxAccel', 'maxAccel', None), ('maxJerk', 'maxJerk', None),
    ('maxCurvature', 'maxCurvature', None), ('maxSpaceCurvature', 'maxSpaceCurvature', None),
    ('initPoints', 'initPoints', np.atleast_2d), ('finalPoints', 'finalPoints', np.atleast_2d),
    ('initSpeeds', 'initSpeeds', np.atleast_1d), ('finalSpeeds', 'finalSpeeds', np.atleast_1d),
    ('initAngs', 'initAngs', np.atleast_1d), ('finalAngs', 'finalAngs', np.atleast_1d),
    ('tf', 'tf', None),
)


# The per-vehicle constraint-row families, each described ONCE: the closures, _fd_values, the Jacobian
# providers, the true* accessors, the constructor's checks and _serve_key all read this table.
#   key: the family's name in _serve / _fd_values / _jac;  bound: its key in `model`, optional: None there means "no bound";
#   rows_attr: the attribute with its rows option ('all' / 'true_min');  rows, true_min, envelope, exact: the _capi.Context
#   methods of the control-point rows, the true minima, the true minima with their envelope blocks and the exact Jacobian
#   (None: not built), every one called (Y, tf[, bound], *lead);  planar: dim == 2 only;  sides: true-minimum rows per
#   vehicle ([B][N] values, or [B][N][2] flattened to row 2 v + side);  constraints, jacobian: the public names, as the
#   messages spell them;  noun: the rows' name in a sentence;  span: the device calls take tf (False: the rows do not depend
#   on the time span -- they are called (Y, bound, *lead), have no d/dtf, and their explicit tf column is an exact 0).
#   A family without a `rows` method (rows_attr and rows None) has true rows only: it has no rows option, its rows are always
#   the true ones, and it enters _serve_key behind the obstacles, only while its bound is set.
#   only_dim: the one dimension the family is built for (None: `planar` says it all) -- every public entry of the family
#   raises in any other dimension before a device call.
_RowFamily = collections.namedtuple('_RowFamily', 'key bound optional rows_attr rows true_min envelope exact lead planar sides '
                                                  'constraints jacobian noun span only_dim', defaults=(True, None))
_ROW_FAMILIES = (
    _RowFamily('vmax', 'maxSpeed', False, 'speedRows', 'speed', 'speed_true_min', 'speed_true_min_jac', 'speed_jac', (True,),
               False, 1, 'maxSpeedConstraints', 'maxSpeedJacobian', 'speed'),
    _RowFamily('vmin', 'minSpeed', False, 'speedRows', 'speed', 'speed_true_min', 'speed_true_min_jac', 'speed_jac', (False,),
               False, 1, 'minSpeedConstraints', 'minSpeedJacobian', 'speed'),
    _RowFamily('ang', 'maxAngRate', False, 'angRateRows', 'ang_rate', 'ang_rate_true_min', 'ang_rate_true_min_jac', 'ang_rate_jac', (),
               True, 2, 'maxAngularRateConstraints', 'maxAngularRateJacobian', 'angular-rate'),
    _RowFamily('amax', 'maxAccel', True, 'accelRows', 'accel', 'accel_true_min', 'accel_true_min_jac', None, (),
               False, 1, 'maxAccelConstraints', 'maxAccelJacobian', 'acceleration'),
    _RowFamily('jmax', 'maxJerk', True, 'jerkRows', 'jerk', 'jerk_true_min', 'jerk_true_min_jac', None, (),
               False, 1, 'maxJerkConstraints', 'maxJerkJacobian', 'jerk'),
    _RowFamily('curv', 'maxCurvature', True, None, None, 'curvature_true_min', 'curvature_true_min_jac', None, (),
               True, 2, 'maxCurvatureConstraints', 'maxCurvatureJacobian', 'curvature', False),
    _RowFamily('scurv', 'maxSpaceCurvature', True, None, None, 'space_curvature_true_min', 'space_curvature_true_min_jac', None, (),
               False, 1, 'maxSpaceCurvatureConstraints', 'maxSpaceCurvatureJacobian', 'space curvature', False, 3),
)
_FAMILY = {fam.key: fam for fam in _ROW_FAMILIES}
_ROWS_OPTIONS = tuple(dict.fromkeys(fam.rows_attr for fam in _ROW_FAMILIES if fam.rows is not None))      # speedRows, angRateRows, accelRows, jerkRows
# What a kept finite-difference batch depends on per family, in _serve_key's order: every rows option with, right behind it,
# the bounds that may be None; the other bounds follow maxSep.  A family enters the key by being in the table.
_KEY_ROWS = tuple((attr, tuple(fam.bound for fam in _ROW_FAMILIES if fam.optional and fam.rows_attr == attr)) for attr in _ROWS_OPTIONS)
_KEY_BOUNDS = tuple(fam.bound for fam in _ROW_FAMILIES if not fam.optional)
_KEY_TAIL = tuple(fam.bound for fam in _ROW_FAMILIES if fam.rows is None)            # (name, value) behind the obstacles, while set

# The keep-in family, BESIDE the table: its operand is an array kept on the object (`keepIn`, like
# `pointObstacles`), not a scalar bound of `model`, so it is in none of the tuples derived above -- the constructor checks its
# rows option after the table's and _serve_key appends its own entry while a region is set.  It is found by key like the
# others; its `bound` names the attribute, and what the device calls take in the bound's place is the pair of tables
# _keep_in_tables makes of it (BezOptimization._operand).
_KEEP_IN = _RowFamily('keepin', 'keepIn', True, 'keepInRows', 'keep_in', 'keep_in_true_min', 'keep_in_true_min_jac', None, (),
                      False, 1, 'keepInConstraints', 'keepInJacobian', 'keep-in', False)
_FAMILY[_KEEP_IN.key] = _KEEP_IN


def _keep_in_tables(keepIn, numVeh, dim):
    """(H[F][dim+1], VF[P][2]) of a `keepIn` argument, checked: a pair (A[F][dim], b[F]) -- the region A p <= b for every
    vehicle, items vehicle-major with the faces in order -- or a LIST of numVeh such pairs or Nones (a vehicle of its own
    region, or of none).  H holds the rows (a_f, b_f), VF the (vehicle, face) items (obtg_ctx_set_keep_in)."""
    if dim not in (2, 3):
        raise ValueError("keepIn needs dimension 2 or 3, not {}".format(dim))

    def faces(pair, who):
        try:
            A, b = pair
            A, b = np.asarray(A, dtype=float), np.asarray(b, dtype=float)
        except (TypeError, ValueError):
            raise ValueError("keepIn{} must be a pair (A[F][{}], b[F])".format(who, dim))
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] != dim or b.shape != (A.shape[0],):
            raise ValueError("keepIn{} must be a pair (A[F][{}], b[F]) with F >= 1, not shapes {} and {}"
                             .format(who, dim, A.shape, b.shape))
        return np.hstack((A, b[:, None]))

    if isinstance(keepIn, list):
        if len(keepIn) != numVeh:
            raise ValueError("a keepIn list must have numVeh = {} entries (pairs or None), not {}".format(numVeh, len(keepIn)))
        tables = [(v, faces(pair, '[{}]'.format(v))) for v, pair in enumerate(keepIn) if pair is not None]
        if not tables:
            raise ValueError("a keepIn list needs a region for at least one vehicle")
        first = np.cumsum([0] + [Hv.shape[0] for _, Hv in tables])
        VF = np.concatenate([np.stack((np.full(Hv.shape[0], v), o + np.arange(Hv.shape[0])), axis=1)
                             for (v, Hv), o in zip(tables, first)])
        return np.ascontiguousarray(np.vstack([Hv for _, Hv in tables])), np.ascontiguousarray(VF, dtype=np.int32)
    H = faces(keepIn, '')
    F = H.shape[0]
    VF = np.stack((np.repeat(np.arange(numVeh), F), np.tile(np.arange(F), numVeh)), axis=1)
    return np.ascontiguousarray(H), np.ascontiguousarray(VF, dtype=np.int32)

# The keep-out family, beside the table as _KEEP_IN is and for the same reason: its operand is the list
# `keepOut` kept on the object.  True rows only, like curvature (no rows option, no `rows` method): one row per (vehicle,
# obstacle), the least of max_f (a_f . c_v - b_f) over the trajectory minus `keepOutMargin`.  What the device calls take in the
# bound's place is the triple of tables _keep_out_tables makes of it; the margin goes beside it (_vehicle_true_min).
_KEEP_OUT = _RowFamily('keepout', 'keepOut', True, None, None, 'keep_out_true_min', 'keep_out_true_min_jac', None, (),
                       False, 1, 'keepOutConstraints', 'keepOutJacobian', 'keep-out', False)
_FAMILY[_KEEP_OUT.key] = _KEEP_OUT
_KEEP_OUT_MAX_FACES = 16


def _keep_out_tables(keepOut, numVeh, dim):
    """(H[F][dim+1], obs_off[O+1], VO[P][2]) of a `keepOut` argument, checked: a LIST of pairs (A[F_o][dim], b[F_o]), the convex
    obstacles A p <= b, every vehicle against every obstacle -- items vehicle-major with the obstacles in order, N * O rows
    (obtg_ctx_set_keep_out)."""
    if dim not in (2, 3):
        raise ValueError("keepOut needs dimension 2 or 3, not {}".format(dim))
    if not isinstance(keepOut, (list, tuple)) or len(keepOut) < 1:
        raise ValueError("keepOut must be a list of pairs (A[F][{}], b[F]), one per obstacle".format(dim))
    tables = []
    for o, pair in enumerate(keepOut):
        try:
            A, b = pair
            A, b = np.asarray(A, dtype=float), np.asarray(b, dtype=float)
        except (TypeError, ValueError):
            raise ValueError("keepOut[{}] must be a pair (A[F][{}], b[F])".format(o, dim))
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] != dim or b.shape != (A.shape[0],):
            raise ValueError("keepOut[{}] must be a pair (A[F][{}], b[F]) with F >= 1, not shapes {} and {}"
                             .format(o, dim, A.shape, b.shape))
        if A.shape[0] > _KEEP_OUT_MAX_FACES:
            raise ValueError("keepOut[{}] has {} faces: an obstacle may have at most {}".format(o, A.shape[0], _KEEP_OUT_MAX_FACES))
        tables.append(np.hstack((A, b[:, None])))
    O = len(tables)
    off = np.cumsum([0] + [Ho.shape[0] for Ho in tables])
    VO = np.stack((np.repeat(np.arange(numVeh), O), np.tile(np.arange(O), numVeh)), axis=1)
    return (np.ascontiguousarray(np.vstack(tables)), np.ascontiguousarray(off, dtype=np.int32),
            np.ascontiguousarray(VO, dtype=np.int32))


# The separation-region family, beside the table like _KEEP_OUT: its operand is the pair `separationRegion` kept
# on the object, ONE convex region around the origin that the relative curve c_i - c_j of every vehicle pair i < j must stay out
# of.  True rows only: one row per pair in the order of np.triu_indices(N, 1), the least of max_f (a_f . (c_i - c_j) - b_f) over
# the trajectory minus `separationRegionMargin` -- or, with separationRegionMetric='euclidean', of the signed Euclidean distance.
# What the device calls take in the bound's place is the table _separation_region_table makes of it.  Its rows belong to PAIRS:
# the envelope provider scatters each block to both vehicles (separationRegionJacobian), not to one owner.
_SEP_REGION = _RowFamily('sepregion', 'separationRegion', True, None, None, 'pair_keep_out_true_min', 'pair_keep_out_true_min_jac',
                         None, (), False, 1, 'separationRegionConstraints', 'separationRegionJacobian', 'separation-region', False)
_FAMILY[_SEP_REGION.key] = _SEP_REGION


def _separation_region_table(region, dim):
    """H[F][dim+1] of a `separationRegion` argument, checked like a `keepOut` entry: a pair (A[F][dim], b[F]), the region
    A d <= b around the origin -- every b_f finite and > 0 (obtg_ctx_set_pair_keep_out)."""
    if dim not in (2, 3):
        raise ValueError("separationRegion needs dimension 2 or 3, not {}".format(dim))
    try:
        A, b = region
        A, b = np.asarray(A, dtype=float), np.asarray(b, dtype=float)
    except (TypeError, ValueError):
        raise ValueError("separationRegion must be a pair (A[F][{}], b[F])".format(dim))
    if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] != dim or b.shape != (A.shape[0],):
        raise ValueError("separationRegion must be a pair (A[F][{}], b[F]) with F >= 1, not shapes {} and {}"
                         .format(dim, A.shape, b.shape))
    if A.shape[0] > _KEEP_OUT_MAX_FACES:
        raise ValueError("separationRegion has {} faces: a region may have at most {}".format(A.shape[0], _KEEP_OUT_MAX_FACES))
    if not (np.all(np.isfinite(b)) and np.all(b > 0.0)):
        raise ValueError("separationRegion needs every b_f finite and > 0 (the origin strictly inside), not {!r}".format(b.tolist()))
    return np.ascontiguousarray(np.hstack((A, b[:, None])))


# The proximity family, beside the table like _SEP_REGION: its operand is the pair of lists `waypoints` and
# `stayWithin` kept on the object.  True rows only: one row per entry, the waypoints in list order (the MAXIMUM over the entry's
# window of (d/2)(radius^2 - |c_v - target|^2): >= 0 iff the vehicle comes within the radius at some time of the window), then the
# stayWithin entries (the MINIMUM: >= 0 iff it never leaves range).  What the device calls take in the bound's place is the
# triple of tables _proximity_tables makes of the lists.  A row with a vehicle target belongs to both vehicles: the envelope
# provider scatters its block with +1 and -1 (proximityJacobian).
_PROXIMITY = _RowFamily('proximity', 'waypoints/stayWithin', True, None, None, 'proximity_true', 'proximity_true_jac', None, (),
                        False, 1, 'proximityConstraints', 'proximityJacobian', 'proximity', False)
_FAMILY[_PROXIMITY.key] = _PROXIMITY


def _proximity_tables(waypoints, stayWithin, numVeh, dim):
    """(items[P][3], params[P][3], points[Q][dim]) of the `waypoints` and `stayWithin` arguments, checked: each a list (or None)
    of entries (vehicle, target, radius) or (vehicle, target, radius, (tau0, tau1)) -- target an int (another vehicle) or a point
    of the problem's dimension, radius finite and > 0, 0 <= tau0 < tau1 <= 1 the window of the normalised parameter (default the
    whole trajectory).  Rows: the waypoints in list order, then the stayWithin entries (obtg_ctx_set_proximity)."""
    if dim not in (2, 3):
        raise ValueError("waypoints and stayWithin need dimension 2 or 3, not {}".format(dim))
    items, params, points = [], [], []
    for name, entries, kind in (('waypoints', waypoints, _capi.PROX_REACH), ('stayWithin', stayWithin, _capi.PROX_WITHIN)):
        if entries is None:
            continue
        if not isinstance(entries, (list, tuple)) or len(entries) < 1:
            raise ValueError("{} must be a list of entries (vehicle, target, radius[, (tau0, tau1)])".format(name))
        for e, entry in enumerate(entries):
            who = "{}[{}]".format(name, e)
            if not isinstance(entry, (list, tuple)) or len(entry) not in (3, 4):
                raise ValueError("{} must be (vehicle, target, radius) or (vehicle, target, radius, (tau0, tau1))".format(who))
            veh, target, radius = entry[:3]
            if not isinstance(veh, (int, np.integer)) or not 0 <= veh < numVeh:
                raise ValueError("{} needs a vehicle index in 0 .. {}, not {!r}".format(who, numVeh - 1, veh))
            if isinstance(target, (int, np.integer)):
                if not 0 <= target < numVeh or target == veh:
                    raise ValueError("{} needs another vehicle's index in 0 .. {} as its target, not {!r}".format(who, numVeh - 1, target))
                b = int(target)
            else:
                try:
                    pt = np.asarray(target, dtype=float).reshape(-1)
                except (TypeError, ValueError):
                    pt = np.zeros(0)
                if pt.shape != (dim,) or not np.all(np.isfinite(pt)):
                    raise ValueError("{} needs a target that is a vehicle index or a finite point of dimension {}, not {!r}"
                                     .format(who, dim, target))
                b = numVeh + len(points)
                points.append(pt)
            try:
                rho = float(radius)
            except (TypeError, ValueError):
                rho = float('nan')
            if not (np.isfinite(rho) and rho > 0.0):
                raise ValueError("{} needs a finite radius > 0, not {!r}".format(who, radius))
            try:
                tau0, tau1 = (float(v) for v in (entry[3] if len(entry) == 4 else (0.0, 1.0)))
            except (TypeError, ValueError):
                tau0 = tau1 = float('nan')
            if not 0.0 <= tau0 < tau1 <= 1.0:
                raise ValueError("{} needs a window (tau0, tau1) with 0 <= tau0 < tau1 <= 1, not {!r}".format(who, entry[3]))
            items.append((int(veh), b, kind))
            params.append((rho, tau0, tau1))
    if not items:
        raise ValueError("waypoints and stayWithin are both None: there are no proximity rows")
    return (np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 3), np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 3),
            np.ascontiguousarray(points, dtype=np.float64).reshape(-1, dim))


def _keep_out_motion_tables(keepOutMotion, keepOut, dim, deg, tf=None):
    """(Q, q_off[O+1], T[O]) of a `keepOutMotion` argument, checked: a LIST with one entry per obstacle of `keepOut` -- None (the
    obstacle stands still), a bezier.Bezier of the problem's dimension with t0 == 0 (the obstacle's offset on [0, tf]), or a pair
    (cpts[dim][m+1], T).  Q holds the [dim][m+1] blocks one after the other, q_off counts control points, an empty run for None
    (obtg_ctx_set_keep_out_motion).  tf: the span of a fixed-tf problem, which no motion may end before."""
    if keepOut is None:
        raise ValueError("keepOutMotion needs keepOut: there are no obstacles to move")
    if not isinstance(keepOutMotion, (list, tuple)) or len(keepOutMotion) != len(keepOut):
        raise ValueError("keepOutMotion must be a list with one entry per obstacle of keepOut ({}): None, a Bezier or a pair "
                         "(cpts[{}][m+1], T)".format(len(keepOut), dim))
    blocks, counts, spans = [], [], []
    for o, entry in enumerate(keepOutMotion):
        if entry is None:
            counts.append(0)
            spans.append(1.0)
            continue
        if isinstance(entry, bez.Bezier):
            if entry.t0 != 0:
                raise ValueError("keepOutMotion[{}] must start at t0 = 0, not {!r}".format(o, entry.t0))
            cpts, T = np.asarray(entry.cpts, dtype=float), float(entry.tf)
        else:
            try:
                cpts, T = entry
                cpts, T = np.asarray(cpts, dtype=float), float(T)
            except (TypeError, ValueError):
                raise ValueError("keepOutMotion[{}] must be None, a Bezier or a pair (cpts[{}][m+1], T)".format(o, dim))
        if cpts.ndim != 2 or cpts.shape[0] != dim or cpts.shape[1] < 1:
            raise ValueError("keepOutMotion[{}] must have dimension {} (control points [{}][m+1]), not shape {}"
                             .format(o, dim, dim, cpts.shape))
        if cpts.shape[1] - 1 > deg:
            raise ValueError("keepOutMotion[{}] has degree {}: a motion's degree may not be above the problem's, {}"
                             .format(o, cpts.shape[1] - 1, deg))
        if not (np.isfinite(T) and T > 0):
            raise ValueError("keepOutMotion[{}] needs a finite span T > 0, not {!r}".format(o, T))
        if tf is not None and T < tf:
            raise ValueError("keepOutMotion[{}] ends at T = {!r}, before the problem's tf = {!r}".format(o, T, tf))
        blocks.append(np.ascontiguousarray(cpts).reshape(-1))
        counts.append(cpts.shape[1])
        spans.append(T)
    Q = np.concatenate(blocks) if blocks else np.zeros(0)
    return (np.ascontiguousarray(Q), np.ascontiguousarray(np.cumsum([0] + counts), dtype=np.int32),
            np.ascontiguousarray(spans, dtype=float))

# The goals with a device call ('timeopt' is x[-1]).  goal, lower case: (key in _serve / _fd_values; values [B] of the rows Y;
# gradient blocks [B][N d][n+1] of the rows Y), both called (bezopt, ctx, Y, what) -- `what` names the caller where a search
# that does not end raises (the arc length alone).
_Goal = collections.namedtuple('_Goal', 'key value grad')
_GOALS = {
    'euclidean': _Goal('obj_euclidean', lambda bo, c, Y, what: c.euclidean_obj(Y), lambda bo, c, Y, what: c.euclidean_grad(Y)),
    'accel': _Goal('obj_accel', lambda bo, c, Y, what: c.deriv_energy_obj(Y, bo.model['tf'], 2),
                   lambda bo, c, Y, what: c.deriv_energy_grad(Y, bo.model['tf'], 2)[0]),
    'jerk': _Goal('obj_jerk', lambda bo, c, Y, what: c.deriv_energy_obj(Y, bo.model['tf'], 3),
                  lambda bo, c, Y, what: c.deriv_energy_grad(Y, bo.model['tf'], 3)[0]),
    'arclength': _Goal('obj_arclength', lambda bo, c, Y, what: bo._arc_length(c, Y, what=what)['val'],
                       lambda bo, c, Y, what: bo._arc_length(c, Y, grad=True, what=what)['grad']),
}
_GOAL_OF_KEY = {goal.key: goal for goal in _GOALS.values()}

_ANG_RATE_ORDER_CODE = {'fast': 0, 'elevate_first': 1, 'exact': 2}      # obtg_ctx_set_ang_rate_order


def _md_checked(r, what='minDist'):
    """r, the dict of a search call -- unless one of its searches did not end: then the exception of the first status, in list
    order, that is not MD_OK (bezier._raise_md): what the reference would hit first in its pair loop (optimization.py:127-131)."""
    status = np.asarray(r['status']).ravel()
    bad = np.flatnonzero(status != _capi.MD_OK)
    if bad.size:
        bez._raise_md(int(status[bad[0]]), what)
    return r


def _min_dist_call(curves, pa, pb, robust):
    """The `_minDist` sweep of the spatial-separation calls: curves is an array [n][3][K] (obtg_min_dist[_robust], as ever) or,
    where degrees differ, a list of [3][K_i] arrays -- obtg_min_dist_mixed, or for robust=True the curves elevated to the
    highest degree (bezier.elevated_stack) through obtg_min_dist_robust."""
    ctx = _capi.scratch_context()
    if robust:
        stack = bez.elevated_stack(curves) if isinstance(curves, list) else curves
        return ctx.min_dist_robust(stack, pa, pb, eps=1e-9, max_nodes=400000)
    call = ctx.min_dist_mixed if isinstance(curves, list) else ctx.min_dist
    return call(curves, pa, pb, eps=1e-9, max_depth=128, max_nodes=4000000)


def _spatial_jac_plan(Y, numVeh, dim, obstacle_curves):
    """The curve and pair lists of ONE `obtg_min_dist` call that yields the 2-point Jacobian of
    spatialSeparationConstraints (optimization.py:109-133): the base evaluation's C(n, 2) pairs of the n = numVeh +
    obstacles curves of row 0 of Y, then, for every finite-difference row k + 1, the pairs that contain a vehicle whose
    control points differ from row 0's, with that vehicle's perturbed curve appended to the curve list.
    Y: [n_x + 1][numVeh * dim][deg + 1]; obstacle_curves: padded [3][K_o] arrays, of any degree each.
    Returns (stack [n_curves][3][deg + 1], pa, pb, P, col, row, pos): entry e of the call's extra pairs is base pair
    row[e] re-evaluated for variable col[e] at position pos[e] of the pair list.  Pairs of a column come in base-pair
    order, columns in order (array form of the loops it replaced: tests/test_host_logic.py holds it to them).
    Where an obstacle's degree is not the vehicles', `stack` is the LIST of the same curves in the same order instead
    (obtg_min_dist_mixed's operand); the pair lists do not depend on degrees."""
    nx = Y.shape[0] - 1
    K = Y.shape[2]
    n = numVeh + len(obstacle_curves)
    Yv = Y.reshape(nx + 1, numVeh, dim, K)
    changed = np.any(Yv[1:] != Yv[0], axis=(2, 3))              # [n_x][numVeh]
    ck, cv = np.nonzero(changed)                                # (column, vehicle), columns ascending, vehicles ascending
    extra = np.zeros((ck.size, 3, K))
    extra[:, :dim, :] = Yv[ck + 1, cv]
    if any(c.shape[1] != K for c in obstacle_curves):
        base = np.zeros((numVeh, 3, K))
        base[:, :dim, :] = Yv[0]
        base = list(base) + list(obstacle_curves)
        extra = list(extra)
        join = lambda: base + extra
    else:
        base = np.zeros((n, 3, K))
        base[:numVeh, :dim, :] = Yv[0]
        for o, c in enumerate(obstacle_curves):
            base[numVeh + o] = c
        join = lambda: np.concatenate((base, extra))
    # The pair lists depend on WHICH vehicles every column moves, not on the values: an SLSQP run asks for the same pattern at
    # every iterate, so the lists of the last pattern are kept (round 6: building them was 16 of the provider's 35 ms at C5 size).
    memo = _spatial_jac_plan.memo
    pattern = (n, numVeh, changed.shape, changed.tobytes())
    if memo.get('pattern') == pattern:
        pa, pb, P, col, row, pos = memo['lists']
        return join(), pa, pb, P, col, row, pos
    pa0, pb0 = np.triu_indices(n, 1)                            # i < j, lexicographic: the reference's pair loop
    P = pa0.size
    new_id = np.full((nx, n), -1, dtype=np.int64)               # curve index of vehicle v's perturbed copy in column k
    new_id[ck, cv] = n + np.arange(ck.size)
    # per column, the base pairs touched: those with an end among the column's changed vehicles.  A column that moves ONE
    # vehicle (all but a trailing tf) touches that vehicle's n - 1 pairs; the others go through a mask over the pair list.
    nchg = changed.sum(axis=1)
    pairs_of = np.empty((numVeh, n - 1), dtype=np.int64)        # base pairs containing vehicle v, ascending
    for v in range(numVeh):
        pairs_of[v] = np.nonzero((pa0 == v) | (pb0 == v))[0]
    k1 = np.nonzero(nchg == 1)[0]
    col = [np.repeat(k1, n - 1)]
    row = [pairs_of[np.argmax(changed[k1], axis=1)].ravel()] if k1.size else [np.zeros(0, dtype=np.int64)]
    for k in np.nonzero(nchg > 1)[0]:
        m = np.zeros(n, dtype=bool)
        m[:numVeh] = changed[k]
        q = np.nonzero(m[pa0] | m[pb0])[0]
        col.append(np.full(q.size, k))
        row.append(q)
    col, row = np.concatenate(col).astype(np.int64), np.concatenate(row)
    order = np.lexsort((row, col))                              # column-major, base-pair order within a column
    col, row = col[order], row[order]
    ia, ib = pa0[row], pb0[row]
    na, nb = new_id[col, ia], new_id[col, ib]
    pa = np.concatenate((pa0, np.where(na >= 0, na, ia))).astype(np.int32)
    pb = np.concatenate((pb0, np.where(nb >= 0, nb, ib))).astype(np.int32)
    pos = P + np.arange(col.size)
    memo['pattern'], memo['lists'] = pattern, (pa, pb, P, col, row, pos)
    return join(), pa, pb, P, col, row, pos


_spatial_jac_plan.memo = {}


class BezOptimization(object):
    def __init__(self,
                 numVeh=1,
                 dimension=1,
                 degree=5,
                 minimizeGoal='Euclidean',
                 maxSep=0.9,
                 minSpeed=0,
                 maxSpeed=1e6,
                 maxAngRate=1e6,
                 initPoints=None,
                 finalPoints=None,
                 initSpeeds=None,
                 finalSpeeds=None,
                 initAngs=None,
                 finalAngs=None,
                 tf=1.0,
                 pointObstacles=None,
                 shapeObstacles=None,
                 device=None,
                 separationRows='all',
                 angRateOrder='fast',
                 activeRows=2,
                 fdBatching=True,
                 speedRows='all',
                 angRateRows='all',
                 maxAccel=None,
                 accelRows='all',
                 maxJerk=None,
                 jerkRows='all',
                 maxCurvature=None,
                 maxSpaceCurvature=None,
                 keepIn=None,
                 keepInRows='all',
                 keepOut=None,
                 keepOutMargin=0.0,
                 keepOutMotion=None,
                 keepOutMetric='faces',
                 separationRegion=None,
                 separationRegionMargin=0.0,
                 separationRegionMetric='faces',
                 waypoints=None,
                 stayWithin=None):
        """Beyond the reference's keywords: `device` (HIP ordinal; None: this process's, see _capi.default_device) and `separationRows` --
        'all': temporalSeparationConstraints returns every elevated control point of every pair, as the
        reference does (optimization.py:337); 'min': one row per pair, the smallest of them -- the
        `dv.normSquare().min()` form the reference leaves commented at optimization.py:338 and uses in
        Examples/SequentialSwarm.py:65 -- which hands SLSQP 2n+R+1 times fewer rows (SURVEY.md 8(f) item 4:
        its dense least-squares step is what dominates an iteration once the callbacks are fast)."""
        # 'active' (round 5; SURVEY.md 8(f) item 4 as worded: "only active / near-active constraint rows"): per pair its
        # `activeRows` SMALLEST elevated control points, in control-point order (1..4; obtg_temporal_sep_active) -- a fixed number of rows, so
        # SLSQP's constraint count is constant, but more than the single piecewise-smooth minimum that makes it stall.
        # 'true_min': per pair the true minimum over the trajectory's time of the squared separation minus maxSep^2
        # (obtg_temporal_sep_true_min) -- the tight continuous-time value that the control points only bound from below
        # and that DEG_ELEV exists to approach: P rows whatever DEG_ELEV is.
        # speedRows 'true_min': per vehicle the true minimum over the trajectory's time of each speed row's polynomial
        # (obtg_speed_true_min) -- N rows per bound whatever DEG_ELEV is, feasible iff >= 0 -- instead of its N (2n+R+1)
        # elevated control points ('all', the reference's rows: optimization.py:349-422), which only bound it from below
        # angRateRows 'true_min': per vehicle the true minima over the trajectory's time of W den - num and W den + num
        # (obtg_ang_rate_true_min; den = |v|^2, num = y'' x' - x'' y', W = maxAngRate): 2N rows whatever DEG_ELEV is, feasible
        # iff >= 0, in units of W speed^2 -- NOT the scale of 'all', the reference's N (4(n+R)+1) quotients W^2 - num_k/den_k
        # of control points (optimization.py:425-459), which bound omega^2 from one side only.  For trajectories that do not stop.
        # maxAccel (None: no bound): |acceleration| <= maxAccel per vehicle, in any dimension -- maxAccelConstraints.  accelRows
        # 'all': the N (2n+R+1) elevated control points of maxAccel^2 - (d/2)|c''|^2 (the curve of the reference's acceleration
        # objective, optimization.py:503-519, under a bound); 'true_min': per vehicle its true minimum over the trajectory's
        # time (obtg_accel_true_min) -- N rows whatever DEG_ELEV is, feasible iff >= 0.
        # maxJerk (None: no bound): |jerk| <= maxJerk per vehicle, in any dimension -- maxJerkConstraints.  jerkRows 'all': the
        # N (2n+R+1) elevated control points of maxJerk^2 - (d/2)|c'''|^2 (the curve of the reference's jerk objective,
        # optimization.py:522-539, under a bound); 'true_min': per vehicle its true minimum over the trajectory's time
        # (obtg_jerk_true_min) -- N rows whatever DEG_ELEV is, feasible iff >= 0.
        # maxCurvature (None: no bound; dim 2): |curvature| <= maxCurvature per vehicle, a turning radius of 1 / maxCurvature
        # that does not move with tf -- maxCurvatureConstraints: 2N true rows, maxCurvature - max over the path of max(0, +-kappa)
        # (obtg_curvature_true_min).  Curvature is not a polynomial: there is no control-point form and no rows option.
        # maxSpaceCurvature (None: no bound; dim 3): curvature <= maxSpaceCurvature per vehicle in space, |c' x c''| / |c'|^3
        # -- maxSpaceCurvatureConstraints: N true rows, maxSpaceCurvature - max over the path of kappa
        # (obtg_space_curvature_true_min).  The norm of a cross product has no sign: one row per vehicle.
        # keepIn (None: no region; dim 2 or 3): stay inside -- a pair (A[F][d], b[F]), the region A p <= b for every vehicle, or
        # a LIST of numVeh such pairs or Nones (a tuple is one pair, a list is per vehicle) -- keepInConstraints: one row
        # b_f - a_f . c_v per (vehicle, face), vehicle-major, faces in order.  keepInRows 'all': its n+R+1 control points, exact
        # linear constraints (obtg_keep_in); 'true_min': its true margin over the trajectory (obtg_keep_in_true_min), P rows
        # whatever DEG_ELEV is.  Kept as `self.keepIn`, like pointObstacles: a driver may edit the arrays in place between solves.
        given = locals()
        for attr in reversed(_ROWS_OPTIONS):         # (the newest family's option is checked first, as it always was)
            if given[attr] not in ('all', 'true_min'):
                raise ValueError("{} must be 'all' or 'true_min', not {!r}".format(attr, given[attr]))
            setattr(self, attr, given[attr])
        if keepInRows not in ('all', 'true_min'):    # (the keep-in family is beside the table: after the table's options)
            raise ValueError("keepInRows must be 'all' or 'true_min', not {!r}".format(keepInRows))
        self.keepInRows = keepInRows
        if keepIn is not None:
            _keep_in_tables(keepIn, numVeh, dimension)      # raises for a region the device calls could not take
        self.keepIn = keepIn
        # keepOut (None: no obstacles; dim 2 or 3): stay outside -- a list of pairs (A[F][d], b[F]), the convex obstacles
        # A p <= b (bezier.halfspacesOfPolygon makes one of a polygon's vertices), every vehicle against every obstacle --
        # keepOutConstraints: N * O true rows, vehicle-major, min over the trajectory of max_f (a_f . c_v - b_f) minus
        # keepOutMargin (obtg_keep_out_true_min).  With unit normals a row >= 0 implies a true clearance >= keepOutMargin; the
        # row is conservative near corners (unless keepOutMetric='euclidean') and negative (minus the depth) inside.  Kept as
        # `self.keepOut`, like keepIn.
        if keepOut is not None:
            _keep_out_tables(keepOut, numVeh, dimension)     # raises for obstacles the device calls could not take
            if not np.isfinite(float(keepOutMargin)):
                raise ValueError("keepOutMargin must be finite, not {!r}".format(keepOutMargin))
        self.keepOut = keepOut
        self.keepOutMargin = float(keepOutMargin)
        # keepOutMotion (None: every obstacle stands still): one entry per obstacle of keepOut -- None, a bezier.Bezier with
        # t0 == 0 or a pair (cpts[d][m+1], T): the obstacle's OFFSET as a function of absolute time on [0, T], translation only,
        # of a degree no higher than the problem's.  The rows become those of the relative curve c_v(s) - q_o(s tf)
        # (obtg_keep_out_moving_true_min) and, in a time-optimal problem, depend on tf.  Kept as `self.keepOutMotion`.
        if keepOutMotion is not None:
            _keep_out_motion_tables(keepOutMotion, keepOut, dimension, degree,
                                    None if str(minimizeGoal).lower() == 'timeopt' else float(tf))
        self.keepOutMotion = keepOutMotion
        # keepOutMetric ('faces': the rows above; 'euclidean': the signed Euclidean distance in their place -- rounded corners,
        # obtg_keep_out_euclid_true_min): with unit normals both agree where the nearest feature is a face; the Euclidean rows
        # are not conservative near corners and C^1 outside.  Kept as `self.keepOutMetric`.
        self._check_keep_out_metric(keepOutMetric, keepOutMotion)
        self.keepOutMetric = keepOutMetric
        # separationRegion (None: none; dim 2 or 3): polytopic vehicle-to-vehicle separation -- a pair (A[F][d], b[F]), every
        # b_f > 0: the relative curve c_i - c_j of every pair i < j stays outside {d : A d <= b}.  separationRegionConstraints:
        # N (N - 1) / 2 true rows in the order of np.triu_indices(N, 1), min over the trajectory of max_f (a_f . (c_i - c_j) - b_f)
        # minus separationRegionMargin (obtg_pair_keep_out_true_min), or with separationRegionMetric='euclidean' of the signed
        # Euclidean distance (obtg_pair_keep_out_euclid_true_min).  Beside maxSep, not in its place; vehicles only.  A region
        # with R != -R makes a row depend on which vehicle of the pair has the smaller index.  Kept as `self.separationRegion`.
        if separationRegion is not None:
            _separation_region_table(separationRegion, dimension)
            if not np.isfinite(float(separationRegionMargin)):
                raise ValueError("separationRegionMargin must be finite, not {!r}".format(separationRegionMargin))
        self._check_separation_region_metric(separationRegionMetric)
        self.separationRegion = separationRegion
        self.separationRegionMargin = float(separationRegionMargin)
        self.separationRegionMetric = separationRegionMetric
        # waypoints, stayWithin (None: none; dim 2 or 3): "come close" and "stay close" -- lists of (vehicle, target, radius) or
        # (vehicle, target, radius, (tau0, tau1)), target another vehicle's index or a point, (tau0, tau1) the window of the
        # normalised parameter in which the row is taken (ordered gates: (0, 0.5), then (0.5, 1)).  proximityConstraints: one
        # true row per entry, the waypoints first (obtg_proximity_true).  A window in tau does not depend on tf.  Kept as
        # `self.waypoints` and `self.stayWithin`, read when a closure is called, like keepOut.
        if waypoints is not None or stayWithin is not None:
            _proximity_tables(waypoints, stayWithin, numVeh, dimension)      # raises for entries the device calls could not take
        self.waypoints = waypoints
        self.stayWithin = stayWithin
        if separationRows not in ('all', 'min', 'active', 'true_min'):
            raise ValueError("separationRows must be 'all', 'min', 'active' or 'true_min', not {!r}".format(separationRows))
        if separationRows == 'active' and not 1 <= int(activeRows) <= 4:
            raise ValueError("activeRows must be 1..4, not {!r}".format(activeRows))
        self.activeRows = int(activeRows)
        # DEG_ELEV > 0 only: 'fast' forms the angular rate's products at degree 4n and elevates them (0.2 ms at C5);
        # 'elevate_first' elevates the position first, the sequence of optimization.py:597 (1.8 ms); 'exact' = 'fast' plus a
        # double-double recompute of the rows of vehicles that nearly stop.  Until round 6 'elevate_first' was called
        # 'reference' (still accepted): it follows the reference's SEQUENCE of operations, but where a vehicle nearly stops it
        # is no closer to the reference's values than the other orders (nearstop.npz's worst vehicle: 4.6e-9 against 3.4e-9
        # for 'fast' and 3.0e-9 for 'exact' -- the reference itself is 3.0e-9 from the exact rational value there, and its
        # own sums run through OpenBLAS in an order no restatement short of that library's kernels reproduces): the name
        # promised what no float64 order delivers (tests/test_gpu_parity.py::test_near_stop_angular_rate_on_device)
        if angRateOrder == 'reference':
            angRateOrder = 'elevate_first'
        if angRateOrder not in ('fast', 'elevate_first', 'exact'):
            raise ValueError("angRateOrder must be 'fast', 'elevate_first' or 'exact', not {!r}".format(angRateOrder))
        self.angRateOrder = angRateOrder
        self.pointObstacles = pointObstacles
        self.shapeObstacles = shapeObstacles
        self._device = _capi.default_device() if device is None else int(device)
        self.separationRows = separationRows
        # SciPy's own finite differences, served from one batched evaluation (see _serve); OBTG_FD_BATCHING=0 turns it off everywhere
        self.fdBatching = bool(fdBatching) and os.environ.get("OBTG_FD_BATCHING", "1") != "0"
        self.fdBatchingStats = {'batches': 0, 'served': 0, 'direct': 0}
        self._fd_state = None

        # `model` keeps the reference's keys (drivers read and edit them, Examples/*.py); what each holds is decided by
        # _MODEL_FIELDS: scalars as given, per-vehicle data as arrays with a vehicle axis
        self.model = {key: (given[kw] if shape is None else shape(given[kw])) for key, kw, shape in _MODEL_FIELDS}
        # free control points per coordinate row: the end points, and with prescribed speeds their neighbours, are
        # not variables (two columns each)
        self._numCols = degree + 1 - 2 * sum(given[kw] is not None for kw in ('initPoints', 'initSpeeds'))
        self._ctxs = {}

    # ------------------------------------------------------------------ device contexts
    def _ctx(self, with_point_obs):
        """Context for the current DEG_ELEV (created on first use; the reference's counterpart
        is the lazily filled class-level matrix caches, bezier.py:48-52)."""
        c = self._ctxs.get(bool(with_point_obs))
        if c is None:
            c = self._new_ctx(bool(with_point_obs), self.model['numVeh'], self.pointObstacles if with_point_obs else None)
        if c.deg_elev != int(DEG_ELEV):
            c.set_deg_elev(int(DEG_ELEV))
        return c

    def _ctx_one(self):
        """A one-vehicle context of the same degree: the per-vehicle families evaluated on a compact
        batch of single vehicles (structured Jacobians)."""
        c = self._ctxs.get('one') or self._new_ctx('one', 1, None)
        if c.deg_elev != int(DEG_ELEV):
            c.set_deg_elev(int(DEG_ELEV))
        return c

    def _new_ctx(self, key, n_veh, obs):
        c = _capi.Context(n_veh, self.model['dim'], self.model['deg'], int(DEG_ELEV), point_obs=obs, device=self._device)
        c.set_ang_rate_order(_ANG_RATE_ORDER_CODE[self.angRateOrder])
        self._ctxs[key] = c
        return c

    @property
    def angRateOrderInEffect(self):
        """'fast' / 'elevate_first' / 'exact': the order the angular rate of this problem REALLY runs in at the current DEG_ELEV
        (the constructor's `angRateOrder` is a request: DEG_ELEV = 0 has one order, and degrees or elevations without a
        products-then-elevation kernel run in the reference's order, without the double-double pass)."""
        return ('fast', 'elevate_first', 'exact')[self._ctx(False).ang_rate_order_in_effect()]

    def _active_k(self):
        """rows per pair of separationRows='active': never more than a pair has control points"""
        return min(self.activeRows, 2 * self.model['deg'] + int(DEG_ELEV) + 1)

    # separationRows='true_min': the rows are differenced with h = FD_STEP (1.5e-8), so the search's own slack must sit far
    # below h x the rows' slope: at the library's default eps_rel = 1e-9 a search path that differs between row 0 and row k
    # would put up to 1e-9 s / 1.5e-8 = 0.07 s into a difference; at 1e-12 it is 7e-5 s, for two or three more bisection
    # levels (the bracket closes as 4^-depth).  1e-12 s is still above the rounding of a degree-40 de Casteljau split.
    TRUE_MIN_EPS_REL = 1e-12

    def _true_min_checked(self, ctx, Y):
        """The true per-pair minima of the rows Y; a search that ran out of budget raises (bezier._raise_md)"""
        return _md_checked(ctx.temporal_sep_true_min(Y, self.model['maxSep'], eps_rel=self.TRUE_MIN_EPS_REL),
                           'temporalSeparationConstraints(true_min)')

    def trueMinSeparation(self, x):
        """(val[P], t_star[P]): per pair of vehicles / point obstacles, in the order of temporalSeparationConstraints, the true
        minimum over the trajectory of the squared separation (normSquare's (d/2) factor kept) minus maxSep^2, and the
        parameter in [0, 1] where it is reached (obtg_temporal_sep_true_min) -- whatever `separationRows` is."""
        with_obs = self.pointObstacles is not None
        r = self._true_min_checked(self._ctx(with_obs), self.reshapeVector(x)[None])
        return r['val'][0], r['t_star'][0]

    # ------------------------------------------------------------------ the per-vehicle row families (_ROW_FAMILIES)
    def _bound(self, fam, what):
        """The family's bound from `model`; `what` (a public name) cannot be answered without one."""
        bound = self._operand(fam)
        if bound is None:
            raise ValueError("{} needs a bound: {} is None".format(what, fam.bound))
        return bound

    def _operand(self, fam):
        """What the family's device calls take as their bound: the value in `model` -- for the keep-in family the region's
        tables (H, VF) of `keepIn` as it is NOW (drivers edit it in place); None: not set."""
        if fam is _KEEP_OUT:
            return None if self.keepOut is None else _keep_out_tables(self.keepOut, self.model['numVeh'], self.model['dim'])
        if fam is _SEP_REGION:
            return None if self.separationRegion is None else _separation_region_table(self.separationRegion, self.model['dim'])
        if fam is _PROXIMITY:
            if self.waypoints is None and self.stayWithin is None:
                return None
            return _proximity_tables(self.waypoints, self.stayWithin, self.model['numVeh'], self.model['dim'])
        if fam is not _KEEP_IN:
            return self.model[fam.bound]
        return None if self.keepIn is None else _keep_in_tables(self.keepIn, self.model['numVeh'], self.model['dim'])

    @staticmethod
    def _check_keep_out_metric(metric, motion):
        if metric not in ('faces', 'euclidean'):
            raise ValueError("keepOutMetric must be 'faces' or 'euclidean', not {!r}".format(metric))
        if metric == 'euclidean' and motion is not None:
            raise ValueError("keepOutMetric='euclidean' together with keepOutMotion is not built: moving obstacles take the "
                             "'faces' metric")

    @staticmethod
    def _check_separation_region_metric(metric):
        if metric not in ('faces', 'euclidean'):
            raise ValueError("separationRegionMetric must be 'faces' or 'euclidean', not {!r}".format(metric))

    def _vehicle_true_min(self, fam, ctx, Y, tf, bound, what, envelope=False):
        """The family's true-minimum call on the rows Y at TRUE_MIN_EPS_REL (envelope: with the envelope blocks): its dict;
        a search that ran out of budget raises in the name of `what` (bezier._raise_md)"""
        if fam is _SEP_REGION:                                        # the vehicle pairs: one region, either metric
            self._check_separation_region_metric(self.separationRegionMetric)
            name = 'pair_keep_out_euclid_true_min' if self.separationRegionMetric != 'faces' else fam.true_min
            call = getattr(ctx, name + ('_jac' if envelope else ''))
            return _md_checked(call(Y, bound, margin=self.separationRegionMargin, eps_rel=self.TRUE_MIN_EPS_REL), what)
        if fam is _KEEP_OUT and self.keepOutMetric != 'faces':        # the Euclidean metric: the same tables, another quantity
            self._check_keep_out_metric(self.keepOutMetric, self.keepOutMotion)
            call = ctx.keep_out_euclid_true_min_jac if envelope else ctx.keep_out_euclid_true_min
            return _md_checked(call(Y, bound, margin=self.keepOutMargin, eps_rel=self.TRUE_MIN_EPS_REL), what)
        if fam is _KEEP_OUT and self.keepOutMotion is not None:       # moving obstacles: the rows of the relative curves, with tf
            call = ctx.keep_out_moving_true_min_jac if envelope else ctx.keep_out_moving_true_min
            return _md_checked(call(Y, tf, bound, self._keep_out_motion(), margin=self.keepOutMargin, eps_rel=self.TRUE_MIN_EPS_REL),
                               what)
        call = getattr(ctx, fam.envelope if envelope else fam.true_min)
        operands = (Y, tf, bound) if fam.span else (Y, bound)
        beside = {'margin': self.keepOutMargin} if fam is _KEEP_OUT else {}
        return _md_checked(call(*operands, *fam.lead, eps_rel=self.TRUE_MIN_EPS_REL, **beside), what)

    def _keep_out_motion(self):
        """The motion's tables (Q, q_off, T) of `keepOutMotion` as it is NOW, checked against the problem as the constructor does"""
        m = self.model
        return _keep_out_motion_tables(self.keepOutMotion, self.keepOut, m['dim'], m['deg'], None if self._timeopt() else m['tf'])

    def _rows_option(self, fam):
        """'all' / 'true_min': the family's rows option; a family without a `rows` method has true rows only"""
        return 'true_min' if fam.rows is None else getattr(self, fam.rows_attr)

    def _vehicle_rows(self, fam, ctx, Y, tf):
        """[B][rows]: the family's rows under its rows option -- 'all': the control points of every vehicle; 'true_min': the
        true minima, [B][N * fam.sides] -- of the rows Y on the context ctx."""
        bound = self._bound(fam, fam.constraints)
        if self._rows_option(fam) == 'true_min':
            v = self._vehicle_true_min(fam, ctx, Y, tf, bound, fam.constraints + '(true_min)')['val']
            return v.reshape(v.shape[0], -1)
        operands = (Y, tf, bound) if fam.span else (Y, bound)
        return getattr(ctx, fam.rows)(*operands, *fam.lead)

    def _vehicle_closure(self, fam):
        def direct(x):
            self._bound(fam, fam.constraints)        # a missing bound answers before anything is computed
            y = self.reshapeVector(x)
            return self._vehicle_rows(fam, self._ctx(False), y, self._tf_of(x))[0]
        return lambda x: self._serve(fam.key, x, direct)

    def _true_rows_at(self, fam, x, bound, what):
        """The true-minimum dict of the family at the one point x, under `bound` -- whatever the family's rows option is."""
        return self._vehicle_true_min(fam, self._ctx(False), self.reshapeVector(x)[None], self._tf_of(x), bound, what)

    def trueAccelMax(self, x):
        """(max_val[N], t_max[N]): per vehicle the true maximum over the trajectory of (d/2)|acceleration|^2 -- normSquare's
        factor kept: the scale of the acceleration rows, without their bound -- and the parameter in [0, 1] where it is
        reached (obtg_accel_true_min with bound 0), whatever `accelRows` is."""
        r = self._true_rows_at(_FAMILY['amax'], np.asarray(x, dtype=float), 0.0, 'trueAccelMax')
        return -r['val'][0], r['t_star'][0]

    def trueJerkMax(self, x):
        """(max_val[N], t_max[N]): per vehicle the true maximum over the trajectory of (d/2)|jerk|^2 -- normSquare's
        factor kept: the scale of the jerk rows, without their bound -- and the parameter in [0, 1] where it is
        reached (obtg_jerk_true_min with bound 0), whatever `jerkRows` is."""
        r = self._true_rows_at(_FAMILY['jmax'], np.asarray(x, dtype=float), 0.0, 'trueJerkMax')
        return -r['val'][0], r['t_star'][0]

    def trueAngularRateRows(self, x):
        """(val[N][2], t_star[N][2]): per vehicle and side the true minimum over the trajectory of maxAngRate den - num (side 0)
        and maxAngRate den + num (side 1), and the parameters in [0, 1] where they are reached (obtg_ang_rate_true_min),
        whatever `angRateRows` is: |angular rate| <= maxAngRate on the whole trajectory iff both are >= 0."""
        x = np.asarray(x, dtype=float)
        self._check_planar()
        r = self._true_rows_at(_FAMILY['ang'], x, self.model['maxAngRate'], 'trueAngularRateRows')
        return r['val'][0], r['t_star'][0]

    def trueCurvatureRange(self, x):
        """(k_min[N], t_min[N], k_max[N], t_max[N]): per vehicle the true extrema over the path of its signed curvature (left
        turns positive) and the parameters in [0, 1] where they are reached (obtg_bern_curvature at TRUE_MIN_EPS_REL),
        whatever maxCurvature is."""
        x = np.asarray(x, dtype=float)
        self._check_planar()
        Y = self.reshapeVector(x).reshape(self.model['numVeh'], 2, self.model['deg'] + 1)
        r = _md_checked(self._ctx(False).bern_curvature(Y, eps_rel=self.TRUE_MIN_EPS_REL), 'trueCurvatureRange')
        return r['k_min'], r['t_min'], r['k_max'], r['t_max']

    def trueSpaceCurvatureMax(self, x):
        """(k_max[N], t_max[N]): per vehicle of a 3-D problem the true maximum over the path of its curvature
        |c' x c''| / |c'|^3 and the parameter in [0, 1] where it is reached (obtg_bern_space_curvature at TRUE_MIN_EPS_REL),
        whatever maxSpaceCurvature is."""
        x = np.asarray(x, dtype=float)
        self._check_dimension(3)
        Y = self.reshapeVector(x).reshape(self.model['numVeh'], 3, self.model['deg'] + 1)
        r = _md_checked(self._ctx(False).bern_space_curvature(Y, eps_rel=self.TRUE_MIN_EPS_REL), 'trueSpaceCurvatureMax')
        return r['k_max'], r['t_max']

    def trueSpeedRange(self, x):
        """(min_val[N], t_min[N], max_val[N], t_max[N]): per vehicle the true extrema over the trajectory of (d/2)|dv/dt|^2
        -- normSquare's factor kept: the scale of the speed rows, without their bound -- and the parameters in [0, 1] where
        they are reached (obtg_speed_true_min with bound 0), whatever `speedRows` is."""
        x = np.asarray(x, dtype=float)
        lo, hi = (self._true_rows_at(_FAMILY[key], x, 0.0, 'trueSpeedRange') for key in ('vmin', 'vmax'))
        return lo['val'][0], lo['t_star'][0], -hi['val'][0], hi['t_star'][0]

    def _check_planar(self):
        if self.model['dim'] != 2:
            raise ValueError('The input curve must be two dimensional,\n'
                             'instead it is {} dimensional'.format(self.model['dim']))                # optimization.py:590-593

    _DIMENSION_WORDS = {3: 'three'}

    def _check_dimension(self, dim):
        if self.model['dim'] != dim:
            raise ValueError('The input curve must be {} dimensional,\n'
                             'instead it is {} dimensional'.format(self._DIMENSION_WORDS[dim], self.model['dim']))

    ARC_LENGTH_EPS_REL = 1e-12

    def _arc_length(self, ctx, Y, grad=False, what='arcLengthObjective'):
        """arc_length_obj of the rows Y at ARC_LENGTH_EPS_REL, every row's search ended (else _md_checked's exception)."""
        return _md_checked(ctx.arc_length_obj(Y, eps_rel=self.ARC_LENGTH_EPS_REL, grad=grad), what)

    def trueArcLengths(self, x):
        """len[N]: per vehicle the true length of its trajectory in space (obtg_bern_arc_length at ARC_LENGTH_EPS_REL),
        whatever the goal is; with minGoal='arcLength' they sum to the objective."""
        x = np.asarray(x, dtype=float)
        Y = self.reshapeVector(x).reshape(self.model['numVeh'], self.model['dim'], self.model['deg'] + 1)
        r = self._ctx(False).bern_arc_length(Y, eps_rel=self.ARC_LENGTH_EPS_REL)
        return _md_checked(r, 'trueArcLengths')['len']

    def _timeopt(self):
        return self.model['minGoal'].lower() == 'timeopt'

    def _tf_of(self, x):
        return x[-1] if self._timeopt() else self.model['tf']

    # ------------------------------------------------------------------ objective
    @property
    def objectiveFunction(self):
        minGoal = self.model['minGoal'].lower()
        objectivesDict = {'euclidean': self.euclideanObjective,
                          'timeopt': lambda x: x[-1],
                          'accel': self.accelObjective,
                          'jerk': self.jerkObjective,
                          'arclength': self.arcLengthObjective,
                          }
        try:
            return objectivesDict[minGoal]
        except KeyError:
            err = ('The provided minimize goal, {}, is not a valid goal. '
                   'The available minimize goals are:\n{}'
                   ).format(minGoal, objectivesDict.keys())
            raise ValueError(err)

    def _objective(self, goal, x):
        """The value of the goal (a key of _GOALS) at x, served like a constraint closure's rows."""
        g = _GOALS[goal]
        return float(self._serve(g.key, x, lambda x_: g.value(self, self._ctx(False), self.reshapeVector(x_)[None], 'arcLengthObjective')[:1])[0])

    def euclideanObjective(self, x):
        return self._objective('euclidean', x)

    def accelObjective(self, x):
        return self._objective('accel', x)

    def jerkObjective(self, x):
        return self._objective('jerk', x)

    def arcLengthObjective(self, x):
        """minGoal='arcLength' (not in the reference): the summed TRUE lengths of the vehicles' curves (obtg_arc_length_obj at
        ARC_LENGTH_EPS_REL) -- what 'euclidean', the control polygon's length, bounds from above.  Forward differences of an
        adaptive value at SciPy's step divide the rule's tolerance by 1.5e-8: pass objectiveGradient(method='exact') as jac."""
        return self._objective('arclength', x)

    def objectiveGradient(self, x, method='fd'):
        """Gradient of `objectiveFunction` the way SciPy would difference it (2-point, abs_step = sqrt(eps)), but from ONE
        batched evaluation of the n_x + 1 rows instead of n_x + 1 callbacks: pass it as `jac=` to `minimize`.  (With
        the constraint Jacobians supplied, the objective's finite differences are what is left of the per-iteration
        callback count: 17 983 of them in examples/example2_swarm_3d.py with 8 vehicles.)
        method='exact': the analytic gradient from the device (obtg_euclidean_grad / obtg_deriv_energy_grad /
        obtg_arc_length_obj's grad) instead."""
        _check_method(method)
        x = np.asarray(x, dtype=float)
        goal = self.model['minGoal'].lower()
        if goal == 'timeopt':
            g = np.zeros(x.size)
            g[-1] = 1.0
            return g
        X, dx = (x[None], None) if method == 'exact' else self._fd_rows(x)
        Y = self.reshapeVectors(X)
        c = self._ctx(False)
        if goal not in _GOALS:
            self.objectiveFunction          # raises the reference's ValueError for an unknown goal
        if method == 'exact':
            G = _GOALS[goal].grad(self, c, Y, 'objectiveGradient')[0]
            first = self._rv_parts()[1]
            return G[:, first:first + self._numCols].ravel()
        F = _GOALS[goal].value(self, c, Y, 'objectiveGradient')
        return (F[1:] - F[0]) / dx

    # ------------------------------------------------------------------ constraints
    @property
    def temporalSeparationConstraints(self):
        # (pointObstacles is read when the closure is CALLED, here as in _fd_values: a driver that sets the obstacles after
        # taking the closure gets the served rows and the one-row calls from the same context)
        def wrapper(x):
            with_obs = self.pointObstacles is not None
            if self.model['numVeh'] + (len(self.pointObstacles) if with_obs else 0) <= 1:
                return None                      # optimization.py:345-346
            return self._serve('tsep', x, direct)

        def direct(x):
            with_obs = self.pointObstacles is not None
            y = self.reshapeVector(x)
            return self._tsep_rows(self._ctx(with_obs), y)[0]
        return wrapper

    def _tsep_rows(self, ctx, Y):
        """[B][rows]: the separation rows of the rows Y under `separationRows`, on the context ctx."""
        rows = self.separationRows
        if rows == 'min':                   # per-pair minimum, reduced on the device (obtg_temporal_sep_min)
            return ctx.temporal_sep_min(Y, self.model['maxSep'])
        if rows == 'active':                 # per pair its k smallest control points, selected on the device
            return ctx.temporal_sep_active(Y, self.model['maxSep'], self._active_k())
        if rows == 'true_min':
            return self._true_min_checked(ctx, Y)['val']
        return ctx.temporal_sep(Y, self.model['maxSep'])

    @property
    def minSpeedConstraints(self):
        return self._vehicle_closure(_FAMILY['vmin'])

    @property
    def maxSpeedConstraints(self):
        return self._vehicle_closure(_FAMILY['vmax'])

    @property
    def maxAccelConstraints(self):
        """maxAccel^2 - (d/2)|acceleration|^2 >= 0: N (2n+R+1) control points (accelRows='all') or N true minima ('true_min')."""
        return self._vehicle_closure(_FAMILY['amax'])

    @property
    def maxJerkConstraints(self):
        """maxJerk^2 - (d/2)|jerk|^2 >= 0: N (2n+R+1) control points (jerkRows='all') or N true minima ('true_min')."""
        return self._vehicle_closure(_FAMILY['jmax'])

    @property
    def maxAngularRateConstraints(self):
        closure = self._vehicle_closure(_FAMILY['ang'])

        def wrapper(x):
            self._check_planar()
            y = self.reshapeVector(x)
            tf = self._tf_of(x)
            if tf <= 0:
                # an SLSQP step to tf <= 0 (time-optimal drivers without a lower bound on tf): the reference's curve
                # arithmetic returns None for an empty span (bezier.py:340-343, 365-368) and optimization.py:603-604
                # multiplies it -- the driver dies with this TypeError.  Same exception, same text, no device call.
                raise TypeError("unsupported operand type(s) for *: 'NoneType' and 'NoneType'")
            return closure(x)
        return wrapper

    @property
    def maxCurvatureConstraints(self):
        """maxCurvature -+ curvature >= 0 on the whole path: float64[2N], row 2 v + side -- side 0: maxCurvature - max(0, max
        kappa) (left turns), side 1: maxCurvature - max(0, max -kappa) (right turns); true rows (obtg_curvature_true_min), the
        same whatever tf is."""
        closure = self._vehicle_closure(_FAMILY['curv'])

        def wrapper(x):
            self._check_planar()
            return closure(x)
        return wrapper

    @property
    def maxSpaceCurvatureConstraints(self):
        """maxSpaceCurvature - curvature >= 0 on the whole path of a vehicle in space: float64[N], one true row per vehicle
        (obtg_space_curvature_true_min), the same whatever tf is."""
        closure = self._vehicle_closure(_FAMILY['scurv'])

        def wrapper(x):
            self._check_dimension(3)
            return closure(x)
        return wrapper

    @property
    def keepInConstraints(self):
        """b_f - a_f . c_v >= 0 for every (vehicle, face) of `keepIn`, vehicle-major: P (n+R+1) control points, exact linear
        constraints (keepInRows='all'; obtg_keep_in), or P true margins over the trajectory ('true_min'; obtg_keep_in_true_min)
        -- the same whatever tf is.  Not part of the one-launch structured step, of the constraint sweep, of distributed.py or
        of sequential.py."""
        return self._vehicle_closure(_KEEP_IN)

    @property
    def keepOutConstraints(self):
        """min over the trajectory of max_f (a_f . c_v - b_f) - keepOutMargin >= 0 for every (vehicle, obstacle) of `keepOut`,
        vehicle-major: N * O true rows (obtg_keep_out_true_min) -- the same whatever tf is, unless `keepOutMotion` moves an
        obstacle: then c_v is the curve relative to the obstacle's offset at the same moment, c_v(s) - q_o(s tf)
        (obtg_keep_out_moving_true_min).  Conservative near corners unless `keepOutMetric='euclidean'` (the row
        is at most the true distance minus the margin, with unit normals); negative, minus the depth, inside.  With
        `keepOutMetric='euclidean'` the rows are the signed Euclidean distance minus the margin (obtg_keep_out_euclid_true_min):
        the obstacle inflated with ROUNDED corners.  Not part of the
        one-launch structured step, of the constraint sweep, of distributed.py or of sequential.py."""
        return self._vehicle_closure(_KEEP_OUT)

    @property
    def separationRegionConstraints(self):
        """min over the trajectory of max_f (a_f . (c_i - c_j) - b_f) - separationRegionMargin >= 0 for every vehicle pair i < j,
        in the order of np.triu_indices(N, 1): N (N - 1) / 2 true rows (obtg_pair_keep_out_true_min) -- the relative curve stays
        outside `separationRegion`; negative, minus the depth, inside (vehicles at the same place: max_f (-b_f) - margin).  With
        `separationRegionMetric='euclidean'` the rows are the signed Euclidean distance to the region minus the margin
        (obtg_pair_keep_out_euclid_true_min).  The same whatever tf is.  A region with R != -R (a triangle, a box off centre)
        makes a row depend on which vehicle of the pair comes first -- the one with the smaller index; ordered pairs are not
        built.  Vehicles only: point and curve obstacles do not enter.  Not part of the one-launch structured step, of the
        constraint sweep, of distributed.py or of sequential.py."""
        return self._vehicle_closure(_SEP_REGION)

    @property
    def proximityConstraints(self):
        """One true row per entry of `waypoints` (list order), then of `stayWithin`: the maximum (waypoints) or the minimum
        (stayWithin) over the entry's window of (d/2)(radius^2 - |c_v - target|^2), >= 0 iff the vehicle comes within the Euclidean
        radius at some time of the window / never leaves it (obtg_proximity_true) -- the same whatever tf is.  Not part of the
        one-launch structured step, of the constraint sweep, of distributed.py or of sequential.py."""
        return self._vehicle_closure(_PROXIMITY)

    def spatialSeparationConstraints(self, x, robust=False):
        """All-pairs minDist over vehicles AND shape obstacles (optimization.py:109-133);
        returns shape (P, 3): (dist, t1, t2) - maxSep, as the reference does.
        robust=True: true minimum distances (obtg_min_dist_robust) instead of the reference's `_minDist`;
        pairs whose search budget runs out (curves coinciding over a stretch) report their best upper bound."""
        return self._serve('spatial_robust' if robust else 'spatial', x, lambda x_: self._spatial_direct(x_, robust))

    def _spatial_direct(self, x, robust):
        numVeh, dim, maxSep = self.model['numVeh'], self.model['dim'], self.model['maxSep']
        y = self.reshapeVector(x)
        curves = [bez.Bezier(y[i * dim:(i + 1) * dim, :]) for i in range(numVeh)] + list(self.shapeObstacles)
        n = len(curves)
        stack = [c._padded() for c in curves]
        if all(c.shape[1] == stack[0].shape[1] for c in stack):
            stack = np.stack(stack)
        pa, pb = np.triu_indices(n, 1)                              # i < j, lexicographic: the reference's pair loop
        r = _min_dist_call(stack, pa, pb, robust)
        if robust:
            return r['res'] - maxSep
        _md_checked(r)
        return r['res'] - maxSep

    def _spatial_fd_values(self, x, robust):
        """F[k + 1] = spatialSeparationConstraints(x + h e_k), F[0] at x, from ONE device call (spatialSeparationJacobian's plan:
        the base pairs and, per variable, the pairs its vehicle touches); None when a search of the call does not end -- the
        closure's own calls then say which, as they always did."""
        numVeh, dim, maxSep = self.model['numVeh'], self.model['dim'], self.model['maxSep']
        X, _ = self._fd_rows(x)
        Y = self.reshapeVectors(X)
        obstacles = list(self.shapeObstacles) if self.shapeObstacles is not None else []
        stack, pa, pb, P, t_col, t_row, t_pos = _spatial_jac_plan(Y, numVeh, dim, [c._padded() for c in obstacles])
        r = _min_dist_call(stack, pa, pb, robust)
        if not robust and np.any(r['status'] != _capi.MD_OK):
            return None
        res = r['res']
        F = np.repeat((res[:P] - maxSep)[None], X.shape[0], axis=0)          # [n_x + 1][P][3]
        F[t_col + 1, t_row] = res[t_pos] - maxSep
        return F

    def spatialSeparationJacobian(self, x, robust=False, column=None, on_cap='raise'):
        """SciPy's 2-point Jacobian of `spatialSeparationConstraints` from ONE device call.  The reference hands the
        constraint to SLSQP as it is (Examples/ComplexObstacles.py:49-63), so SciPy evaluates it n_x + 1 times, each an
        all-pairs `_minDist` sweep.  A variable of vehicle v moves only the pairs that contain v: the call carries the
        base evaluation's C(N+M, 2) pairs plus, per variable, the N+M-1 pairs of its perturbed vehicle (a trailing tf
        that moves the speed columns of every vehicle takes all their pairs) as extra curves of the same
        `obtg_min_dist` launch.  Entry for entry what n_x + 1 calls of the closure give: shape (3 P, n_x), rows in the
        order of `spatialSeparationConstraints(x).ravel()`; column=0 keeps the distance rows only, shape (P, n_x) --
        the 1-D constraint a driver would hand to SLSQP.  Statuses are treated as by the closure: a pair on which the
        reference's search does not end (depth / node caps; the reference itself recurses until Python gives up) raises;
        on_cap='nan' marks the entries of such pairs NaN instead (max_depth 128, 4 000 000 nodes per pair as in the
        closure)."""
        numVeh, dim, maxSep = self.model['numVeh'], self.model['dim'], self.model['maxSep']
        X, dx = self._fd_rows(x)
        Y = self.reshapeVectors(X)                                  # [n_x + 1][numVeh*dim][deg+1]
        nx = X.shape[1]
        obstacles = list(self.shapeObstacles) if self.shapeObstacles is not None else []
        stack, pa, pb, P, t_col, t_row, t_pos = _spatial_jac_plan(Y, numVeh, dim, [c._padded() for c in obstacles])
        r = _min_dist_call(stack, pa, pb, robust)
        res = r['res']
        if not robust:
            if on_cap == 'nan':
                res = np.where((r['status'] != 0)[:, None], np.nan, res)
            else:
                _md_checked(r)
        F0 = res[:P] - maxSep
        if column is not None:           # the one column a driver hands to SLSQP: its (P, n_x) matrix alone (a third of the zeros to write)
            J1 = np.zeros((P, nx))
            J1[t_row, t_col] = ((res[t_pos, column] - maxSep) - F0[t_row, column]) / dx[t_col]
            return J1
        J = np.zeros((P, 3, nx))
        J[t_row, :, t_col] = ((res[t_pos] - maxSep) - F0[t_row]) / dx[t_col][:, None]
        return J.reshape(3 * P, nx)

    # ------------------------------------------------------------------ batched Jacobians (new)
    def _fd_rows(self, x):
        """x and its n_x forward-difference neighbours, SciPy-style: rows[k+1] = x + h e_k,
        dx[k] = (x_k + h) - x_k."""
        x = np.asarray(x, dtype=float)
        X = np.repeat(x[None], x.size + 1, axis=0)
        idx = np.arange(x.size)
        X[idx + 1, idx] += FD_STEP
        dx = X[idx + 1, idx] - x
        return X, dx

    def _serve(self, family, x, direct):
        """A constraint closure's value at x -- from ONE batched evaluation when x is a row of SciPy's finite differences.

        The reference hands SLSQP bare closures (Examples/*.py: `{'type': 'ineq', 'fun': bezopt.temporalSeparationConstraints}`),
        so SciPy differentiates each of them itself: n_x calls at x0 + h e_k per closure and iteration, each a device launch of
        one row (Example2's five vehicles: 3112 calls per solve).  The driver stays as it is; this notices the pattern instead.
        The first call that differs from the last base point x0 in ONE variable by exactly SciPy's step is taken for row k of a
        forward difference: the closure's whole batch F(x0), F(x0 + h e_1), ... is evaluated in one launch (the rows `_jac`
        forms, formed on the device from x0), kept, and this and the following calls are answered from it.  A call at any other
        point is a new base (a line-search step, the next iterate) and drops the batches.  Values are those of the one-row call,
        element for element (tests/test_gpu_dropin.py::test_scipy_finite_differences_served_from_one_batch: SLSQP takes the same
        iterates either way).  Batches above OBTG_FD_BATCH_MB (512) per closure are not formed; steps SciPy turned around at a
        bound (x0 - h) are evaluated directly."""
        if not self.fdBatching:
            return direct(x)
        x = np.asarray(x, dtype=float)
        st = self._fd_state
        d = None
        if st is not None and st['x0'].shape == x.shape:
            d = np.flatnonzero(x != st['x0'])
            if d.size > 1 or st['key'] != self._serve_key(True):      # several variables moved, or the problem was edited: a new base
                st = None
        else:
            st = None
        if st is None:
            self.fdBatchingStats['direct'] += 1
            v = direct(x)
            # (the key after the evaluation: reshapeVector has just refreshed the model's byte key, nothing is computed twice)
            self._fd_state = {'key': self._serve_key(False), 'x0': x.copy(), 'base': {family: v}, 'rows': {}}
            return None if v is None else v.copy()
        if d.size == 0:
            if family not in st['base']:
                self.fdBatchingStats['direct'] += 1
                st['base'][family] = direct(x)
            v = st['base'][family]
            return None if v is None else v.copy()
        k = int(d[0])
        if x[k] != st['x0'][k] + FD_STEP:
            self.fdBatchingStats['direct'] += 1              # (a step turned around at a bound, or not SciPy's at all)
            return direct(x)
        rows = st['rows'].get(family)
        if rows is None:
            base = st['base'].get(family)
            if base is None:
                base = st['base'][family] = direct(st['x0'])
                self.fdBatchingStats['direct'] += 1
            limit = float(os.environ.get("OBTG_FD_BATCH_MB", "512")) * 2.0 ** 20
            if base is None or 8.0 * base.size * (x.size + 1) > limit:
                rows = st['rows'][family] = False            # (too large, or a closure without rows: evaluate directly)
            elif family.startswith('spatial'):
                rows = self._spatial_fd_values(st['x0'], family == 'spatial_robust')
                rows = st['rows'][family] = False if rows is None else rows
                self.fdBatchingStats['batches'] += rows is not False
            else:
                rows = st['rows'][family] = self._fd_values(st['x0'], family)[0]
                self.fdBatchingStats['batches'] += 1
        if rows is False:
            self.fdBatchingStats['direct'] += 1
            return direct(x)
        self.fdBatchingStats['served'] += 1
        return rows[k + 1].copy()

    def _serve_key(self, refresh):
        """What a kept batch depends on besides x: DEG_ELEV, the row options, the model (its arrays by their bytes: the key
        reshapeVector keeps; refresh = recompute it now), the bounds' values, the obstacles.  The obstacles by their BYTES on
        every call, on purpose: drivers edit `pointObstacles` / a track's control points in place between solves, which a key of
        object identities would not see (4 point obstacles: 1 us; 32 curve obstacles: 30 us beside a `_minDist` sweep of
        milliseconds); _serve asks for the key only when at most one variable moved."""
        if refresh or getattr(self, '_rv_cache', None) is None:
            self._rv_parts()
        m = self.model
        rows = [v for attr, optional in _KEY_ROWS for v in (getattr(self, attr), *[m[b] for b in optional])]
        bounds = [m[b] for b in _KEY_BOUNDS]
        tail = [(b, m[b]) for b in _KEY_TAIL if m[b] is not None]
        if self.keepIn is not None:          # the region by its tables' BYTES, as the obstacles: drivers edit it in place
            H, VF = self._operand(_KEEP_IN)
            tail.append(('keepIn', self.keepInRows, H.tobytes() + VF.tobytes()))
        if self.keepOut is not None:         # after keep-in's, likewise by the tables' bytes
            tail.append(('keepOut', self.keepOutMargin, b''.join(t.tobytes() for t in self._operand(_KEEP_OUT))))
            if self.keepOutMotion is not None:      # one more entry, only while a motion is set: its control points and spans
                tail.append(('keepOutMotion', b''.join(t.tobytes() for t in self._keep_out_motion())))
            if self.keepOutMetric != 'faces':       # one more entry, only while the metric is not the default
                tail.append(('keepOutMetric', self.keepOutMetric))
        if self.separationRegion is not None:       # one trailing entry, only while a region is set: its bytes, margin and metric
            tail.append(('separationRegion', self._operand(_SEP_REGION).tobytes(), self.separationRegionMargin,
                         self.separationRegionMetric))
        if self.waypoints is not None or self.stayWithin is not None:      # one trailing entry, only while a list is set
            tail.append(('proximity', b''.join(t.tobytes() for t in self._operand(_PROXIMITY))))
        return (int(DEG_ELEV), self.separationRows, *rows, self.activeRows, self._rv_cache[0], self.model['maxSep'], *bounds,
                None if self._timeopt() else self.model['tf'],
                None if self.pointObstacles is None else np.asarray(self.pointObstacles, dtype=float).tobytes(),
                None if self.shapeObstacles is None else tuple(np.asarray(c.cpts, dtype=float).tobytes() for c in self.shapeObstacles),
                *tail)

    def _jac(self, x, family):
        F, dx = self._fd_values(x, family)
        return ((F[1:] - F[0:1]) / dx[:, None]).T

    def _fd_values(self, x, family):
        """(F, dx): the closure `family` on x and its n_x forward-difference neighbours, F[k + 1] = closure(x + h e_k), in one
        batched device call."""
        X, dx = self._fd_rows(x)
        Y = self.reshapeVectors(X)
        fam = _FAMILY.get(family)
        if fam is not None:
            tf = X[:, -1] if self._timeopt() else np.full(X.shape[0], self.model['tf'])
            return self._vehicle_rows(fam, self._ctx(False), Y, tf), dx
        if family == 'tsep':
            return self._tsep_rows(self._ctx(self.pointObstacles is not None), Y), dx
        F = _GOAL_OF_KEY[family].value(self, self._ctx(False), Y, 'arcLengthObjective')      # (one value per row; a column here)
        return np.asarray(F, dtype=float).reshape(-1, 1), dx

    def temporalSeparationJacobian(self, x, structured=True, method='fd'):
        """d(temporalSeparationConstraints)/dx by SciPy-style forward differences.

        structured=True: a variable of vehicle v only moves the N-1 pairs
        that contain v, so only those pairs are re-evaluated (obtg_temporal_sep_fd) and the dense
        matrix is assembled from them; every entry equals the brute-force batch's
        (structured=False) bit for bit.  Variables that move every vehicle (tf with prescribed
        speeds) and shapes outside the specialised kernels take the batch path.

        method='exact': the analytic Jacobian (obtg_temporal_sep_jac, one launch at x; `structured` is ignored).  With
        separationRows 'min' / 'active' its rows are those of the control points the value kernels select at x.

        method='envelope' (separationRows='true_min' only): the envelope derivative of the true per-pair minima -- the
        derivative of each pair's polynomial at the minimiser the search returns (obtg_temporal_sep_true_min_jac, one call
        at x with TRUE_MIN_EPS_REL; DESIGN.md 4.14 says what it is where minimisers tie)."""
        if method == 'envelope':
            if self.separationRows != 'true_min':
                raise ValueError("temporalSeparationJacobian(method='envelope') needs separationRows='true_min', not {!r}"
                                 .format(self.separationRows))
            return self._temporal_sep_jac_envelope(x)
        _check_method(method)
        if method == 'exact':
            if self.separationRows == 'true_min':
                raise ValueError("temporalSeparationJacobian(method='exact') is not available with separationRows='true_min' "
                                 "(the envelope derivative is not built under that name): use method='envelope' or method='fd'")
            return self._temporal_sep_jac_exact(x)
        if not structured or self.separationRows in ('active', 'true_min'):
            # 'active': the forward differences of the order statistics themselves -- what SciPy builds from n_x + 1 calls
            # of the closure -- from one batched call (k values per pair and row leave the device, not 2n+R+1)
            return self._jac(x, 'tsep')
        x = np.asarray(x, dtype=float)
        X, dx = self._fd_rows(x)
        with_obs = self.pointObstacles is not None
        ctx = self._ctx(with_obs)
        n_obj = ctx.n_veh + ctx.n_obs
        if n_obj < 2:
            return self._jac(x, 'tsep')
        dim, numCols = self.model['dim'], self._numCols
        n_pts = self.model['numVeh'] * dim * numCols          # control-point variables; a trailing tf is not one
        offset = (self.model['deg'] + 1 - numCols) // 2
        Y0 = self.reshapeVectors(x[None])[0]
        k = np.arange(n_pts)
        prow, pcol = k // numCols, offset + k % numCols
        try:
            blk = ctx.temporal_sep_fd(Y0, prow, pcol, X[k + 1, k], self.model['maxSep'])
        except _capi.ObtgError:
            return self._jac(x, 'tsep')
        F0 = ctx.temporal_sep(Y0[None], self.model['maxSep'])[0]
        LR = blk.shape[2]
        reduced = self.separationRows == 'min'
        if reduced:
            # forward differences of the per-pair minimum itself: min over the perturbed pair's control points minus
            # min over the unperturbed ones -- exactly what SciPy would form from n_x + 1 calls of the 'min' closure
            blk = blk.min(axis=2, keepdims=True)
            F0 = F0.reshape(-1, LR).min(axis=1)
            LR = 1
        J = np.zeros((F0.size, x.size))
        veh = prow // dim
        partners = np.arange(n_obj - 1)[None, :] + (np.arange(n_obj - 1)[None, :] >= veh[:, None])   # [n_pts][n_obj-1]
        lo, hi = np.minimum(veh[:, None], partners), np.maximum(veh[:, None], partners)
        pidx = lo * n_obj - lo * (lo + 1) // 2 + (hi - lo - 1)                                        # lexicographic pair index
        rows = pidx[:, :, None] * LR + np.arange(LR)[None, None, :]
        J[rows.reshape(n_pts, -1), k[:, None]] = (blk - F0[rows]).reshape(n_pts, -1) / dx[:n_pts, None]
        if x.size > n_pts:      # tf: moves columns 1 / -2 of every vehicle when speeds are prescribed
            Yt = self.reshapeVectors(X[n_pts + 1:])
            Ft = self._tsep_rows(ctx, Yt)                   # ('all' or 'min' here)
            J[:, n_pts:] = ((Ft - F0[None]) / dx[n_pts:, None]).T
        return J

    def _jac_vehicle(self, x, family, structured=True, method='fd'):
        """Per-vehicle families (speed, angular rate): the Jacobian is block diagonal -- a control
        point of vehicle v only moves v's own rows.  structured=True evaluates, per variable, that one
        vehicle (a compact batch on a one-vehicle context: n_x vehicle evaluations instead of
        n_x N); entries equal the brute-force batch's bit for bit.  A trailing tf moves everything and
        takes the batch path.  method='exact': the analytic blocks (obtg_speed_jac / obtg_ang_rate_jac, one launch at x; not
        built for the acceleration and jerk rows).

        With the family's rows option 'true_min': method='envelope' is the envelope derivative of the true per-vehicle minima
        -- each row's polynomial differentiated at the minimiser the search returns, with its d/dtf (obtg_<family>_true_min_jac,
        one call at x with TRUE_MIN_EPS_REL; dense [N * sides][n_x]); method='fd' differences the search
        itself (one batched call); method='exact' is not built for these rows.  _check_jac_method says which of them raise."""
        fam = _FAMILY[family]
        true_min = self._check_jac_method(fam, method)
        if method == 'envelope':
            return self._jac_vehicle_envelope(x, fam)
        if method == 'exact':
            return self._jac_vehicle_exact(x, fam)
        if not structured or true_min:
            return self._jac(x, family)
        x = np.asarray(x, dtype=float)
        X, dx = self._fd_rows(x)
        dim, numCols, numVeh = self.model['dim'], self._numCols, self.model['numVeh']
        n_pts = numVeh * dim * numCols
        offset = (self.model['deg'] + 1 - numCols) // 2
        Y0 = self.reshapeVectors(x[None])[0]
        tf0 = float(self._tf_of(x))

        def evaluate(ctx, Y, tf):                                 # (the control-point rows here)
            return self._vehicle_rows(fam, ctx, Y, tf)

        F0 = evaluate(self._ctx(False), Y0[None], np.array([tf0]))[0]
        per = F0.size // numVeh
        k = np.arange(n_pts)
        prow, pcol = k // numCols, offset + k % numCols
        veh = prow // dim
        Yc = Y0.reshape(numVeh, dim, -1)[veh].copy()              # [n_pts][dim][deg+1]: the touched vehicle of each variable
        Yc[k, prow % dim, pcol] = X[k + 1, k]
        Fc = evaluate(self._ctx_one(), Yc, np.full(n_pts, tf0))   # [n_pts][per]
        J = np.zeros((F0.size, x.size))
        rows = veh[:, None] * per + np.arange(per)[None, :]
        J[rows, k[:, None]] = (Fc - F0[rows]) / dx[:n_pts, None]
        if x.size > n_pts:
            Xt = X[n_pts + 1:]
            Ft = evaluate(self._ctx(False), self.reshapeVectors(Xt), Xt[:, -1])
            J[:, n_pts:] = ((Ft - F0[None]) / dx[n_pts:, None]).T
        return J

    def maxSpeedJacobian(self, x, structured=True, method='fd'):
        return self._jac_vehicle(x, 'vmax', structured, method)

    def minSpeedJacobian(self, x, structured=True, method='fd'):
        return self._jac_vehicle(x, 'vmin', structured, method)

    def maxAngularRateJacobian(self, x, structured=True, method='fd'):
        return self._jac_vehicle(x, 'ang', structured, method)

    def maxAccelJacobian(self, x, structured=True, method='fd'):
        return self._jac_vehicle(x, 'amax', structured, method)

    def maxJerkJacobian(self, x, structured=True, method='fd'):
        return self._jac_vehicle(x, 'jmax', structured, method)

    def maxCurvatureJacobian(self, x, structured=True, method='fd'):
        """d(maxCurvatureConstraints)/dx, dense [2N][n_x]: method='fd' differences the search (one batched call),
        method='envelope' is the derivative of each row at the parameter its search returns (obtg_curvature_true_min_jac; zero
        for a row that is maxCurvature itself).  The rows have no explicit dependence on tf: that part of a time-optimal
        problem's tf column is an exact 0 (with prescribed speeds the column still carries dY/dtf)."""
        return self._jac_vehicle(x, 'curv', structured, method)

    def maxSpaceCurvatureJacobian(self, x, structured=True, method='fd'):
        """d(maxSpaceCurvatureConstraints)/dx, dense [N][n_x]: method='fd' differences the search (one batched call),
        method='envelope' is the derivative of each row at the parameter its search returns
        (obtg_space_curvature_true_min_jac; zero for a row that is maxSpaceCurvature itself).  The rows have no explicit
        dependence on tf: that part of a time-optimal problem's tf column is an exact 0 (with prescribed speeds the column
        still carries dY/dtf)."""
        return self._jac_vehicle(x, 'scurv', structured, method)

    def keepInJacobian(self, x, structured=True, method='fd'):
        """d(keepInConstraints)/dx, dense [rows][n_x]: method='fd' differences the closure's rows (one batched call; the rows
        are linear in x, `structured` changes nothing); method='envelope' (keepInRows='true_min') is the derivative of each true
        margin at the parameter its search returns (obtg_keep_in_true_min_jac, one call at x), scattered to the columns of the
        item's own vehicle; method='exact' is not built.  The rows have no explicit dependence on tf: that part of a
        time-optimal problem's tf column is an exact 0 (with prescribed speeds the column still carries dY/dtf)."""
        fam = _KEEP_IN
        region = self._bound(fam, fam.jacobian)          # a missing region answers before anything is computed
        self._check_jac_method(fam, method)
        if method != 'envelope':
            return self._jac(x, fam.key)
        x = np.asarray(x, dtype=float)
        r = self._vehicle_true_min(fam, self._ctx(False), self.reshapeVectors(x[None]), None, region, fam.jacobian + '(envelope)',
                                   envelope=True)
        owner = region[1][:, 0].astype(np.int64)
        return self._scatter_exact(r['jac'][0][:, None], (owner,), (1.0,), np.zeros((owner.size, 1)))      # blocks of one row each

    def trueKeepInMargins(self, x):
        """(val[P], t_star[P]): per (vehicle, face) of `keepIn`, in the order of keepInConstraints, the true minimum over the
        trajectory of b_f - a_f . c_v and the parameter in [0, 1] where it is reached (obtg_keep_in_true_min), whatever
        `keepInRows` is: the vehicle stays inside iff every one is >= 0."""
        region = self._bound(_KEEP_IN, 'trueKeepInMargins')
        r = self._true_rows_at(_KEEP_IN, np.asarray(x, dtype=float), region, 'trueKeepInMargins')
        return r['val'][0], r['t_star'][0]

    def keepOutJacobian(self, x, structured=True, method='fd'):
        """d(keepOutConstraints)/dx, dense [N * O][n_x]: method='fd' differences the closure's rows (one batched call;
        `structured` changes nothing); method='envelope' is the derivative of each row at the parameter and the active faces its
        search returns -- one face at an end or a smooth minimum, the weighted pair at a kink (obtg_keep_out_true_min_jac, one
        call at x) -- scattered to the columns of the item's own vehicle; method='exact' is not built.  The rows have no explicit
        dependence on tf: that part of a time-optimal problem's tf column is an exact 0 (with prescribed speeds the column still
        carries dY/dtf).  With `keepOutMotion` the rows are those of the relative curves (obtg_keep_out_moving_true_min[_jac])
        and DO depend on tf: the envelope's tf column then carries the kernel's jac_tf = -(a^ . E'(t*)) t* / tf as well."""
        fam = _KEEP_OUT
        tables = self._bound(fam, fam.jacobian)          # missing obstacles answer before anything is computed
        self._check_jac_method(fam, method)
        if method != 'envelope':
            return self._jac(x, fam.key)
        x = np.asarray(x, dtype=float)
        moving = self.keepOutMotion is not None
        r = self._vehicle_true_min(fam, self._ctx(False), self.reshapeVectors(x[None]), np.atleast_1d(self._tf_of(x)) if moving else None,
                                   tables, fam.jacobian + '(envelope)', envelope=True)
        owner = tables[2][:, 0].astype(np.int64)
        # (blocks of one row each; against moving obstacles the rows have an explicit d/dtf, the kernel's jac_tf)
        dtf = r['jac_tf'][0][:, None] if moving else np.zeros((owner.size, 1))
        return self._scatter_exact(r['jac'][0][:, None], (owner,), (1.0,), dtf)

    def trueKeepOutClearances(self, x):
        """dict(val[P], t_star[P], face[P][2], lam[P], status[P]): per (vehicle, obstacle) of `keepOut`, in the order of
        keepOutConstraints, the row (clearance minus keepOutMargin), the parameter in [0, 1] where it is reached, the active
        faces as indices into the stacked face table (the second -1 without one), the first face's weight and the search's
        status (obtg_keep_out_true_min): the vehicles stay clear iff every val is >= 0.  With keepOutMetric='euclidean':
        dict(val[P], t_star[P], faces[P][3], dir[P][dim], status[P]) -- the Euclidean clearance minus keepOutMargin, the active
        set (-1 padded) and the unit direction from the obstacle's nearest point to the trajectory there
        (obtg_keep_out_euclid_true_min)."""
        tables = self._bound(_KEEP_OUT, 'trueKeepOutClearances')
        r = self._true_rows_at(_KEEP_OUT, np.asarray(x, dtype=float), tables, 'trueKeepOutClearances')
        if self.keepOutMetric != 'faces':
            return {k: r[k][0] for k in ('val', 't_star', 'faces', 'dir', 'status')}
        return {k: r[k][0] for k in ('val', 't_star', 'face', 'lam', 'status')}

    def separationRegionJacobian(self, x, structured=True, method='fd'):
        """d(separationRegionConstraints)/dx, dense [N (N - 1) / 2][n_x]: method='fd' differences the closure's rows (one batched
        call; `structured` changes nothing); method='envelope' is the derivative of each row at the parameter and the active faces
        (Euclidean metric: the direction) its search returns (obtg_pair_keep_out[_euclid]_true_min_jac, one call at x): the block
        of the pair's first vehicle, scattered with +1 to its columns and with -1 to the second vehicle's; method='exact' is not
        built.  The rows have no explicit dependence on tf: that part of a time-optimal problem's tf column is an exact 0 (with
        prescribed speeds the column still carries dY/dtf)."""
        fam = _SEP_REGION
        region = self._bound(fam, fam.jacobian)          # a missing region answers before anything is computed
        self._check_jac_method(fam, method)
        if method != 'envelope':
            return self._jac(x, fam.key)
        x = np.asarray(x, dtype=float)
        r = self._vehicle_true_min(fam, self._ctx(False), self.reshapeVectors(x[None]), None, region, fam.jacobian + '(envelope)',
                                   envelope=True)
        pa, pb = np.triu_indices(self.model['numVeh'], 1)
        return self._scatter_exact(r['jac'][0][:, None], (pa, pb), (1.0, -1.0))      # blocks of one row each

    def trueSeparationRegionClearances(self, x):
        """dict(val[P], t_star[P], face[P][2], lam[P], status[P]): per vehicle pair, in the order of separationRegionConstraints,
        the row (clearance of c_i - c_j from the region minus separationRegionMargin), the parameter in [0, 1] where it is
        reached, the active faces of the region (the second -1 without one), the first face's weight and the search's status
        (obtg_pair_keep_out_true_min).  With separationRegionMetric='euclidean': dict(val[P], t_star[P], faces[P][3], dir[P][dim],
        status[P]) (obtg_pair_keep_out_euclid_true_min)."""
        region = self._bound(_SEP_REGION, 'trueSeparationRegionClearances')
        r = self._true_rows_at(_SEP_REGION, np.asarray(x, dtype=float), region, 'trueSeparationRegionClearances')
        if self.separationRegionMetric != 'faces':
            return {k: r[k][0] for k in ('val', 't_star', 'faces', 'dir', 'status')}
        return {k: r[k][0] for k in ('val', 't_star', 'face', 'lam', 'status')}

    def proximityJacobian(self, x, structured=True, method='fd'):
        """d(proximityConstraints)/dx, dense [P][n_x]: method='fd' differences the closure's rows (one batched call; `structured`
        changes nothing); method='envelope' is the derivative of each row's polynomial at the parameter its search returns
        (obtg_proximity_true_jac, one call at x): the block of the entry's vehicle, scattered with +1 to its columns and, when
        the target is a vehicle, with -1 to that vehicle's (a point has no variable); method='exact' is not built.  The rows
        have no explicit dependence on tf: that part of a time-optimal problem's tf column is an exact 0 (with prescribed speeds
        the column still carries dY/dtf)."""
        fam = _PROXIMITY
        tables = self._bound(fam, fam.jacobian)          # missing lists answer before anything is computed
        self._check_jac_method(fam, method)
        if method != 'envelope':
            return self._jac(x, fam.key)
        x = np.asarray(x, dtype=float)
        r = self._vehicle_true_min(fam, self._ctx(False), self.reshapeVectors(x[None]), None, tables, fam.jacobian + '(envelope)',
                                   envelope=True)
        items = tables[0].astype(np.int64)
        return self._scatter_exact(r['jac'][0][:, None], (items[:, 0], items[:, 1]), (1.0, -1.0))      # blocks of one row each

    def trueProximityMargins(self, x):
        """(val[P], t_star[P]): per entry of `waypoints`, then of `stayWithin`, in the order of proximityConstraints, the row --
        (d/2)(radius^2 - distance^2) at the closest approach (waypoints) or at the farthest point (stayWithin) of its window -- and
        the parameter in [0, 1] where it is attained (obtg_proximity_true): every entry holds iff every val is >= 0."""
        tables = self._bound(_PROXIMITY, 'trueProximityMargins')
        r = self._true_rows_at(_PROXIMITY, np.asarray(x, dtype=float), tables, 'trueProximityMargins')
        return r['val'][0], r['t_star'][0]

    # ------------------------------------------------------------------ exact Jacobians (method='exact')
    # The device returns d rows / d Y per pair or vehicle ([..][rows][dim][deg+1] blocks, include/obtg.h obtg_*_jac); the chain
    # rule to x keeps the free columns, and for a time-optimal problem adds the tf column: the explicit d/dtf of the speed and
    # angular-rate rows plus, with prescribed speeds, the rows' derivative along dY/dtf (columns 1 and -2, reshapeVectors).
    def _dY_dtf(self):
        """dY/dtf [numVeh*dim][deg+1]: nonzero in columns 1 and -2 when speeds are prescribed (p0 + (v0 tf / deg) (cos, sin))."""
        template, _, headings = self._rv_parts()
        D = np.zeros(template.shape)
        if headings is not None:
            deg = self.model['deg']
            for col, (speed, _px, _py, c, s) in ((1, headings[0]), (-2, headings[1])):
                D[0::2, col] = speed * c / deg
                D[1::2, col] = speed * s / deg
        return D

    def _scatter_exact(self, blk, owner, sign, dtf=None):
        """Dense J [K * rows][n_x] from blocks blk[K][rows][dim][deg+1]: block k is the derivative of its rows with respect to
        the control points of vehicle owner[j][k], times sign[j] (j over the block's sides; owner >= numVeh: a point obstacle,
        no variable).  dtf[K][rows]: the explicit d/dtf of the rows (time-optimal problems)."""
        numVeh, dim, numCols = self.model['numVeh'], self.model['dim'], self._numCols
        first = self._rv_parts()[1]
        K, rows = blk.shape[:2]
        free = blk[..., first:first + numCols].reshape(K, rows, dim * numCols)
        J4 = np.zeros((K, rows, numVeh, dim * numCols))
        kk = np.arange(K)
        for own, sg in zip(owner, sign):
            m = own < numVeh
            J4[kk[m], :, own[m], :] += sg * free[m]
        J = J4.reshape(K * rows, numVeh * dim * numCols)
        if not self._timeopt():
            return J
        D = np.zeros((numVeh + 1, dim, blk.shape[3]))
        D[:numVeh] = self._dY_dtf().reshape(numVeh, dim, -1)
        Dk = sum(sg * D[np.minimum(own, numVeh)] for own, sg in zip(owner, sign))   # [K][dim][deg+1]
        t = np.einsum('krci,kci->kr', blk, Dk)
        if dtf is not None:
            t = t + dtf
        return np.hstack((J, t.reshape(-1, 1)))

    def _temporal_sep_jac_exact(self, x):
        x = np.asarray(x, dtype=float)
        with_obs = self.pointObstacles is not None
        ctx = self._ctx(with_obs)
        n_obj = ctx.n_veh + ctx.n_obs
        if n_obj < 2:
            return np.zeros((0, x.size))
        Y0 = self.reshapeVectors(x[None])
        blk = ctx.temporal_sep_jac(Y0)[0]                                   # [P][2n+R+1][dim][deg+1]
        P = blk.shape[0]
        if self.separationRows in ('min', 'active'):
            k = 1 if self.separationRows == 'min' else self._active_k()
            val, idx = ctx.temporal_sep_active(Y0, self.model['maxSep'], k, with_index=True)
            blk = blk[np.arange(P)[:, None], idx[0].reshape(P, k)]
            # a pair with a non-finite element has NaN rows (include/obtg.h, "Non-finite control points") and no control point
            # that they follow: its derivative is NaN in the columns of its own vehicles, not the one of control points 0 .. k-1
            blk[np.isnan(val[0].reshape(P, k))] = np.nan
        pa, pb = np.triu_indices(n_obj, 1)
        return self._scatter_exact(blk, (pa, pb), (1.0, -1.0))

    def _temporal_sep_jac_envelope(self, x):
        x = np.asarray(x, dtype=float)
        with_obs = self.pointObstacles is not None
        ctx = self._ctx(with_obs)
        n_obj = ctx.n_veh + ctx.n_obs
        if n_obj < 2:
            return np.zeros((0, x.size))
        r = ctx.temporal_sep_true_min_jac(self.reshapeVectors(x[None]), self.model['maxSep'], eps_rel=self.TRUE_MIN_EPS_REL)
        _md_checked(r, 'temporalSeparationJacobian(envelope)')
        pa, pb = np.triu_indices(n_obj, 1)
        return self._scatter_exact(r['jac'][0][:, None], (pa, pb), (1.0, -1.0))      # blocks of one row each

    def _check_jac_method(self, fam, method):
        """Whether the family's Jacobian provider can answer `method` under the family's rows option -- the same order of
        checks for every family; what cannot be answered raises.  Returns whether the rows are the true minima."""
        rows = self._rows_option(fam)
        true_min = rows == 'true_min'
        if fam.only_dim is not None:
            self._check_dimension(fam.only_dim)
        if fam.planar and (method == 'envelope' or true_min):      # (control-point rows of another dimension: the device call answers)
            self._check_planar()
        if method == 'envelope':
            if not true_min:
                raise ValueError("{}(method='envelope') needs {}='true_min', not {!r}".format(fam.jacobian, fam.rows_attr, rows))
            return true_min
        _check_method(method)
        if method == 'exact':
            if fam.exact is None and fam.rows is None:
                raise ValueError("{}(method='exact') is not built for the {} rows: use method='fd' or method='envelope'"
                                 .format(fam.jacobian, fam.noun))
            if fam.exact is None:
                raise ValueError("{}(method='exact') is not built for the {} rows: use method='fd' or, with {}='true_min', "
                                 "method='envelope'".format(fam.jacobian, fam.noun, fam.rows_attr))
            if true_min:
                raise ValueError("{}(method='exact') is not available with {}='true_min' (the envelope derivative is not built "
                                 "under that name): use method='envelope' or method='fd'".format(fam.jacobian, fam.rows_attr))
        elif fam.optional:
            self._bound(fam, fam.jacobian)
        return true_min

    def _jac_vehicle_envelope(self, x, fam):
        x = np.asarray(x, dtype=float)
        ctx = self._ctx(False)
        Y0, tf = self.reshapeVectors(x[None]), float(self._tf_of(x))
        r = self._vehicle_true_min(fam, ctx, Y0, tf, self._bound(fam, fam.jacobian), fam.jacobian + '(envelope)', envelope=True)
        N = self.model['numVeh']
        blk = r['jac'][0].reshape((N, fam.sides) + r['jac'].shape[-2:])            # blocks of fam.sides rows each
        dtf = r['jac_tf'][0].reshape(N, fam.sides) if fam.span else np.zeros((N, fam.sides))
        return self._scatter_exact(blk, (np.arange(N),), (1.0,), dtf)

    def trueMinSeparationJacobian(self, x):
        """temporalSeparationJacobian(x, method='envelope')"""
        return self.temporalSeparationJacobian(x, method='envelope')

    def _jac_vehicle_exact(self, x, fam):
        x = np.asarray(x, dtype=float)
        Y0 = self.reshapeVectors(x[None])
        tf = float(self._tf_of(x))
        c = self._ctx(False)
        if fam.planar:
            self._check_planar()
        blk, dtf = getattr(c, fam.exact)(Y0, tf, *fam.lead)
        N = self.model['numVeh']
        return self._scatter_exact(blk[0], (np.arange(N),), (1.0,), dtf[0])

    # ------------------------------------------------------------------ x <-> y
    def generateGuess(self, std=0, seed=None):
        """Straight-line initial guess with N(0, std^2) noise (optimization.py:189-240), all vehicles at once.
        One `randn` draw of numVeh*dim*len values consumes NumPy's legacy stream in the order the reference's
        per-row draws do, so a given `seed` yields the reference's guess."""
        m = self.model
        numVeh, dim, deg = m['numVeh'], m['dim'], m['deg']
        start = np.asarray(m['initPoints'], dtype=float)[:numVeh]
        stop = np.asarray(m['finalPoints'], dtype=float)[:numVeh]
        npts = deg + 1
        if m['initSpeeds'][0] is not None:
            if dim != 2:
                raise ValueError('The dimension must be 2 for initial and final speeds and angles.')
            # prescribed speeds pin the second and the second-to-last control point: the line runs between those
            heading0 = np.stack((np.cos(m['initAngs']), np.sin(m['initAngs'])), axis=1)
            heading1 = np.stack((np.cos(m['finalAngs']), np.sin(m['finalAngs'])), axis=1)
            start = start + (np.asarray(m['initSpeeds'], dtype=float) * m['tf'] / deg)[:, None] * heading0
            stop = stop - (np.asarray(m['finalSpeeds'], dtype=float) * m['tf'] / deg)[:, None] * heading1
            npts = deg - 1
        np.random.seed(seed)
        # row by row: np.linspace with array end points switches formula when ANY row has start == stop, which
        # would move the other rows' last bits away from the reference's scalar calls
        lines = np.array([np.linspace(a, b, npts) for a, b in zip(start.ravel(), stop.ravel())])
        lines += np.random.randn(numVeh * dim, npts) * std
        guess = lines[:, 1:-1].reshape(-1)
        return np.append(guess, m['tf']) if self._timeopt() else guess

    def reshapeVector(self, x):
        """x -> y[(numVeh*dim) x (deg+1)] (optimization.py:242-285).

        SLSQP calls this once per callback, and at Example1's size a dozen small NumPy operations cost more than the
        device call they feed (23 us).  Everything that does not depend on x -- end points, the headings' sines and
        cosines -- is worked out once per problem (`_rv_parts`); a call copies that template, sets the two speed
        columns from tf and drops x into the free columns: 8 us.  `reshapeVectors` is the same thing with a leading
        batch axis (one row per finite-difference neighbour of x)."""
        return self.reshapeVectors(x)

    def reshapeVectors(self, X):
        """X[B][n_x] -> Y[B][numVeh*dim][deg+1] (any number of leading axes, none included): the template broadcast
        over the rows."""
        template, first_free, headings = self._rv_parts()
        X = np.asarray(X, dtype=float)
        if self._timeopt():                                   # time-optimal problems carry tf as the last variable
            tf, X = (X[..., -1:] if X.ndim > 1 else X[-1]), X[..., :-1]
        else:
            tf = float(self.model['tf'])
        lead = X.shape[:-1]
        if lead:
            Y = np.empty(lead + template.shape)
            Y[...] = template
        else:
            Y = template.copy()
        if headings is not None:
            # the second / second-to-last control points realise the prescribed speeds: p0 + (v0 tf / deg) (cos, sin)
            # and pf - (vf tf / deg) (cos, sin); even rows of y are x coordinates, odd rows y coordinates
            deg = self.model['deg']
            for col, (speed, px, py, c, s) in ((1, headings[0]), (-2, headings[1])):
                reach = speed * tf / deg                      # [...][numVeh]; the final end's cos / sin carry the minus
                Y[..., 0::2, col] = px + reach * c
                Y[..., 1::2, col] = py + reach * s
        Y[..., first_free:template.shape[1] - first_free] = X.reshape(lead + (template.shape[0], self._numCols))
        return Y

    def _rv_parts(self):
        """(template of y with its constant columns set, index of the first free column, per end of the curve
        (speed, x, y, cos, sin) or None) -- rebuilt when the problem's `model` entries change."""
        m = self.model
        fields = [m[k] for k in ('initPoints', 'finalPoints', 'initSpeeds', 'finalSpeeds', 'initAngs', 'finalAngs')]
        key = (m['numVeh'], m['dim'], m['deg']) + tuple(a.tobytes() if a.dtype != object else id(a) for a in fields)
        cached = getattr(self, '_rv_cache', None)
        if cached is not None and cached[0] == key:
            return cached[1]
        p0, pf, v0, vf, a0, af = fields
        dim = m['dim']
        # atleast_2d(None) is an object array: like the reference, a problem without end points fails on its first
        # reshape (optimization.py:267-271 assigns None into y) -- float() raises the same TypeError here
        p0, pf = p0.astype(float), pf.astype(float)
        template = np.empty((dim * m['numVeh'], m['deg'] + 1))
        rows = p0.shape[0] * dim
        template[:rows, 0] = p0.reshape(-1)[:rows]
        template[:rows, -1] = pf.reshape(-1)[:rows]
        first_free, headings = 1, None
        if v0[0] is not None:
            first_free = 2
            headings = ((v0.astype(float), p0[:, 0].copy(), p0[:, 1].copy(), np.cos(a0), np.sin(a0)),
                        (vf.astype(float), pf[:, 0].copy(), pf[:, 1].copy(), -np.cos(af), -np.sin(af)))
        self._rv_cache = (key, (template, first_free, headings))
        return self._rv_cache[1]
