"""The Python layer's family table (optimization._ROW_FAMILIES, _GOALS, _tsep_rows), without a device.

Two things a table can get wrong, and nothing else checks without a GPU:
  * the refusals -- which (provider, method, rows option, bound, dimension) is answered in Python before any device call, with
    which exception and which text: REFUSALS holds the texts of the commit before the table, written out;
  * the routing -- which _capi.Context method a family's closure, its _fd_values and its Jacobian provider call, with which
    bound of `model`, which leading flags and which eps_rel: ROUTES holds them, written out, and a recording stand-in for
    _capi.Context notes what is really called.
"""
import itertools

import numpy as np
import pytest

from optimalbeziertrajectorygeneration_amd import optimization as opt


class Recorder(object):
    """Stands in for _capi.Context: every call returns zeros of the real call's shape and leaves
    (method, bound, flags, eps_rel) in Recorder.log."""
    log = []

    def __init__(self, n_veh, dim, deg, deg_elev=0, point_obs=None, device=0):
        self.n_veh, self.dim, self.deg, self.deg_elev = n_veh, dim, deg, int(deg_elev)
        self.n_obs = 0 if point_obs is None else len(point_obs)

    def set_ang_rate_order(self, code):
        pass

    def set_deg_elev(self, R):
        self.deg_elev = int(R)

    @property
    def num_pairs(self):
        n = self.n_veh + self.n_obs
        return n * (n - 1) // 2

    def _note(self, Y, method, bound=None, flags=(), eps_rel=None):
        Recorder.log.append((method, bound, tuple(flags), eps_rel))
        return np.asarray(Y).size // (self.n_veh * self.dim * (self.deg + 1)), 2 * self.deg + self.deg_elev + 1

    def _search(self, shape, blocks=()):
        r = dict(val=np.zeros(shape), t_star=np.zeros(shape), status=np.zeros(shape, np.int32))
        if 'jac' in blocks:
            r['jac'] = np.zeros(shape + (self.dim, self.deg + 1))
        if 'jac_tf' in blocks:
            r['jac_tf'] = np.zeros(shape)
        return r

    # -- separation
    def temporal_sep(self, Y, max_sep):
        B, L = self._note(Y, 'temporal_sep', max_sep)
        return np.zeros((B, self.num_pairs * L))

    def temporal_sep_min(self, Y, max_sep):
        B, _ = self._note(Y, 'temporal_sep_min', max_sep)
        return np.zeros((B, self.num_pairs))

    def temporal_sep_active(self, Y, max_sep, k, with_index=False):
        B, _ = self._note(Y, 'temporal_sep_active', max_sep, (k,))
        out = np.zeros((B, self.num_pairs * k))
        return (out, np.zeros(out.shape, np.int32)) if with_index else out

    def temporal_sep_true_min(self, Y, max_sep, eps_rel=1e-9):
        B, _ = self._note(Y, 'temporal_sep_true_min', max_sep, (), eps_rel)
        return self._search((B, self.num_pairs))

    def temporal_sep_true_min_jac(self, Y, max_sep, eps_rel=1e-9):
        B, _ = self._note(Y, 'temporal_sep_true_min_jac', max_sep, (), eps_rel)
        return self._search((B, self.num_pairs), ('jac',))

    def temporal_sep_fd(self, Y0, pert_row, pert_col, pert_val, max_sep):
        _, L = self._note(Y0, 'temporal_sep_fd', max_sep)
        return np.zeros((len(pert_row), self.n_veh + self.n_obs - 1, L))

    def temporal_sep_jac(self, Y):
        B, L = self._note(Y, 'temporal_sep_jac')
        return np.zeros((B, self.num_pairs, L, self.dim, self.deg + 1))

    def speed_jac(self, Y, tf, is_max):
        B, L = self._note(Y, 'speed_jac', None, (is_max,))
        return np.zeros((B, self.n_veh, L, self.dim, self.deg + 1)), np.zeros((B, self.n_veh, L))

    def ang_rate_jac(self, Y, tf):
        B, _ = self._note(Y, 'ang_rate_jac')
        La = 4 * (self.deg + self.deg_elev) + 1
        return np.zeros((B, self.n_veh, La, 2, self.deg + 1)), np.zeros((B, self.n_veh, La))

    # -- the per-vehicle families
    def _rows(self, method, Y, bound, flags=()):
        B, L = self._note(Y, method, bound, flags)
        return np.zeros((B, self.n_veh * (4 * (self.deg + self.deg_elev) + 1 if method == 'ang_rate' else L)))

    def _true(self, method, Y, bound, flags, eps_rel, sides=()):
        B, _ = self._note(Y, method, bound, flags, eps_rel)
        return self._search((B, self.n_veh) + sides, ('jac', 'jac_tf') if method.endswith('_jac') else ())

    def speed(self, Y, tf, bound, is_max):
        return self._rows('speed', Y, bound, (is_max,))

    def speed_true_min(self, Y, tf, bound, is_max, eps_rel=1e-9):
        return self._true('speed_true_min', Y, bound, (is_max,), eps_rel)

    def speed_true_min_jac(self, Y, tf, bound, is_max, eps_rel=1e-9):
        return self._true('speed_true_min_jac', Y, bound, (is_max,), eps_rel)

    def accel(self, Y, tf, bound):
        return self._rows('accel', Y, bound)

    def accel_true_min(self, Y, tf, bound, eps_rel=1e-9):
        return self._true('accel_true_min', Y, bound, (), eps_rel)

    def accel_true_min_jac(self, Y, tf, bound, eps_rel=1e-9):
        return self._true('accel_true_min_jac', Y, bound, (), eps_rel)

    def jerk(self, Y, tf, bound):
        return self._rows('jerk', Y, bound)

    def jerk_true_min(self, Y, tf, bound, eps_rel=1e-9):
        return self._true('jerk_true_min', Y, bound, (), eps_rel)

    def jerk_true_min_jac(self, Y, tf, bound, eps_rel=1e-9):
        return self._true('jerk_true_min_jac', Y, bound, (), eps_rel)

    def ang_rate(self, Y, tf, max_rate):
        return self._rows('ang_rate', Y, max_rate)

    def ang_rate_true_min(self, Y, tf, max_rate, eps_rel=1e-9):
        return self._true('ang_rate_true_min', Y, max_rate, (), eps_rel, (2,))

    def ang_rate_true_min_jac(self, Y, tf, max_rate, eps_rel=1e-9):
        return self._true('ang_rate_true_min_jac', Y, max_rate, (), eps_rel, (2,))

    # -- the objectives
    def euclidean_obj(self, Y):
        return np.zeros(self._note(Y, 'euclidean_obj')[0])

    def euclidean_grad(self, Y):
        return np.zeros((self._note(Y, 'euclidean_grad')[0], self.n_veh * self.dim, self.deg + 1))

    def deriv_energy_obj(self, Y, tf, order):
        return np.zeros(self._note(Y, 'deriv_energy_obj', tf, (order,))[0])

    def deriv_energy_grad(self, Y, tf, order):
        B, _ = self._note(Y, 'deriv_energy_grad', tf, (order,))
        return np.zeros((B, self.n_veh * self.dim, self.deg + 1)), np.zeros(B)

    def arc_length_obj(self, Y, eps_rel=1e-12, grad=False):
        B, _ = self._note(Y, 'arc_length_obj', None, (grad,), eps_rel)
        r = dict(val=np.zeros(B), status=np.zeros(B, np.int32))
        if grad:
            r['grad'] = np.zeros((B, self.n_veh * self.dim, self.deg + 1))
        return r


@pytest.fixture(autouse=True)
def recorder(monkeypatch):
    monkeypatch.setattr(opt._capi, 'Context', Recorder)
    monkeypatch.setattr(opt, 'DEG_ELEV', 0)
    Recorder.log = []


BOUNDS = dict(maxSep=0.9, minSpeed=0.5, maxSpeed=5.0, maxAngRate=1.5, maxAccel=7.0, maxJerk=11.0)


def problem(dim=2, goal='TimeOpt', **kw):
    """dim 2: 2 vehicles, degree 5, prescribed speeds (time-optimal: n_x = 9); dim 3: 2 vehicles, degree 5, no speeds."""
    kw = dict(BOUNDS, **kw)
    if dim == 2:
        return opt.BezOptimization(numVeh=2, dimension=2, degree=5, minimizeGoal=goal, initPoints=[(0, 0), (0, 3)],
                                   finalPoints=[(10, 3), (10, 0)], initSpeeds=[1, 1], finalSpeeds=[1, 1], initAngs=[0, 0],
                                   finalAngs=[0, 0], tf=10.0, device=0, **kw)
    return opt.BezOptimization(numVeh=2, dimension=3, degree=5, initPoints=[(0, 0, 0), (0, 3, 1)],
                               finalPoints=[(10, 3, 1), (10, 0, 0)], tf=10.0, device=0, **kw)


def calls(fn, *args, **kw):
    """The set of distinct (method, bound, flags, eps_rel) the call leaves in the recorder."""
    Recorder.log = []
    fn(*args, **kw)
    return set(Recorder.log)


# ------------------------------------------------------------------------------------------------ the refusals
# provider: (its rows option, its bound where that may be None)
PROVIDERS = {'maxSpeedJacobian': ('speedRows', None), 'minSpeedJacobian': ('speedRows', None),
             'maxAngularRateJacobian': ('angRateRows', None), 'maxAccelJacobian': ('accelRows', 'maxAccel'),
             'maxJerkJacobian': ('jerkRows', 'maxJerk'), 'temporalSeparationJacobian': ('separationRows', None)}
CASES = [(p, method, rows, no_bound, dim)
         for p, (_, bound) in PROVIDERS.items() for method in ('fd', 'exact', 'envelope', 'bogus') for rows in ('all', 'true_min')
         for no_bound in ((False, True) if bound else (False,)) for dim in (2, 3)]


def refusal(provider, method, rows, no_bound, dim):
    """(exception type's name, its full text) when the provider answers before any call of the context, else None."""
    option, bound = PROVIDERS[provider]
    bo = problem(dim, **dict({option: rows}, **({bound: None} if no_bound else {})))
    x = bo.generateGuess(std=0.1, seed=1)
    Recorder.log = []
    try:
        getattr(bo, provider)(x, method=method)
    except Exception as e:
        if Recorder.log:
            raise
        return type(e).__name__, str(e)
    assert Recorder.log, "answered without a device call and without an exception"
    return None


# (provider, method, rows option, bound is None, dimension) -> the ValueError's text: what the commit before the family table
# raised, taken from a run of it on these problems (every case not listed went on to a call of the context)
REFUSALS = {}
BOTH, ROWS, DIMS = (False, True), ('all', 'true_min'), (2, 3)


def refused(text, provider, method, rows=ROWS, no_bound=(False,), dims=DIMS):
    for case in itertools.product((provider,), (method,), rows, no_bound, dims):
        assert case not in REFUSALS
        REFUSALS[case] = text


NOT_FD_EXACT = "method must be 'fd' or 'exact', not 'bogus'"
PLANAR = 'The input curve must be two dimensional,\ninstead it is 3 dimensional'

refused("maxSpeedJacobian(method='exact') is not available with speedRows='true_min' (the envelope derivative is not built under "
        "that name): use method='envelope' or method='fd'", 'maxSpeedJacobian', 'exact', ('true_min',))
refused("maxSpeedJacobian(method='envelope') needs speedRows='true_min', not 'all'", 'maxSpeedJacobian', 'envelope', ('all',))
refused(NOT_FD_EXACT, 'maxSpeedJacobian', 'bogus')
refused("minSpeedJacobian(method='exact') is not available with speedRows='true_min' (the envelope derivative is not built under "
        "that name): use method='envelope' or method='fd'", 'minSpeedJacobian', 'exact', ('true_min',))
refused("minSpeedJacobian(method='envelope') needs speedRows='true_min', not 'all'", 'minSpeedJacobian', 'envelope', ('all',))
refused(NOT_FD_EXACT, 'minSpeedJacobian', 'bogus')

# the angular rate in 3-D: from Python for 'envelope', 'exact' or the true-minimum rows -- before the method's name is looked at
refused(PLANAR, 'maxAngularRateJacobian', 'fd', ('true_min',), dims=(3,))
refused(PLANAR, 'maxAngularRateJacobian', 'exact', dims=(3,))
refused(PLANAR, 'maxAngularRateJacobian', 'envelope', dims=(3,))
refused(PLANAR, 'maxAngularRateJacobian', 'bogus', ('true_min',), dims=(3,))
refused("maxAngularRateJacobian(method='exact') is not available with angRateRows='true_min' (the envelope derivative is not "
        "built under that name): use method='envelope' or method='fd'", 'maxAngularRateJacobian', 'exact', ('true_min',), dims=(2,))
refused("maxAngularRateJacobian(method='envelope') needs angRateRows='true_min', not 'all'", 'maxAngularRateJacobian', 'envelope',
        ('all',), dims=(2,))
refused(NOT_FD_EXACT, 'maxAngularRateJacobian', 'bogus', ('all',))
refused(NOT_FD_EXACT, 'maxAngularRateJacobian', 'bogus', ('true_min',), dims=(2,))

# acceleration and jerk: 'envelope' without the true-minimum rows and an unknown or unbuilt method answer before a missing bound
refused("maxAccelJacobian needs a bound: maxAccel is None", 'maxAccelJacobian', 'fd', no_bound=(True,))
refused("maxAccelJacobian(method='exact') is not built for the acceleration rows: use method='fd' or, with accelRows='true_min', "
        "method='envelope'", 'maxAccelJacobian', 'exact', no_bound=BOTH)
refused("maxAccelJacobian(method='envelope') needs accelRows='true_min', not 'all'", 'maxAccelJacobian', 'envelope', ('all',), BOTH)
refused("maxAccelJacobian needs a bound: maxAccel is None", 'maxAccelJacobian', 'envelope', ('true_min',), (True,))
refused(NOT_FD_EXACT, 'maxAccelJacobian', 'bogus', no_bound=BOTH)
refused("maxJerkJacobian needs a bound: maxJerk is None", 'maxJerkJacobian', 'fd', no_bound=(True,))
refused("maxJerkJacobian(method='exact') is not built for the jerk rows: use method='fd' or, with jerkRows='true_min', "
        "method='envelope'", 'maxJerkJacobian', 'exact', no_bound=BOTH)
refused("maxJerkJacobian(method='envelope') needs jerkRows='true_min', not 'all'", 'maxJerkJacobian', 'envelope', ('all',), BOTH)
refused("maxJerkJacobian needs a bound: maxJerk is None", 'maxJerkJacobian', 'envelope', ('true_min',), (True,))
refused(NOT_FD_EXACT, 'maxJerkJacobian', 'bogus', no_bound=BOTH)

refused("temporalSeparationJacobian(method='exact') is not available with separationRows='true_min' (the envelope derivative is "
        "not built under that name): use method='envelope' or method='fd'", 'temporalSeparationJacobian', 'exact', ('true_min',))
refused("temporalSeparationJacobian(method='envelope') needs separationRows='true_min', not 'all'", 'temporalSeparationJacobian',
        'envelope', ('all',))
refused(NOT_FD_EXACT, 'temporalSeparationJacobian', 'bogus')


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_refusals_are_those_of_the_code_before_the_table(case):
    assert refusal(*case) == (('ValueError', REFUSALS[case]) if case in REFUSALS else None)


def test_the_refusal_matrix_is_the_issue_s():
    assert len(CASES) == 128 and set(REFUSALS) <= set(CASES) and len(REFUSALS) == 87


def test_rows_options_are_checked_in_the_constructor_s_order():
    for option in ('speedRows', 'angRateRows', 'accelRows', 'jerkRows'):
        with pytest.raises(ValueError) as e:
            opt.BezOptimization(**{option: 'bogus'})
        assert str(e.value) == "%s must be 'all' or 'true_min', not 'bogus'" % option
    with pytest.raises(ValueError) as e:
        opt.BezOptimization(speedRows='a', angRateRows='b', accelRows='c', jerkRows='d', separationRows='e')
    assert str(e.value) == "jerkRows must be 'all' or 'true_min', not 'd'"
    with pytest.raises(ValueError) as e:
        opt.BezOptimization(speedRows='a', angRateRows='b', accelRows='c', separationRows='e')
    assert str(e.value) == "accelRows must be 'all' or 'true_min', not 'c'"
    with pytest.raises(ValueError) as e:
        opt.BezOptimization(speedRows='a', angRateRows='b', separationRows='e')
    assert str(e.value) == "angRateRows must be 'all' or 'true_min', not 'b'"
    with pytest.raises(ValueError) as e:
        opt.BezOptimization(speedRows='a', separationRows='e')
    assert str(e.value) == "speedRows must be 'all' or 'true_min', not 'a'"
    with pytest.raises(ValueError) as e:
        opt.BezOptimization(separationRows='e')
    assert str(e.value) == "separationRows must be 'all', 'min', 'active' or 'true_min', not 'e'"


@pytest.mark.parametrize("closure, what", [('maxAccelConstraints', 'maxAccel'), ('maxJerkConstraints', 'maxJerk')])
@pytest.mark.parametrize("rows", ['all', 'true_min'])
def test_a_closure_without_its_bound_answers_before_the_device(closure, what, rows):
    bo = problem(2, **{what: None, {'maxAccel': 'accelRows', 'maxJerk': 'jerkRows'}[what]: rows})
    x = bo.generateGuess(std=0.1, seed=1)
    Recorder.log = []
    with pytest.raises(ValueError) as e:
        getattr(bo, closure)(x)
    assert str(e.value) == "%s needs a bound: %s is None" % (closure, what) and not Recorder.log
    with pytest.raises(ValueError) as e:
        bo._fd_values(x, {'maxAccel': 'amax', 'maxJerk': 'jmax'}[what])
    assert str(e.value) == "%s needs a bound: %s is None" % (closure, what) and not Recorder.log


def test_angular_rate_closure_refuses_in_python():
    bo = problem(3)
    with pytest.raises(ValueError) as e:
        bo.maxAngularRateConstraints(bo.generateGuess(std=0.1, seed=1))
    assert str(e.value) == PLANAR and not Recorder.log
    bo = problem(2)
    x = bo.generateGuess(std=0.1, seed=1)
    x[-1] = 0.0
    with pytest.raises(TypeError) as e:
        bo.maxAngularRateConstraints(x)
    assert str(e.value) == "unsupported operand type(s) for *: 'NoneType' and 'NoneType'" and not Recorder.log
    with pytest.raises(ValueError) as e:
        problem(3).trueAngularRateRows(problem(3).generateGuess(std=0.1, seed=1))
    assert str(e.value) == PLANAR and not Recorder.log


# ------------------------------------------------------------------------------------------------ the routing
EPS = 1e-12       # BezOptimization.TRUE_MIN_EPS_REL, ARC_LENGTH_EPS_REL
# family key: (rows option, closure, provider, {rows: (Context method, bound of BOUNDS, leading flags)}, envelope's method)
ROUTES = {
    'vmax': ('speedRows', 'maxSpeedConstraints', 'maxSpeedJacobian',
             {'all': ('speed', 5.0, (True,)), 'true_min': ('speed_true_min', 5.0, (True,))}, 'speed_true_min_jac'),
    'vmin': ('speedRows', 'minSpeedConstraints', 'minSpeedJacobian',
             {'all': ('speed', 0.5, (False,)), 'true_min': ('speed_true_min', 0.5, (False,))}, 'speed_true_min_jac'),
    'ang': ('angRateRows', 'maxAngularRateConstraints', 'maxAngularRateJacobian',
            {'all': ('ang_rate', 1.5, ()), 'true_min': ('ang_rate_true_min', 1.5, ())}, 'ang_rate_true_min_jac'),
    'amax': ('accelRows', 'maxAccelConstraints', 'maxAccelJacobian',
             {'all': ('accel', 7.0, ()), 'true_min': ('accel_true_min', 7.0, ())}, 'accel_true_min_jac'),
    'jmax': ('jerkRows', 'maxJerkConstraints', 'maxJerkJacobian',
             {'all': ('jerk', 11.0, ()), 'true_min': ('jerk_true_min', 11.0, ())}, 'jerk_true_min_jac'),
}


def test_true_min_eps_is_the_class_constant():
    assert opt.BezOptimization.TRUE_MIN_EPS_REL == EPS and opt.BezOptimization.ARC_LENGTH_EPS_REL == EPS


@pytest.mark.parametrize("rows", ['all', 'true_min'])
@pytest.mark.parametrize("key", sorted(ROUTES))
def test_vehicle_family_routes(key, rows):
    option, closure, provider, route, envelope = ROUTES[key]
    method, bound, flags = route[rows]
    want = {(method, bound, flags, EPS if rows == 'true_min' else None)}
    bo = problem(2, **{option: rows})
    x = bo.generateGuess(std=0.1, seed=1)
    assert calls(getattr(bo, closure), x) == want
    assert calls(bo._fd_values, x, key) == want
    F, dx = bo._fd_values(x, key)
    per = {'all': 2 * (4 * 5 + 1) if key == 'ang' else 2 * (2 * 5 + 1), 'true_min': 4 if key == 'ang' else 2}[rows]
    assert F.shape == (x.size + 1, per) and dx.shape == (x.size,)
    for structured in (True, False):
        assert calls(getattr(bo, provider), x, structured=structured, method='fd') == want
        assert getattr(bo, provider)(x, structured=structured).shape == (per, x.size)
    if rows == 'true_min':
        assert calls(getattr(bo, provider), x, method='envelope') == {(envelope, bound, flags, EPS)}
        assert getattr(bo, provider)(x, method='envelope').shape == (per, x.size)


def test_vehicle_family_exact_and_true_accessors_route():
    bo = problem(2)
    x = bo.generateGuess(std=0.1, seed=1)
    assert calls(bo.maxSpeedJacobian, x, method='exact') == {('speed_jac', None, (True,), None)}
    assert calls(bo.minSpeedJacobian, x, method='exact') == {('speed_jac', None, (False,), None)}
    assert calls(bo.maxAngularRateJacobian, x, method='exact') == {('ang_rate_jac', None, (), None)}
    assert bo.maxSpeedJacobian(x, method='exact').shape == (22, 9) and bo.maxAngularRateJacobian(x, method='exact').shape == (42, 9)
    # the accessors: the family's true minima under bound 0 (the angular rate: its own bound), whatever the rows option is
    assert calls(bo.trueSpeedRange, x) == {('speed_true_min', 0.0, (False,), EPS), ('speed_true_min', 0.0, (True,), EPS)}
    assert calls(bo.trueAccelMax, x) == {('accel_true_min', 0.0, (), EPS)}
    assert calls(bo.trueJerkMax, x) == {('jerk_true_min', 0.0, (), EPS)}
    assert calls(bo.trueAngularRateRows, x) == {('ang_rate_true_min', 1.5, (), EPS)}
    assert calls(bo.trueMinSeparation, x) == {('temporal_sep_true_min', 0.9, (), EPS)}
    assert [np.shape(a) for a in bo.trueSpeedRange(x)] == [(2,)] * 4
    assert [np.shape(a) for a in bo.trueAngularRateRows(x)] == [(2, 2)] * 2


# goal: (value's method, bound = the tf of the problem, flags), (gradient's)
GOAL_ROUTES = {
    'Euclidean': (('euclidean_obj', None, (), None), ('euclidean_grad', None, (), None)),
    'Accel': (('deriv_energy_obj', 10.0, (2,), None), ('deriv_energy_grad', 10.0, (2,), None)),
    'Jerk': (('deriv_energy_obj', 10.0, (3,), None), ('deriv_energy_grad', 10.0, (3,), None)),
    'arcLength': (('arc_length_obj', None, (False,), EPS), ('arc_length_obj', None, (True,), EPS)),
}


@pytest.mark.parametrize("goal", sorted(GOAL_ROUTES))
def test_objective_routes(goal):
    value, grad = GOAL_ROUTES[goal]
    bo = problem(2, goal=goal)
    x = bo.generateGuess(std=0.1, seed=1)
    assert x.size == 8
    assert calls(bo.objectiveFunction, x) == {value}
    named = {'Euclidean': 'euclideanObjective', 'Accel': 'accelObjective', 'Jerk': 'jerkObjective', 'arcLength': 'arcLengthObjective'}
    assert calls(getattr(bo, named[goal]), x) == set()                   # (the same point: kept, not asked again)
    assert calls(getattr(problem(2, goal=goal), named[goal]), x) == {value}
    assert calls(bo._fd_values, x, 'obj_' + goal.lower()) == {value}
    assert bo._fd_values(x, 'obj_' + goal.lower())[0].shape == (9, 1)
    assert calls(bo.objectiveGradient, x) == {value}
    assert calls(bo.objectiveGradient, x, method='exact') == {grad}
    assert bo.objectiveGradient(x).shape == (8,) and bo.objectiveGradient(x, method='exact').shape == (8,)


def test_time_optimal_and_unknown_goals():
    bo = problem(2)
    x = bo.generateGuess(std=0.1, seed=1)
    assert calls(lambda: bo.objectiveFunction(x)) == set() and bo.objectiveFunction(x) == x[-1]
    for method in ('fd', 'exact'):
        assert calls(bo.objectiveGradient, x, method=method) == set()
        assert np.array_equal(bo.objectiveGradient(x, method=method), np.eye(9)[-1])
    bad = problem(2, goal='Snap')
    for ask in (lambda: bad.objectiveFunction, lambda: bad.objectiveGradient(x[:-1]), lambda: bad.objectiveGradient(x[:-1], method='exact')):
        with pytest.raises(ValueError) as e:
            ask()
        assert str(e.value) == ("The provided minimize goal, snap, is not a valid goal. The available minimize goals are:\n"
                                "dict_keys(['euclidean', 'timeopt', 'accel', 'jerk', 'arclength'])")


SEP_ROUTES = {'all': ('temporal_sep', 0.9, (), None), 'min': ('temporal_sep_min', 0.9, (), None),
              'active': ('temporal_sep_active', 0.9, (2,), None), 'true_min': ('temporal_sep_true_min', 0.9, (), EPS)}


@pytest.mark.parametrize("rows", sorted(SEP_ROUTES))
def test_separation_routes(rows):
    bo = problem(2, separationRows=rows)
    x = bo.generateGuess(std=0.1, seed=1)
    per = {'all': 11, 'min': 1, 'active': 2, 'true_min': 1}[rows]
    assert calls(bo.temporalSeparationConstraints, x) == {SEP_ROUTES[rows]}
    assert bo.temporalSeparationConstraints(x).shape == (per,)
    assert calls(bo._fd_values, x, 'tsep') == {SEP_ROUTES[rows]}
    assert calls(bo.temporalSeparationJacobian, x, structured=False) == {SEP_ROUTES[rows]}
    assert bo.temporalSeparationJacobian(x, structured=False).shape == (per, 9)
    if rows == 'true_min':
        assert calls(bo.temporalSeparationJacobian, x, method='envelope') == {('temporal_sep_true_min_jac', 0.9, (), EPS)}
        assert calls(bo.trueMinSeparationJacobian, x) == {('temporal_sep_true_min_jac', 0.9, (), EPS)}


# ------------------------------------------------------------------------------------------------ the key of a kept batch
def test_serve_key_is_the_tuple_it_was_and_sees_every_option_and_bound():
    bo = problem(2)
    key = bo._serve_key(True)
    assert key[:9] == (0, 'all', 'all', 'all', 'all', 7.0, 'all', 11.0, 2)      # DEG_ELEV, the rows options (optional bounds behind theirs), activeRows
    assert key[10:] == (0.9, 5.0, 0.5, 1.5, None, None, None) and key[9] == bo._rv_cache[0]
    fixed = problem(2, goal='Euclidean', pointObstacles=[(5.0, 1.0)])
    assert fixed._serve_key(True)[14:16] == (10.0, np.asarray([(5.0, 1.0)]).tobytes())
    seen = {key}
    for option, value in (('separationRows', 'min'), ('speedRows', 'true_min'), ('angRateRows', 'true_min'),
                          ('accelRows', 'true_min'), ('jerkRows', 'true_min'), ('activeRows', 3)):
        setattr(bo, option, value)
        k = bo._serve_key(True)
        assert k not in seen, option
        seen.add(k)
    for bound in sorted(BOUNDS):
        for value in (BOUNDS[bound] + 1.0, None):
            bo.model[bound] = value
            k = bo._serve_key(True)
            assert k not in seen, bound
            seen.add(k)
    opt.DEG_ELEV = 3                     # (the fixture's monkeypatch puts it back)
    assert bo._serve_key(True) not in seen
