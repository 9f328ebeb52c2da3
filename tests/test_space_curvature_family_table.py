"""The space-curvature family's entry in the Python layer's table (optimization._ROW_FAMILIES 'scurv'), without a device:
which _capi.Context method its closure, its _fd_values, its Jacobian provider and trueSpaceCurvatureMax call, with which
bound and eps_rel; what is refused in Python, in which words; the tf column; and _serve_key.  The recording stand-in is
test_row_family_table.py's, with the space-curvature calls added."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_row_family_table as T  # noqa: E402
from optimalbeziertrajectorygeneration_amd import optimization as opt  # noqa: E402
from optimalbeziertrajectorygeneration_amd import bezier  # noqa: E402

EPS = 1e-12


class Recorder(T.Recorder):
    block = 0.0            # what every entry of a recorded envelope block holds

    def space_curvature_true_min(self, Y, max_curv, eps_rel=1e-9):
        B, _ = self._note(Y, 'space_curvature_true_min', max_curv, (), eps_rel)
        return self._search((B, self.n_veh))

    def space_curvature_true_min_jac(self, Y, max_curv, eps_rel=1e-9):
        B, _ = self._note(Y, 'space_curvature_true_min_jac', max_curv, (), eps_rel)
        r = self._search((B, self.n_veh), ('jac',))
        r['jac'] += Recorder.block
        return r

    def bern_space_curvature(self, c, eps_rel=1e-9):
        M = np.asarray(c).shape[0]
        assert np.asarray(c).shape[1] == 3
        T.Recorder.log.append(('bern_space_curvature', None, (), eps_rel))
        return dict(k_max=np.zeros(M), t_max=np.zeros(M), status=np.zeros(M, np.int32))


@pytest.fixture(autouse=True)
def recorder(monkeypatch):
    monkeypatch.setattr(opt._capi, 'Context', Recorder)
    monkeypatch.setattr(opt, 'DEG_ELEV', 0)
    T.Recorder.log = []
    Recorder.block = 0.0


def timeopt3(**kw):
    """2 vehicles in space, degree 5, time-optimal, no prescribed speeds: n_x = 2 * 3 * 4 + 1 = 25 and dY/dtf = 0"""
    return opt.BezOptimization(numVeh=2, dimension=3, degree=5, minimizeGoal='TimeOpt', initPoints=[(0, 0, 0), (0, 3, 1)],
                               finalPoints=[(10, 3, 1), (10, 0, 0)], tf=10.0, device=0, **dict(T.BOUNDS, **kw))


ROUTE = ('space_curvature_true_min', 0.4, (), EPS)
ROUTE_JAC = ('space_curvature_true_min_jac', 0.4, (), EPS)
BERN = ('bern_space_curvature', None, (), EPS)


def test_the_record():
    fam = opt._FAMILY['scurv']
    assert fam.bound == 'maxSpaceCurvature' and fam.optional and fam.rows is None and fam.rows_attr is None and fam.exact is None
    assert fam.sides == 1 and fam.span is False and fam.planar is False and fam.only_dim == 3 and fam.lead == ()
    # the new field has a default: every other record reads as it did
    assert all(f.only_dim is None for f in opt._ROW_FAMILIES if f.key != 'scurv')
    assert opt._KEY_TAIL == ('maxCurvature', 'maxSpaceCurvature')
    assert ('maxSpaceCurvature', 'maxSpaceCurvature', None) in opt._MODEL_FIELDS


def test_routes():
    bo = T.problem(3, maxSpaceCurvature=0.4)
    x = bo.generateGuess(std=0.1, seed=1)
    n_x = x.size
    assert n_x == 2 * 3 * 4
    assert T.calls(bo.maxSpaceCurvatureConstraints, x) == {ROUTE}
    rows = bo.maxSpaceCurvatureConstraints(x)
    assert rows.shape == (2,) and rows.dtype == np.float64
    assert T.calls(bo._fd_values, x, 'scurv') == {ROUTE}
    assert bo._fd_values(x, 'scurv')[0].shape == (n_x + 1, 2)
    for structured in (True, False):
        assert T.calls(bo.maxSpaceCurvatureJacobian, x, structured=structured) == {ROUTE}
        assert T.calls(bo.maxSpaceCurvatureJacobian, x, structured=structured, method='fd') == {ROUTE}
    assert bo.maxSpaceCurvatureJacobian(x).shape == (2, n_x)
    assert T.calls(bo.maxSpaceCurvatureJacobian, x, method='envelope') == {ROUTE_JAC}
    assert bo.maxSpaceCurvatureJacobian(x, method='envelope').shape == (2, n_x)
    assert T.calls(bo.trueSpaceCurvatureMax, x) == {BERN}
    assert [a.shape for a in bo.trueSpaceCurvatureMax(x)] == [(2,)] * 2
    assert not hasattr(bo, 'spaceCurvatureRows')


def test_a_kept_batch_serves_scipy_s_differences_and_sees_the_bound():
    bo = T.problem(3, maxSpaceCurvature=0.4)
    x = bo.generateGuess(std=0.1, seed=1)
    bo.maxSpaceCurvatureConstraints(x)
    T.Recorder.log = []
    for k in range(x.size):
        xk = x.copy()
        xk[k] += opt.FD_STEP
        bo.maxSpaceCurvatureConstraints(xk)
    assert T.Recorder.log == [ROUTE]                       # one batch
    bo.model['maxSpaceCurvature'] = 0.5                    # the bound edited: the kept batch is not served
    xk = x.copy()
    xk[0] += opt.FD_STEP
    assert T.calls(bo.maxSpaceCurvatureConstraints, xk) == {('space_curvature_true_min', 0.5, (), EPS)}


def test_refusals():
    spatial = 'The input curve must be three dimensional,\ninstead it is 2 dimensional'
    no_bound = "%s needs a bound: maxSpaceCurvature is None"
    bo2 = T.problem(2, maxSpaceCurvature=0.4)
    x2 = bo2.generateGuess(std=0.1, seed=1)
    for ask in (lambda: bo2.maxSpaceCurvatureConstraints(x2), lambda: bo2.maxSpaceCurvatureJacobian(x2),
                lambda: bo2.maxSpaceCurvatureJacobian(x2, structured=False),
                lambda: bo2.maxSpaceCurvatureJacobian(x2, method='envelope'), lambda: bo2.maxSpaceCurvatureJacobian(x2, method='exact'),
                lambda: bo2.maxSpaceCurvatureJacobian(x2, method='bogus'), lambda: bo2.trueSpaceCurvatureMax(x2),
                lambda: bezier.Bezier(np.array([[0.0, 1.0, 2.0], [0.0, 1.0, 0.0]])).spaceCurvatureMax()):
        T.Recorder.log = []
        with pytest.raises(ValueError) as e:
            ask()
        assert str(e.value) == spatial and not T.Recorder.log
    # maxCurvature in dimension 3 goes on raising exactly as it did
    bo3 = T.problem(3, maxCurvature=0.4, maxSpaceCurvature=0.4)
    x3 = bo3.generateGuess(std=0.1, seed=1)
    with pytest.raises(ValueError) as e:
        bo3.maxCurvatureConstraints(x3)
    assert str(e.value) == 'The input curve must be two dimensional,\ninstead it is 3 dimensional'
    bo = T.problem(3)                                      # maxSpaceCurvature is None
    x = bo.generateGuess(std=0.1, seed=1)
    for ask, who in ((lambda: bo.maxSpaceCurvatureConstraints(x), 'maxSpaceCurvatureConstraints'),
                     (lambda: bo._fd_values(x, 'scurv'), 'maxSpaceCurvatureConstraints'),
                     (lambda: bo.maxSpaceCurvatureJacobian(x), 'maxSpaceCurvatureJacobian'),
                     (lambda: bo.maxSpaceCurvatureJacobian(x, method='envelope'), 'maxSpaceCurvatureJacobian')):
        T.Recorder.log = []
        with pytest.raises(ValueError) as e:
            ask()
        assert str(e.value) == no_bound % who and not T.Recorder.log
    assert T.calls(bo.trueSpaceCurvatureMax, x) == {BERN}  # the maximum needs no bound
    for b in (bo, T.problem(3, maxSpaceCurvature=0.4)):    # 'exact' and an unknown method answer before a missing bound
        T.Recorder.log = []
        with pytest.raises(ValueError) as e:
            b.maxSpaceCurvatureJacobian(x, method='exact')
        assert str(e.value) == ("maxSpaceCurvatureJacobian(method='exact') is not built for the space curvature rows: use "
                                "method='fd' or method='envelope'") and not T.Recorder.log
        with pytest.raises(ValueError) as e:
            b.maxSpaceCurvatureJacobian(x, method='bogus')
        assert str(e.value) == "method must be 'fd' or 'exact', not 'bogus'" and not T.Recorder.log


def test_the_tf_column():
    """The rows do not depend on tf: without prescribed speeds (dY/dtf = 0) the envelope's tf column is an exact 0 whatever
    the blocks hold; a fixed-time problem has no tf column.  (Speeds are prescribed for planar problems only: the column
    that carries dY/dtf is scatter_exact's, held by test_curvature_family_table.py.)"""
    Recorder.block = 3.0
    bo = timeopt3(maxSpaceCurvature=0.4)
    x = bo.generateGuess(std=0.1, seed=1)
    assert x.size == 25
    J = bo.maxSpaceCurvatureJacobian(x, method='envelope')
    assert J.shape == (2, 25) and (J[:, :24] != 0).any()
    assert np.array_equal(J[:, 24], np.zeros(2)) and not np.signbit(J[:, 24]).any()
    # each vehicle's row moves with its own control points alone
    assert (J[0, :12] == 3.0).all() and not J[0, 12:24].any() and (J[1, 12:24] == 3.0).all() and not J[1, :12].any()
    fixed = T.problem(3, maxSpaceCurvature=0.4)
    xf = fixed.generateGuess(std=0.1, seed=1)
    assert fixed.maxSpaceCurvatureJacobian(xf, method='envelope').shape == (2, 24)


def test_serve_key():
    """With the bound None the key is element for element the tuple it was (written out); set, the bound follows maxCurvature's"""
    bo = T.problem(2)
    key = bo._serve_key(True)
    assert len(key) == 17
    assert key[:9] == (0, 'all', 'all', 'all', 'all', 7.0, 'all', 11.0, 2) and key[9] == bo._rv_cache[0]
    assert key[10:] == (0.9, 5.0, 0.5, 1.5, None, None, None)
    bo3 = T.problem(3)
    k3 = bo3._serve_key(True)
    assert len(k3) == 17 and k3[:9] == (0, 'all', 'all', 'all', 'all', 7.0, 'all', 11.0, 2) and k3[10:] == (0.9, 5.0, 0.5, 1.5, 10.0, None, None)
    bo3.model['maxSpaceCurvature'] = 0.4
    assert bo3._serve_key(True) == k3 + (('maxSpaceCurvature', 0.4),)
    bo3.model['maxCurvature'] = 0.3
    assert bo3._serve_key(True) == k3 + (('maxCurvature', 0.3), ('maxSpaceCurvature', 0.4))
    bo3.model['maxSpaceCurvature'] = None
    assert bo3._serve_key(True) == k3 + (('maxCurvature', 0.3),)


def test_a_search_that_ends_on_a_cap_raises(monkeypatch):
    plain = Recorder.space_curvature_true_min

    def capped(self, Y, max_curv, eps_rel=1e-9):
        r = plain(self, Y, max_curv, eps_rel)
        r['status'][0, 1] = opt._capi.MD_NODE_CAP
        return r
    monkeypatch.setattr(Recorder, 'space_curvature_true_min', capped)
    bo = T.problem(3, maxSpaceCurvature=0.4)
    x = bo.generateGuess(std=0.1, seed=1)
    with pytest.raises(RuntimeError, match=r"maxSpaceCurvatureConstraints\(true_min\): node budget exhausted"):
        bo.maxSpaceCurvatureConstraints(x)
