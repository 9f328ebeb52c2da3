"""`bezier.Bezier` look-alike whose arithmetic runs on the MI355X through libobtg_hip.so.

Mirrors the part of the reference's object API that the SLSQP constraint callbacks and the
drivers use (reference bezier.py:34-270 container, 318-519 add/sub/mul/div/elev/diff,
840-889 minDist/minDist2Poly/normSquare).  Every method below that computes control points
calls the C ABI (include/obtg.h); there is no CPU implementation of those in this package.

Differences from the reference, on purpose:
  * the constructor accepts any array-like (the reference needs an ndarray and crashes on
    the lists its own `_minDist` passes, bezier.py:58, 1304);
  * `minDist` / `minDist2Poly` work (at the reference's HEAD they raise because `gjkNew` is
    never imported, bezier.py:21-22) and report the reference's non-terminating inputs as
    exceptions instead of hanging;
  * plotting (`plot`, matplotlib) is outside the accelerated path and is not provided; `curve` /
    `__call__` -- what the drivers' own plotting code reads after a solve -- are (obtg_bern_eval);
  * curves with different [t0, tf]: the reference's `add` / `sub` always align them (`_temporalAlignment`,
    bezier.py:903-941); here that is `add(other, align=True)` / `sub(other, align=True)` (obtg_bern_restrict), and the
    default -- so `+` and `-` -- still raises NotImplementedError on unequal spans;
  * `min` / `max` return the curve's true extremum within `tol` (obtg_bern_extrema: a certified subdivision search), not
    what the reference's recursion returns (bezier.py:631-667, 727-763).  That recursion splits a child at
    `minIdx / deg` taken as an absolute parameter, outside the child's span (bezier.py:659-661 with 560-561): on the
    reference's own example c6 = Bezier([(0,1,2,3,4,5), (5,0,2,5,7,5)]) `c6.min(dim=1)` returns 1.7744000000000004 where
    the minimum is 2.2606668630782703, and `c6.max(dim=1)` ends in RecursionError (true maximum 5.699106677492463);
  * `minDist` on curves of different degree (obtg_min_dist_mixed) pads each 2-D curve to 3-D by its OWN length.  The
    reference pads the second curve with `[0] * x1.size` (bezier.py:1302), the FIRST curve's length, so it raises on a
    2-D second curve of another degree; 3-D pairs and a 2-D first curve against a 3-D second one are the reference's.
    `minDist(robust=True)` and `collCheck(robust=True)` -- not the reference's algorithms: their answer is the true
    distance of the curves -- elevate the lower curve to the other's degree (obtg_bern_elev: the same curve, the same
    parameter) and run the equal-degree search; `collCheck` without `robust` still takes equal degrees only;
  * `arcLength` is not in the reference: the true length of the curve (obtg_bern_arc_length), the quantity the reference's
    control-polygon sum (optimization.py:462-489) bounds from above.  `integrate` is the reference's (bezier.py:521-531),
    on the host: a sum of deg + 1 numbers.
"""
import numpy as np

from . import _capi


def _ctx():
    return _capi.scratch_context()


class _Grid(object):
    """Time span of a curve: its two ends and, on demand only, the sampling grid over them (the
    accelerated path never samples; drivers that plot do)."""
    __slots__ = ('ends', 'samples')
    POINTS = 1001                                          # the reference's grid size (bezier.py:118)

    def __init__(self, t0, tf, samples=None):
        if samples is None:
            self.ends = [float(t0), float(tf)]
        else:                                              # a grid that is handed in decides the span
            self.ends = [samples[0], samples[-1]]
        self.samples = samples

    def move_end(self, which, value):
        self.ends[which] = float(value)
        self.samples = None                                # a stale grid must not outlive its span

    def grid(self):
        if not isinstance(self.samples, np.ndarray):
            self.samples = (np.linspace(self.ends[0], self.ends[1], self.POINTS) if self.samples is None
                            else np.array(self.samples))
        return self.samples


def _span_end(which, name):
    return property(lambda self: self._span.ends[which], lambda self, v: self._span.move_end(which, v),
                    doc='%s of the span; assigning drops a cached tau grid' % name)


def _shape_field(axis, off, name):
    return property(lambda self: None if self._cpts is None else self._cpts.shape[axis] - off, doc=name)


class BezierParams(object):
    """Container half of the reference's curve type (bezier.py:34-145): control points d x (n+1) plus the
    time span.  The reference keeps `_dim` / `_deg` / `_t0` / `_tf` / `_tau` slots side by side and
    updates them in every setter; here the shape IS dim and deg (read off the array) and the span is
    one `_Grid`, so there is nothing to keep in step."""
    _cpts = None

    def __init__(self, cpts=None, tau=None, t0=0.0, tf=1.0):
        if cpts is not None:
            self.cpts = cpts
        self._span = _Grid(t0, tf, tau)

    @property
    def cpts(self):
        return self._cpts

    @cpts.setter
    def cpts(self, value):
        # float64 matrices are taken as they are (the kernels' results arrive that way); anything else --
        # lists, 1-D arrays, integer arrays -- is promoted the way the reference's setter does (bezier.py:92)
        ready = isinstance(value, np.ndarray) and value.ndim == 2 and value.dtype == np.float64
        self._cpts = value if ready else np.array(value, ndmin=2, dtype=float)

    dim = dimension = _shape_field(0, 0, 'rows of cpts')
    deg = degree = _shape_field(1, 1, 'columns of cpts, less one')
    t0 = _span_end(0, 't0')
    tf = _span_end(1, 'tf')

    @property
    def tau(self):
        return self._span.grid()

    @tau.setter
    def tau(self, val):
        self._span = _Grid(0.0, 0.0, np.array(val))


class Bezier(BezierParams):
    """Bezier(cpts=None, t0=0.0, tf=1.0, tau=None) -- reference bezier.py:148-166."""

    def __init__(self, cpts=None, t0=0.0, tf=1.0, tau=None):
        super(Bezier, self).__init__(cpts=cpts, tau=tau, t0=t0, tf=tf)

    def __add__(self, curve):
        return self.add(curve)

    def __sub__(self, curve):
        return self.sub(curve)

    def __mul__(self, curve):
        return self.mul(curve)

    def __truediv__(self, curve):
        return self.div(curve)

    def __repr__(self):
        return 'Bezier({}, {}, {}, {})'.format(self.cpts, self.tau, self.t0, self.tf)       # (bezier.py:180-182: tau is printed too)

    @property
    def x(self):
        return Bezier(self.cpts[0], t0=self.t0, tf=self.tf)

    @property
    def y(self):
        return Bezier(self.cpts[1], t0=self.t0, tf=self.tf) if self.dim > 1 else None

    @property
    def z(self):
        return Bezier(self.cpts[2], t0=self.t0, tf=self.tf) if self.dim > 2 else None

    def __call__(self, t):
        """The curve at the value(s) t, dim x len(t) (bezier.py:184-199); not cached."""
        return _ctx().bern_eval(self.cpts, np.atleast_1d(t), self.t0, self.tf)

    @property
    def curve(self):
        """The curve at every value of `tau` (1001 samples over [t0, tf] unless a grid was given), dim x len(tau)
        (bezier.py:233-258): what the drivers plot after a solve.  Sampled on the device on every access -- the
        reference caches it until cpts / tau change; a sample set is 24 KB and one launch."""
        return _ctx().bern_eval(self.cpts, self.tau, self.t0, self.tf)

    def copy(self):
        return Bezier(self.cpts, self.t0, self.tf)

    # ---- arithmetic (bezier.py:318-374).  Curves on different time spans: align=True cuts both down to the overlap first
    # (the reference always does, `_temporalAlignment` below); the default, and with it `+` and `-`, still refuses them
    def _same_span(self, other):
        if not (self.t0 == other.t0 and self.tf == other.tf):
            raise NotImplementedError('curves with different [t0, tf]: pass align=True to add / sub for the reference\'s '
                                      'temporal alignment (bezier.py:903-941); the operators + and - take equal spans only')

    def _operands(self, other, align):
        """(cpts, other's cpts, t0, tf) of the two curves on a common span, or None when there is none (t0 >= tf)."""
        a, b = self, other
        if align and not (self.t0 == other.t0 and self.tf == other.tf):
            if max(self.t0, other.t0) >= min(self.tf, other.tf):          # the reference's `if t0 >= tf: return None`
                return None
            a, b = _temporalAlignment(self, other)
        else:
            self._same_span(other)
            if self.t0 >= self.tf:
                return None
        return a.cpts, b.cpts, a.t0, a.tf

    def add(self, other, align=False):
        ops = self._operands(other, align)
        return None if ops is None else Bezier(ops[0] + ops[1], t0=ops[2], tf=ops[3])

    def sub(self, other, align=False):
        ops = self._operands(other, align)
        return None if ops is None else Bezier(ops[0] - ops[1], t0=ops[2], tf=ops[3])

    def mul(self, multiplicand):
        """Product of two curves (bezier.py:376-432), dimension by dimension."""
        if not isinstance(multiplicand, Bezier):
            raise TypeError('The multiplicand must be a {} object, not a {}'.format(Bezier, type(multiplicand)))
        if multiplicand.dim != self.dim:
            raise ValueError('The dimension of both Bezier curves must be the same.\n'
                             'The first dimension is {} and the second is {}'.format(self.dim, multiplicand.dim))
        new = self.copy()
        new.cpts = _ctx().bern_mul(self.cpts, multiplicand.cpts)
        return new

    def div(self, denominator):
        """Rational curve numerator/denominator (bezier.py:434-467): element-wise on control points."""
        if not isinstance(denominator, Bezier):
            raise TypeError('The denominator must be a Bezier object, not a {}. '
                            'Or the module has been reloaded.'.format(type(denominator)))
        num, den = self.cpts, denominator.cpts
        with np.errstate(divide='ignore', invalid='ignore'):
            cpts = np.where(num == 0, 0.0, np.where(den == 0, np.inf, num / den))
        return RationalBezier(cpts.astype(np.float64), den.astype(np.float64), tau=self.tau, tf=self.tf)

    def elev(self, R=1):
        """Degree elevation by R (bezier.py:469-495)."""
        new = self.copy()
        new.cpts = _ctx().bern_elev(self.cpts, int(R))
        return new

    def diff(self):
        """Derivative, elevated back to the original degree (bezier.py:497-519)."""
        new = self.copy()
        new.cpts = _ctx().bern_diff(self.cpts, self.tf - self.t0)
        return new

    def integrate(self):
        """The integral of every coordinate over the curve's span, one float per dimension (bezier.py:521-531):
        tf * sum(cpts[d]) / (deg + 1), the control points summed left to right as Python's `sum` does, on the host.  The
        reference scales by `tf` and not by `tf - t0` -- the integral over a span that starts at 0; that is kept."""
        return np.array([self.tf * sum(list(row)) / (self.deg + 1) for row in self.cpts])

    def arcLength(self, eps=1e-12, max_nodes=100000):
        """The length of the curve in space, int |dc/dtau| dtau over [0, 1] (it depends on neither t0 nor tf), within eps x
        (the length of the control polygon) by adaptive Gauss-Legendre bisection on the device (obtg_bern_arc_length); a
        search that does not end within max_nodes panel estimates, or that meets a cusp it cannot resolve at eps, raises as
        minDist does.  Not in the reference."""
        r = _ctx().bern_arc_length(self.cpts, eps_rel=float(eps), max_nodes=int(max_nodes))
        _raise_md(r['status'][0], 'arcLength')
        return float(r['len'][0])

    def curvatureRange(self, eps=1e-9, max_nodes=100000):
        """(k_min, t_min, k_max, t_max): the extrema over the curve of the signed curvature of a planar curve (left turns
        positive) and the parameters in [0, 1] where they are reached, each within eps x |its value| of the true extremum
        (obtg_bern_curvature: a certified bisection on the device); a search that does not end within max_nodes sub-curves --
        a cusp, a stop -- raises as minDist does.  Curvature does not depend on t0 or tf.  Not in the reference."""
        if self.dim != 2:
            raise ValueError('The input curve must be two dimensional,\n'
                             'instead it is {} dimensional'.format(self.dim))
        r = _ctx().bern_curvature(self.cpts, eps_rel=float(eps), max_nodes=int(max_nodes))
        for side in (1, 0):
            _raise_md(r['status'][0][side], 'curvatureRange')
        return float(r['k_min'][0]), float(r['t_min'][0]), float(r['k_max'][0]), float(r['t_max'][0])

    def spaceCurvatureMax(self, eps=1e-9, max_nodes=100000):
        """(k_max, t_max): the largest curvature |c' x c''| / |c'|^3 of a curve in space and the parameter in [0, 1] where it
        is reached, within eps x k_max of the true maximum (obtg_bern_space_curvature: a certified bisection on the device); a
        search that does not end within max_nodes sub-curves -- a cusp, a stop -- raises as minDist does.  Curvature does
        not depend on t0 or tf.  Not in the reference."""
        if self.dim != 3:
            raise ValueError('The input curve must be three dimensional,\n'
                             'instead it is {} dimensional'.format(self.dim))
        r = _ctx().bern_space_curvature(self.cpts, eps_rel=float(eps), max_nodes=int(max_nodes))
        _raise_md(r['status'][0], 'spaceCurvatureMax')
        return float(r['k_max'][0]), float(r['t_max'][0])

    def keepInMargins(self, A, b, eps=1e-12, max_nodes=100000):
        """(margins[F], t[F]): per half-space a_f . p <= b_f of the region A p <= b (A[F][dim], b[F], dim 2 or 3) the true
        minimum over the curve of b_f - a_f . c(t) and the parameter in [0, 1] where it is reached (obtg_keep_in_true_min, the
        call behind BezOptimization.keepInConstraints): the curve stays inside iff every margin is >= 0; with |a_f| = 1 a
        margin is a distance.  It depends on neither t0 nor tf.  Not in the reference."""
        if self.dim not in (2, 3):
            raise ValueError('The input curve must be two or three dimensional,\n'
                             'instead it is {} dimensional'.format(self.dim))
        A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] != self.dim or b.shape != (A.shape[0],):
            raise ValueError('keepInMargins needs A[F][{}] and b[F], F >= 1, not shapes {} and {}'.format(self.dim, A.shape, b.shape))
        F = A.shape[0]
        ctx = _capi.Context(1, self.dim, self.deg, 0, device=_capi.default_device())
        try:
            region = (np.hstack((A, b[:, None])), np.stack((np.zeros(F, np.int32), np.arange(F, dtype=np.int32)), axis=1))
            r = ctx.keep_in_true_min(self.cpts, region, eps_rel=float(eps), max_nodes=int(max_nodes))
        finally:
            ctx.close()
        for st in r['status'][0]:
            _raise_md(st, 'keepInMargins')
        return r['val'][0].copy(), r['t_star'][0].copy()

    def keepOutClearance(self, A, b, eps=1e-12, max_nodes=100000, motion=None, metric='faces'):
        """(clearance, t): the minimum over the curve of G(t) = max_f (a_f . c(t) - b_f) for the convex obstacle A p <= b
        (A[F][dim], b[F], dim 2 or 3, F <= 16) and the parameter in [0, 1] where it is reached (obtg_bern_keep_out, the search
        behind BezOptimization.keepOutConstraints).  Positive: the curve stays outside, and with |a_f| = 1 its true distance to
        the obstacle is at least the clearance (equal where the nearest feature is a face, larger near a corner: conservative
        near corners unless metric='euclidean'); negative:
        minus the deepest penetration.  It depends on neither t0 nor tf.  Not in the reference.
        motion (a Bezier of this curve's dimension, of a degree no higher than this curve's, whose span contains this curve's):
        the obstacle's offset as a function of time, translation only -- the clearance is then that of the relative curve
        c(t) - motion(t) over this curve's span (obtg_bern_keep_out_moving; the motion is cut down to the span on the host by
        obtg_bern_restrict, so the device call gets r = 1).
        metric='euclidean': the signed Euclidean distance to the obstacle in G's place (obtg_bern_keep_out_euclid) -- the true
        clearance near a corner too, whatever |a_f| is; not built together with a motion."""
        if metric not in ('faces', 'euclidean'):
            raise ValueError("metric must be 'faces' or 'euclidean', not {!r}".format(metric))
        if metric == 'euclidean' and motion is not None:
            raise ValueError("metric='euclidean' together with a motion is not built")
        if self.dim not in (2, 3):
            raise ValueError('The input curve must be two or three dimensional,\n'
                             'instead it is {} dimensional'.format(self.dim))
        A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] != self.dim or b.shape != (A.shape[0],):
            raise ValueError('keepOutClearance needs A[F][{}] and b[F], F >= 1, not shapes {} and {}'.format(self.dim, A.shape, b.shape))
        H = np.hstack((A, b[:, None]))
        if metric == 'euclidean':
            r = _ctx().bern_keep_out_euclid(self.cpts, H, eps_rel=float(eps), max_nodes=int(max_nodes))
        elif motion is None:
            r = _ctx().bern_keep_out(self.cpts, H, eps_rel=float(eps), max_nodes=int(max_nodes))
        else:
            if not isinstance(motion, Bezier) or motion.dim != self.dim:
                raise ValueError('keepOutClearance needs a motion that is a Bezier of dimension {}'.format(self.dim))
            if motion.deg > self.deg:
                raise ValueError("the motion's degree, {}, may not be above the curve's, {}".format(motion.deg, self.deg))
            if not (motion.t0 <= self.t0 and self.tf <= motion.tf):
                raise ValueError("the motion's span [{}, {}] must contain the curve's, [{}, {}]"
                                 .format(motion.t0, motion.tf, self.t0, self.tf))
            Q = _ctx().bern_restrict(motion.cpts, (motion.t0, motion.tf), (self.t0, self.tf))
            r = _ctx().bern_keep_out_moving(self.cpts, H, Q, eps_rel=float(eps), max_nodes=int(max_nodes))
        _raise_md(r['status'][0], 'keepOutClearance')
        return float(r['val'][0]), float(r['t_star'][0])

    def proximityMargin(self, target, radius, kind='reach', window=(0.0, 1.0), eps=1e-12, max_nodes=100000):
        """(margin, t): the certified extremum over the window (tau0, tau1) of the curve's normalised parameter of
        g = (dim/2) (radius^2 - |c - target|^2) and the parameter in [0, 1] where it is attained (obtg_proximity_true, the
        search behind BezOptimization.proximityConstraints).  kind='reach': the maximum -- >= 0 iff the curve comes within the
        Euclidean `radius` of the target at some time of the window; kind='within': the minimum -- >= 0 iff it never leaves that
        range.  target: a point of the curve's dimension, or a Bezier of the same dimension, degree and span (the distance is
        then taken at equal times).  Dimension 2 or 3.  Not in the reference."""
        if kind not in ('reach', 'within'):
            raise ValueError("kind must be 'reach' or 'within', not {!r}".format(kind))
        if self.dim not in (2, 3):
            raise ValueError('The input curve must be two or three dimensional,\n'
                             'instead it is {} dimensional'.format(self.dim))
        code = _capi.PROX_REACH if kind == 'reach' else _capi.PROX_WITHIN
        if isinstance(target, Bezier):
            if target.dim != self.dim or target.deg != self.deg or (target.t0, target.tf) != (self.t0, self.tf):
                raise ValueError('proximityMargin needs a target curve of the same dimension, degree and span')
            Y, n_veh, b, pts = np.vstack((self.cpts, target.cpts)), 2, 1, None
        else:
            pts = np.asarray(target, dtype=np.float64).reshape(-1)
            if pts.shape != (self.dim,):
                raise ValueError('proximityMargin needs a target point of dimension {} or a Bezier'.format(self.dim))
            Y, n_veh, b = self.cpts, 1, 1
        ctx = _capi.Context(n_veh, self.dim, self.deg, 0, device=_capi.default_device())
        try:
            tables = (np.array([[0, b, code]], np.int32), np.array([[float(radius), float(window[0]), float(window[1])]]),
                      np.zeros((0, self.dim)) if pts is None else pts[None])
            r = ctx.proximity_true(Y, tables, eps_rel=float(eps), max_nodes=int(max_nodes))
        finally:
            ctx.close()
        _raise_md(r['status'][0, 0], 'proximityMargin')
        return float(r['val'][0, 0]), float(r['t_star'][0, 0])

    def split(self, tDiv):
        """Two curves, before and after tDiv (bezier.py:533-572): de Casteljau at (tDiv - t0)/(tf - t0); the
        pieces keep the original span's ends, [t0, tDiv] and [tDiv, tf]."""
        if np.isnan(tDiv):
            print('[!] Warning, tDiv is {}, changing to 0.'.format(tDiv))
            tDiv = 0
        left, right = _ctx().bern_split(self.cpts, (tDiv - self.t0) / (self.tf - self.t0))
        return Bezier(left, t0=self.t0, tf=tDiv), Bezier(right, t0=tDiv, tf=self.tf)

    def normSquare(self):
        """(d/2) * |curve|^2 as a 1 x (2n+1) curve -- the reference's factor is kept (bezier.py:869-889)."""
        new = self.copy()
        new.cpts = _ctx().bern_normsq(self.cpts)
        return new

    # ---- distances (bezier.py:840-857)
    def _padded(self):
        c = np.zeros((3, self.deg + 1))
        c[:self.dim] = self.cpts
        return c

    def minDist(self, otherCurve, eps=1e-9, max_depth=128, max_nodes=4000000, robust=False):
        """(dist, t1, t2).  Default: the reference's `_minDist` step for step (bezier.py:1283-1408), including
        its non-minimal answers; the curves may differ in degree (obtg_min_dist_mixed).  robust=True:
        obtg_min_dist_robust, the true minimum within relative eps (on unequal degrees: the lower curve elevated)."""
        if self.dim < 2 or self.dim > 3 or otherCurve.dim < 2 or otherCurve.dim > 3:
            raise ValueError('Both curves must be either 2D or 3D, not {}D and {}D.'.format(self.dim, otherCurve.dim))
        if robust:
            r = _ctx().min_dist_robust(elevated_stack([self._padded(), otherCurve._padded()]), [0], [1], eps=eps,
                                       max_nodes=max_nodes)
            if r['status'][0] != _capi.MD_OK:
                raise RuntimeError('minDist(robust): search budget exhausted (curves coincide over a stretch?); '
                                   'best distance so far %g' % r['res'][0][0])
            a, t1, t2 = r['res'][0]
            return (float(a), float(t1), float(t2))
        if self.deg != otherCurve.deg:
            r = _ctx().min_dist_mixed([self._padded(), otherCurve._padded()], [0], [1], eps=eps,
                                      max_depth=max_depth, max_nodes=max_nodes)
        else:
            r = _ctx().min_dist(np.stack([self._padded(), otherCurve._padded()]), [0], [1], eps=eps,
                                max_depth=max_depth, max_nodes=max_nodes)
        _raise_md(r['status'][0])
        a, t1, t2 = r['res'][0]
        return (float(a), float(t1), float(t2))

    def minDist2Poly(self, poly, eps=1e-6, max_depth=128, max_nodes=4000000, robust=False):
        """(dist, t, closest point on the polygon).  Default: the reference's `_minDist2Poly` step for step
        (bezier.py:1411-1496).  robust=True: obtg_min_dist2poly_robust, the true minimum within relative eps."""
        poly = np.asarray(poly, dtype=float)
        if robust:
            r = _ctx().min_dist2poly_robust(self._padded()[None], poly, [0, poly.shape[0]], [0], [0], eps=min(eps, 1e-9),
                                            max_nodes=max_nodes)
            if r['status'][0] != _capi.MD_OK:
                raise RuntimeError('minDist2Poly(robust): search budget exhausted; best distance so far %g' % r['res'][0][0])
            res = r['res'][0]
            return (float(res[0]), float(res[1]), res[2:].copy())
        r = _ctx().min_dist2poly(self._padded()[None], poly, [0, poly.shape[0]], [0], [0], eps=eps,
                                 max_depth=max_depth, max_nodes=max_nodes)
        _raise_md(r['status'][0])
        res = r['res'][0]
        return (float(res[0]), float(res[1]), res[2:].copy())

    # ---- extrema of one coordinate (bezier.py:631-667 min, 727-763 max)
    def _extremum(self, dim, tol, want_max, what):
        row = self.cpts[dim]                      # IndexError for a dimension the curve does not have, as in the reference
        r = _ctx().bern_extrema(np.atleast_2d(row), want_max=want_max, eps_rel=0.0, eps_abs=float(tol))
        _raise_md(r['status'][0], what)
        return float(r['val'][0])

    def min(self, dim=0, globMin=-np.inf, tol=1e-6):
        """The minimum of coordinate `dim` over the curve, within the absolute tolerance `tol` above it (never below).
        The reference's signature; `globMin` is its recursion plumbing, accepted and ignored.  See the module docstring:
        this is the true minimum, which the reference's recursion is not."""
        return self._extremum(dim, tol, False, 'min')

    def max(self, dim=0, globMax=np.inf, tol=1e-6):
        """The maximum of coordinate `dim` over the curve, within `tol` below it; `globMax` accepted and ignored."""
        return self._extremum(dim, tol, True, 'max')

    # ---- collision checks (bezier.py:859-867)
    def collCheck(self, otherCurve, max_nodes=4000000, robust=False):
        """What the reference's `_collCheckBez2Bez` returns (bezier.py:1561-1614), step for step: 1 when no collision is
        found -- so test `== 1` -- else -1 (its recursion counter passed 100), 0.0 or the smallest end-point distance met
        on the way (a value below 1 does NOT mean that the curves touch).  A search the reference does not come back from
        raises, as minDist does.  robust=True is NOT the reference's value: 1 when obtg_min_dist_robust's true minimum
        distance is above its own "the curves touch" tolerance, 1e-9 x the largest coordinate, else 0."""
        if self.dim < 2 or self.dim > 3 or otherCurve.dim < 2 or otherCurve.dim > 3:
            raise ValueError('Both curves must be either 2D or 3D, not {}D and {}D.'.format(self.dim, otherCurve.dim))
        if self.deg != otherCurve.deg and not robust:
            raise ValueError('collCheck takes curves of equal degree (got {} and {}); collCheck(robust=True) takes any two'
                             .format(self.deg, otherCurve.deg))
        curves = elevated_stack([self._padded(), otherCurve._padded()])
        if robust:
            r = _ctx().min_dist_robust(curves, [0], [1], eps=1e-9, max_nodes=max_nodes)
            if r['status'][0] != _capi.MD_OK:
                raise RuntimeError('collCheck(robust): search budget exhausted (curves coincide over a stretch?)')
            return 1 if r['res'][0][0] > 1e-9 * np.abs(curves).max() else 0
        r = _ctx().coll_check(curves, [0], [1], max_nodes=max_nodes)
        _raise_md(r['status'][0], 'collCheck')
        v = float(r['res'][0])
        return int(v) if v in (1.0, -1.0) else v

    def collCheck2Poly(self, poly, max_nodes=4000000, robust=False):
        """What the reference's `_collCheckBez2Poly` returns (bezier.py:1617-1651), step for step: 1 when no collision is
        found, else 0.  A search the reference does not come back from raises, as minDist2Poly does.  robust=True is NOT
        the reference's value: 1 when obtg_min_dist2poly_robust's true minimum distance to the polygon's convex hull is
        above 1e-9 x the largest coordinate, else 0."""
        poly = np.asarray(poly, dtype=float)
        if robust:
            r = _ctx().min_dist2poly_robust(self._padded()[None], poly, [0, poly.shape[0]], [0], [0], eps=1e-9,
                                            max_nodes=max_nodes)
            if r['status'][0] != _capi.MD_OK:
                raise RuntimeError('collCheck2Poly(robust): search budget exhausted')
            return 1 if r['res'][0][0] > 1e-9 * max(np.abs(self.cpts).max(), np.abs(poly).max()) else 0
        r = _ctx().coll_check2poly(self._padded()[None], poly, [0, poly.shape[0]], [0], [0], max_nodes=max_nodes)
        _raise_md(r['status'][0], 'collCheck2Poly')
        return int(r['res'][0])


def halfspacesOfPolygon(vertices):
    """(A[F][2], b[F]) with unit outward normals: the convex polygon with the given vertices, in order, in either orientation,
    as the half-planes a_f . p <= b_f -- face f through vertices f and f + 1 -- that BezOptimization(keepOut=...),
    Bezier.keepOutClearance and keepIn take.  ValueError for fewer than 3 vertices, a repeated vertex or an order that is not
    convex (collinear neighbours included).  Host arithmetic only: no device is touched."""
    V = np.asarray(vertices, dtype=np.float64)
    if V.ndim != 2 or V.shape[1] != 2 or V.shape[0] < 3:
        raise ValueError('halfspacesOfPolygon needs at least 3 vertices [n][2], not shape {}'.format(V.shape))
    n = V.shape[0]
    for i in range(n):
        for j in range(i + 1, n):
            if np.array_equal(V[i], V[j]):
                raise ValueError('halfspacesOfPolygon: vertices {} and {} are the same point'.format(i, j))
    E = np.roll(V, -1, axis=0) - V                      # edge f: vertex f -> vertex f + 1
    E2 = np.roll(E, -1, axis=0)
    turn = E[:, 0] * E2[:, 1] - E[:, 1] * E2[:, 0]
    if not (np.all(turn > 0.0) or np.all(turn < 0.0)):
        raise ValueError('halfspacesOfPolygon: the vertices are not in a convex order')
    if abs(np.sum(np.arctan2(turn, np.sum(E * E2, axis=1)))) > 2.0 * np.pi + 1e-6:
        raise ValueError('halfspacesOfPolygon: the vertices are not in a convex order')      # (winds more than once)
    sgn = 1.0 if turn[0] > 0.0 else -1.0                # counter-clockwise: the outward normal is the edge turned by -90 degrees
    A = sgn * np.stack((E[:, 1], -E[:, 0]), axis=1)
    A /= np.hypot(A[:, 0], A[:, 1])[:, None]
    return A, np.sum(A * V, axis=1)


def elevated_stack(curves):
    """Padded curves [3][K_i] -> one array [n][3][max K_i]: the shorter ones degree-elevated to the longest (bezier.py:469-495
    through obtg_bern_elev; a curve and its parameterisation do not change under elevation).  One device call per LENGTH
    that occurs, all curves of that length as its rows.  Equal lengths: np.stack."""
    K = max(c.shape[1] for c in curves)
    out = np.empty((len(curves), 3, K))
    for k in set(c.shape[1] for c in curves):
        idx = [i for i, c in enumerate(curves) if c.shape[1] == k]
        rows = np.concatenate([curves[i] for i in idx])
        out[idx] = (rows if k == K else _ctx().bern_elev(rows, K - k)).reshape(len(idx), 3, K)
    return out


def _temporalAlignment(c1, c2):
    """The reference's function of the same name (bezier.py:903-941): both curves cut down to the overlap
    [max t0, min tf] of their spans -> (Bezier, Bezier) on that span.  One device call for the two curves
    (obtg_bern_restrict: the reference's cut order -- what lies before the overlap is split off first, then what lies
    after it; an end that already is the overlap's is left alone).  The spans must overlap (t0 < tf of the result): the
    reference extrapolates there and its callers then return None, which `add` / `sub` here do without calling this."""
    t0, tf = max(c1.t0, c2.t0), min(c1.tf, c2.tf)
    if c1.dim != c2.dim or c1.deg != c2.deg:      # (one batched call: rows of equal length)
        parts = [_ctx().bern_restrict(c.cpts, (c.t0, c.tf), (t0, tf)) for c in (c1, c2)]
    else:
        rows = np.concatenate([c1.cpts, c2.cpts])
        spans = np.repeat([(c1.t0, c1.tf), (c2.t0, c2.tf)], c1.dim, axis=0)
        out = _ctx().bern_restrict(rows, spans, (t0, tf))
        parts = [out[:c1.dim], out[c1.dim:]]
    return Bezier(parts[0], t0=t0, tf=tf), Bezier(parts[1], t0=t0, tf=tf)


def _raise_md(status, what='minDist'):
    if status == _capi.MD_OK:
        return
    if status == _capi.MD_DEPTH_CAP:
        raise RecursionError(what + ': subdivision deeper than max_depth (the reference overflows its stack here)')
    if status == _capi.MD_NODE_CAP:
        raise RuntimeError(what + ': node budget exhausted (the reference does not return on this input)')
    raise RuntimeError(what + ': an inner gjkNew did not converge (the reference loops forever here)')


class RationalBezier(BezierParams):
    """Container for control points + weights (bezier.py:894-900)."""

    def __init__(self, cpts=None, weights=None, tau=None, tf=1.0):
        super(RationalBezier, self).__init__(cpts=cpts, tau=tau, tf=tf)
        self._weights = np.array(weights, ndmin=2)
