"""The yardstick of the single-curve Bernstein algebra (obtg_bern_elev / diff / mul / normsq / split / restrict / eval) and
of the objectives (obtg_euclidean_obj / accel_obj / jerk_obj): every operation in EXACT arithmetic, with the forward-error
bound a float64 evaluation of the same formula has to meet.  No device, no oracle, no reference code.

A float64 is a dyadic rational, so a row is a list of Python integers over a common power of two and every operation here
is integer arithmetic; only the last step (a quotient by a binomial, by T, or a sum of such quotients) leaves the integers.
For every output element an operation returns

    value     the exact value,
    majorant  M: the same formula on absolute values -- every subtraction a sum of magnitudes, |z| and |1 - z| for z, 1 - z,
    count     K: the number of rounded operations on the element's longest dependency chain in the device's kernel.

A candidate c passes when |c - value| <= K * 2^-53 * M, element by element (M == 0 demands equality): the standard forward
bound of a sum of products whose every operation is rounded once -- (1 + u)^K - 1 <= K u / (1 - K u), and K u < 1e-12 here,
which the slack between the counted K and the K granted below covers many times over.  A derivation, not a measurement.

The counts, against csrc/bern_kernels.hip (u = one rounding; a binomial table entry is one rounding of a long-double chain,
tables.cpp binom(): at most 1 u; a fused multiply-add only lowers a count):

  elev, mul   k_bern_elev / k_bern_mul: `lds[e] = a[e] * bn[e]` 2 (entry, product); conv_at's chain of T_k fma: T_k, its
              other operand's entry 1 (mul: 2); `/ bo[k]` 2 (entry, quotient)                    -> T_k + 6 <= T_k + 10 granted
  normsq      k_bern_normsq: scaled operands 2 each; d chains of T_k fma joined by d sums: d T_k + d - 1 counted as d T_k + 2
              for d <= 3; `(0.5 d) * s` 1; `/ bo[k]` 2                                           -> d T_k + 9 <= d T_k + 12
  diff        k_bern_diff: `val = n / T` 1; `s[c] * (-val) + s[c+1] * val` 2; `c / n` 1, its product 1, the sum 1
                                                                                                 -> 6 <= 8
  split       k_bern_split: `w = 1 - z` 1 (the reference keeps 1 - z exact); per level `w * cur[i] + z * cur[i+1]` 2, and
              w's own rounding enters every level once more: 3 per level                         -> 3 level + 1 <= 4 level + 2
  eval        k_bern_eval: t = fl(fl(tau - t0) / fl(tf - t0)) is formed here exactly as there (correctly rounded division);
              `u = 1 - t` 1, then n levels as split                                              -> 3 n + 1 <= 4 n + 2
  restrict    k_bern_restrict: SpanCut's zh, zt formed here in float64 as there; split_keep_lds twice.  Element k of the
              second cut depends on elements 0..k of the first, whose largest count is its element 0's:
              head only 4 (n - j) + 2, tail only 4 k + 2, both (4 n + 2) + (4 k + 2)
  euclidean   k_euclid: per segment `dim` differences 1, fma chain dim, sqrt 1; lane sum of ceil(n_veh n / 64) terms and 6
              shuffle steps <= n_veh n                                                           -> n_veh n + dim + 4,
              relative to the (positive) sum itself; the square roots in `decimal` at 60 digits
  deriv_energy launch_deriv_energy_obj: `order` times diff 8 each (the last inside the speed kernel), the speed kernel's
              product d (n + 1) + 12 and elevation (2 n + 1) + 10, k_rowsum's n_veh (2 n + R + 1) terms in lane-strided
              sums and 6 shuffle steps <= (2 n + R + 1) + n_veh
                                   -> 8 order + (dim (n + 1) + 12) + (2 n + 11) + (2 n + R + 1) + n_veh, on the majorant of the sum
"""
import decimal
import functools
import math
import operator
from fractions import Fraction

import numpy as np

UNIT_BITS = 53                      # the bound's unit is 2^-53


# ---------------------------------------------------------------------------------------------------------------------
#  exact results and the comparison
# ---------------------------------------------------------------------------------------------------------------------
class Ref(object):
    """Per output element (flat, C order over `shape`): value = num / den * 2^e, majorant = mnum / den * 2^e, count K."""

    def __init__(self, num, den, mnum, e, K, shape):
        self.num, self.den, self.mnum, self.e, self.K, self.shape = num, den, mnum, e, K, tuple(shape)
        assert len(num) == len(den) == len(mnum) == len(K) == int(np.prod(self.shape))

    @classmethod
    def from_fractions(cls, val, maj, K, shape):
        num = [v.numerator * m.denominator for v, m in zip(val, maj)]
        mnum = [m.numerator * v.denominator for v, m in zip(val, maj)]
        den = [v.denominator * m.denominator for v, m in zip(val, maj)]
        return cls(num, den, mnum, 0, K, shape)

    def value(self, i):
        return Fraction(self.num[i], self.den[i]) * Fraction(2) ** self.e

    def majorant(self, i):
        return Fraction(self.mnum[i], self.den[i]) * Fraction(2) ** self.e

    def nearest(self):
        """The exact values rounded to float64 (for building wrong answers, never for judging one)."""
        return np.array([float(self.value(i)) for i in range(len(self.num))]).reshape(self.shape)


def shares(cand, ref):
    """|cand - value| / (K 2^-53 M) per element, as floats for the record (inf where M == 0 and cand != value, or cand is
    not finite), and the exact verdict per element."""
    c = np.asarray(cand, dtype=np.float64)
    assert c.shape == ref.shape, "shape %s, expected %s" % (c.shape, ref.shape)
    out = np.zeros(c.size)
    ok = np.ones(c.size, dtype=bool)
    up, dn = (1 << ref.e, 1) if ref.e >= 0 else (1, 1 << -ref.e)
    for i, x in enumerate(c.reshape(-1).tolist()):
        if not math.isfinite(x):
            out[i], ok[i] = math.inf, False
            continue
        p, q = x.as_integer_ratio()
        # |p / q - num / den * up / dn| * 2^53 <= K * mnum / den * up / dn, cleared of denominators
        lhs = abs(p * ref.den[i] * dn - ref.num[i] * up * q) << UNIT_BITS
        rhs = ref.K[i] * ref.mnum[i] * up * q
        ok[i] = lhs <= rhs
        out[i] = (lhs / rhs) if rhs else (0.0 if lhs == 0 else math.inf)
    return out.reshape(ref.shape), ok.reshape(ref.shape)


def share(cand, ref):
    """Largest share of the bound used (<= 1 passes)."""
    s, ok = shares(cand, ref)
    worst = float(s.max()) if s.size else 0.0
    return worst if ok.all() else max(worst, 1.0 + 1e-12)


def assert_within(cand, ref, what=""):
    """Assert the element-wise bound; returns the largest share of it that was used."""
    s, ok = shares(cand, ref)
    if not ok.all():
        i = int(np.argmax(np.where(ok, -1.0, s).reshape(-1)))
        raise AssertionError("%s: %d of %d elements outside K * 2^-53 * M; worst at flat index %d: got %r, exact %r, K = %d, "
                             "share of the bound %.3g" % (what, int((~ok).sum()), ok.size, i,
                                                          float(np.asarray(cand, dtype=np.float64).reshape(-1)[i]),
                                                          float(ref.value(i)), ref.K[i], s.reshape(-1)[i]))
    return float(s.max()) if s.size else 0.0


def within(cand, ref):
    return bool(shares(cand, ref)[1].all())


def pair_within(x, y, ref):
    """|x - y| <= 2 K 2^-53 M element by element: two candidates of the same exact value, each granted its bound"""
    x, y = (np.asarray(t, dtype=np.float64).reshape(-1) for t in (x, y))
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return False
    unit = Fraction(1, 1 << (UNIT_BITS - 1))
    return all(abs(Fraction(a) - Fraction(b)) <= ref.K[i] * unit * ref.majorant(i) for i, (a, b) in enumerate(zip(x.tolist(), y.tolist())))


# ---------------------------------------------------------------------------------------------------------------------
#  integers
# ---------------------------------------------------------------------------------------------------------------------
def _ints(x):
    """float64 array -> (flat list of ints v, e): x_i = v_i * 2^e, e <= 0"""
    fr = [float(t).as_integer_ratio() for t in np.asarray(x, dtype=np.float64).reshape(-1)]
    s = max([q.bit_length() - 1 for _, q in fr] + [0])
    return [p << (s - (q.bit_length() - 1)) for p, q in fr], -s


def _dyadic(z):
    """float -> (p, s): z = p / 2^s"""
    p, q = float(z).as_integer_ratio()
    return p, q.bit_length() - 1


def _binrow(n):
    return [math.comb(n, k) for k in range(n + 1)]


def _conv(A, B):
    """sum_j A[j] B[k - j], k < len(A) + len(B) - 1"""
    la, lb = len(A), len(B)
    Br = B[::-1]
    out = []
    for k in range(la + lb - 1):
        j0, j1 = max(0, k - (lb - 1)), min(la - 1, k)
        out.append(sum(map(operator.mul, A[j0:j1 + 1], Br[lb - 1 - k + j0:lb - k + j1])))
    return out


def _terms(la, lb, k):
    return min(la - 1, k) - max(0, k - (lb - 1)) + 1


def _absl(v):
    return [abs(t) for t in v]


def _memo(fn):
    """Reference results cached per input (arrays by their bytes)."""
    cache = {}

    @functools.wraps(fn)
    def wrapped(*args):
        key = tuple((a.shape, a.tobytes()) if isinstance(a, np.ndarray) else a for a in args)
        if key not in cache:
            cache[key] = fn(*args)
        return cache[key]
    return wrapped


def _f2(a):
    return np.atleast_2d(np.ascontiguousarray(a, dtype=np.float64))


# ---------------------------------------------------------------------------------------------------------------------
#  the single-curve algebra
# ---------------------------------------------------------------------------------------------------------------------
@_memo
def _elev(a, R):
    rows, nc = a.shape
    n = nc - 1
    v, e = _ints(a)
    bn, bR, bo = _binrow(n), _binrow(R), _binrow(n + R)
    num, mnum, den, K = [], [], [], []
    for r in range(rows):
        A = [v[r * nc + j] * bn[j] for j in range(nc)]
        num += _conv(A, bR)
        mnum += _conv(_absl(A), bR)
        den += bo
        K += [_terms(nc, R + 1, k) + 10 for k in range(nc + R)]
    return Ref(num, den, mnum, e, K, (rows, nc + R))


def elev(a, R):
    """elev(a, R)[k] = sum_j a_j C(n, j) C(R, k - j) / C(n + R, k), every row of a[rows][n + 1]; K = T_k + 10"""
    return _elev(_f2(a), int(R))


@_memo
def _mul(a, b):
    rows, mc = a.shape
    nc = b.shape[1]
    va, ea = _ints(a)
    vb, eb = _ints(b)
    bm, bn, bo = _binrow(mc - 1), _binrow(nc - 1), _binrow(mc + nc - 2)
    num, mnum, den, K = [], [], [], []
    for r in range(rows):
        A = [va[r * mc + j] * bm[j] for j in range(mc)]
        B = [vb[r * nc + j] * bn[j] for j in range(nc)]
        num += _conv(A, B)
        mnum += _conv(_absl(A), _absl(B))
        den += bo
        K += [_terms(mc, nc, k) + 10 for k in range(mc + nc - 1)]
    return Ref(num, den, mnum, ea + eb, K, (rows, mc + nc - 1))


def mul(a, b):
    """mul(a, b)[k] = sum_j a_j b_{k-j} C(m, j) C(n, k - j) / C(m + n, k), row by row; K = T_k + 10"""
    a, b = _f2(a), _f2(b)
    assert a.shape[0] == b.shape[0]
    return _mul(a, b)


def _normsq_nums(rows_v, nc):
    """d * sum_q conv(C(n, .) x_q, C(n, .) x_q) of integer rows: twice C(2n, k) times the (d/2)-scaled coefficient"""
    bn = _binrow(nc - 1)
    d = len(rows_v)
    tot = [0] * (2 * nc - 1)
    for x in rows_v:
        A = [x[j] * bn[j] for j in range(nc)]
        tot = list(map(operator.add, tot, _conv(A, A)))
    return [d * t for t in tot]


@_memo
def _normsq(x):
    d, nc = x.shape
    v, e = _ints(x)
    rows_v = [v[q * nc:(q + 1) * nc] for q in range(d)]
    num = _normsq_nums(rows_v, nc)
    mnum = _normsq_nums([_absl(r) for r in rows_v], nc)
    den = [2 * c for c in _binrow(2 * nc - 2)]
    K = [d * _terms(nc, nc, k) + 12 for k in range(2 * nc - 1)]
    return Ref(num, den, mnum, 2 * e, K, (1, 2 * nc - 1))


def normsq(x):
    """normsq(x)[k] = (d / 2) sum_q mul(x_q, x_q)[k] of x[d][n + 1] (the reference's factor); K = d T_k + 12"""
    return _normsq(_f2(x))


def _diff_nums(v, m, n):
    """T * diff of one integer row v (magnitudes m): c (v_c - v_{c-1}) + (n - c) (v_{c+1} - v_c), and its majorant"""
    num, mnum = [], []
    for c in range(n + 1):
        s = t = 0
        if c > 0:
            s += c * (v[c] - v[c - 1])
            t += c * (m[c] + m[c - 1])
        if c < n:
            s += (n - c) * (v[c + 1] - v[c])
            t += (n - c) * (m[c + 1] + m[c])
        num.append(s)
        mnum.append(t)
    return num, mnum


@_memo
def _diff(a, T):
    rows, nc = a.shape
    v, e = _ints(a)
    Tp, Ts = _dyadic(T)
    sgn = 1 if Tp > 0 else -1
    num, mnum = [], []
    for r in range(rows):
        row = v[r * nc:(r + 1) * nc]
        s, t = _diff_nums(row, _absl(row), nc - 1)
        num += [sgn * x for x in s]
        mnum += t
    return Ref(num, [abs(Tp)] * (rows * nc), mnum, e + Ts, [8] * (rows * nc), (rows, nc))


def diff(a, T):
    """diff(a, T)[c]: the derivative (n / T)(a_{c+1} - a_c) elevated by 1 = (c (a_c - a_{c-1}) + (n - c)(a_{c+1} - a_c)) / T; K = 8"""
    a = _f2(a)
    assert a.shape[1] >= 2 and T != 0
    return _diff(a, float(T))


def _decast(v, m, p, s):
    """de Casteljau of the integer row v (magnitudes m) at z = p / 2^s, 1 - z exact -> left, right, their majorants, all
    over 2^(s n); left[k] is the first element of level k, right[j] (the curve's own orientation) the last of level n - j"""
    n = len(v) - 1
    q = (1 << s) - p
    ap, aq = abs(p), abs(q)
    cur, cm = list(v), list(m)
    L, Lm, R, Rm = [0] * (n + 1), [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    for lev in range(n + 1):
        sh = s * (n - lev)
        L[lev], Lm[lev], R[n - lev], Rm[n - lev] = cur[0] << sh, cm[0] << sh, cur[-1] << sh, cm[-1] << sh
        cur = [q * x + p * y for x, y in zip(cur[:-1], cur[1:])]
        cm = [aq * x + ap * y for x, y in zip(cm[:-1], cm[1:])]
    return L, Lm, R, Rm


@_memo
def _split(a, z):
    rows, nc = a.shape
    n = nc - 1
    v, e = _ints(a)
    p, s = _dyadic(z)
    out = [[], [], [], []]
    for r in range(rows):
        row = v[r * nc:(r + 1) * nc]
        for dst, src in zip(out, _decast(row, _absl(row), p, s)):
            dst += src
    den = [1 << (s * n)] * (rows * nc)
    KL = [4 * k + 2 for k in range(nc)] * rows
    KR = [4 * (n - j) + 2 for j in range(nc)] * rows
    return Ref(out[0], den, out[1], e, KL, (rows, nc)), Ref(out[2], den, out[3], e, KR, (rows, nc))


def split(a, z):
    """-> (left, right) of every row at the float z, w = 1 - z exact; K = 4 level + 2 (left[k]: k, right[j]: n - j)"""
    return _split(_f2(a), float(z))


def eval_t(tau, t0, tf):
    """The parameter as the kernel forms it: fl(fl(tau - t0) / fl(tf - t0)) (NumPy float64: IEEE, correctly rounded)"""
    tau = np.atleast_1d(np.asarray(tau, dtype=np.float64)).reshape(-1)
    with np.errstate(all="ignore"):
        return (tau - np.float64(t0)) / (np.float64(tf) - np.float64(t0))


@_memo
def _eval(a, t):
    rows, nc = a.shape
    n = nc - 1
    v, e = _ints(a)
    m = _absl(v)
    bn = _binrow(n)
    cols = []
    for tk in t.tolist():
        p, s = _dyadic(tk)
        q = (1 << s) - p
        pw, qw = [1], [1]
        for _ in range(n):
            pw.append(pw[-1] * p)
            qw.append(qw[-1] * q)
        W = [bn[i] * pw[i] * qw[n - i] for i in range(nc)]            # C(n, i) z^i (1 - z)^(n - i), over 2^(s n)
        Wa = _absl(W)
        cols.append(([sum(map(operator.mul, v[r * nc:(r + 1) * nc], W)) for r in range(rows)],
                     [sum(map(operator.mul, m[r * nc:(r + 1) * nc], Wa)) for r in range(rows)], 1 << (s * n)))
    num = [c[0][r] for r in range(rows) for c in cols]
    mnum = [c[1][r] for r in range(rows) for c in cols]
    den = [c[2] for r in range(rows) for c in cols]
    return Ref(num, den, mnum, e, [4 * n + 2] * len(num), (rows, len(cols)))


def eval_curve(a, tau, t0, tf):
    """Every row at every tau: de Casteljau at t = eval_t(tau, t0, tf), whose exact value and majorant are the Bernstein sums
    sum_i a_i C(n, i) t^i (1 - t)^(n - i) and sum_i |a_i| C(n, i) |t|^i |1 - t|^(n - i); K = 4 n + 2"""
    return _eval(_f2(a), eval_t(tau, t0, tf))


def span_cut(span, target):
    """SpanCut of bern_kernels.hip in float64: (head, zh, tail, zt)"""
    t0, tf, a, e = (np.float64(x) for x in (span[0], span[1], target[0], target[1]))
    head = bool(t0 < a)
    zh = float((a - t0) / (tf - t0))
    if head:
        t0 = a
    tail = bool(tf > e)
    zt = float((e - t0) / (tf - t0))
    return head, zh, tail, zt


@_memo
def _restrict(a, span, target):
    rows, nc = a.shape
    n = nc - 1
    v, e = _ints(a)
    num, mnum, den, K = [], [], [], []
    for r in range(rows):
        row = v[r * nc:(r + 1) * nc]
        mag = _absl(row)
        head, zh, tail, zt = span_cut(span[r], target[r])
        d = 1
        k = [0] * nc
        if head:
            p, s = _dyadic(zh)
            _, _, row, mag = _decast(row, mag, p, s)
            d <<= s * n
            k = [4 * (n - j) + 2 for j in range(nc)]
        if tail:
            p, s = _dyadic(zt)
            row, mag, _, _ = _decast(row, mag, p, s)
            d <<= s * n
            k = [max(k) + 4 * j + 2 for j in range(nc)]
        num += row
        mnum += mag
        den += [d] * nc
        K += k
    return Ref(num, den, mnum, e, K, (rows, nc))


def restrict(a, span, target):
    """Every row of a, a curve on span[r] = (t0, tf), cut down to target[r] = (a, e) by the two cuts of SpanCut in its order
    (one span / target for all rows, or one per row).  A row that takes no cut is the input (K = 0: equality)."""
    a = _f2(a)
    span = np.ascontiguousarray(np.broadcast_to(np.asarray(span, dtype=np.float64).reshape(-1, 2), (a.shape[0], 2)))
    target = np.ascontiguousarray(np.broadcast_to(np.asarray(target, dtype=np.float64).reshape(-1, 2), (a.shape[0], 2)))
    return _restrict(a, span, target)


# ---------------------------------------------------------------------------------------------------------------------
#  the objectives: Y[n_veh * dim][n + 1], one iterate
# ---------------------------------------------------------------------------------------------------------------------
@_memo
def _euclidean(Y, n_veh, dim):
    nc = Y.shape[1]
    n = nc - 1
    v, e = _ints(Y)
    ctx = decimal.Context(prec=60)
    tot = decimal.Decimal(0)
    for veh in range(n_veh):
        for i in range(n):
            q = sum((v[(veh * dim + j) * nc + i + 1] - v[(veh * dim + j) * nc + i]) ** 2 for j in range(dim))
            tot = ctx.add(tot, ctx.sqrt(decimal.Decimal(q)))          # (an integer: Decimal holds it exactly)
    S = Fraction(tot) * Fraction(2) ** e
    return Ref.from_fractions([S], [S], [n_veh * n + dim + 4], (1,))


def euclidean_obj(Y, n_veh, dim):
    """sum over vehicles and segments of |P_{i+1} - P_i|; K = n_veh n + dim + 4 relative to the sum itself (60-digit square
    roots: 1e-59 against the bound's 1e-16)"""
    return _euclidean(_f2(Y), int(n_veh), int(dim))


@_memo
def _deriv_energy(Y, n_veh, dim, R, tf, order):
    nc = Y.shape[1]
    n = nc - 1
    v, e = _ints(Y)
    Tp, Ts = _dyadic(tf)
    bR, bo = _binrow(R), _binrow(2 * n + R)
    val = maj = Fraction(0)
    for veh in range(n_veh):
        rows = [v[(veh * dim + q) * nc:(veh * dim + q + 1) * nc] for q in range(dim)]
        mags = [_absl(r) for r in rows]
        for _ in range(order):                                        # each pass: times T (an odd power's sign squares away)
            rows, mags = map(list, zip(*[_diff_nums(r, m, n) for r, m in zip(rows, mags)]))
        N = _conv(_normsq_nums(rows, nc), bR)                         # 2 C(2n + R, k) times the elevated coefficient
        Nm = _conv(_normsq_nums(mags, nc), bR)
        val += sum(Fraction(x, 2 * c) for x, c in zip(N, bo))
        maj += sum(Fraction(x, 2 * c) for x, c in zip(Nm, bo))
    scale = Fraction(2) ** (2 * (e + order * Ts)) / Fraction(Tp) ** (2 * order)
    K = 8 * order + (dim * (n + 1) + 12) + (2 * n + 11) + (2 * n + R + 1) + n_veh
    return Ref.from_fractions([val * scale], [maj * scale], [K], (1,))


def deriv_energy_obj(Y, n_veh, dim, R, tf, order):
    """sum over vehicles of the control points of elev(normsq(diff^order(pos)), R) (order 2: acceleration, 3: jerk)"""
    return _deriv_energy(_f2(Y), int(n_veh), int(dim), int(R), float(tf), int(order))


# ---------------------------------------------------------------------------------------------------------------------
#  the inputs and shapes both test modules use
# ---------------------------------------------------------------------------------------------------------------------
def input_rows(seed, length, rows=4):
    """rows x length: normal(0, 3); uniform(-1, 1) * 1e6; all-positive |normal|; mixed magnitudes uniform(-1, 1) * 10^integers(-6, 7)
    -- the row a tolerance scaled by the largest magnitude cannot see into.  More than four rows: the four kinds in turn."""
    rng = np.random.default_rng(seed)
    out = np.empty((rows, length))
    for r in range(rows):
        kind = r % 4
        if kind == 0:
            out[r] = rng.normal(0, 3, length)
        elif kind == 1:
            out[r] = rng.uniform(-1, 1, length) * 1e6
        elif kind == 2:
            out[r] = np.abs(rng.normal(0, 3, length))
        else:
            out[r] = rng.uniform(-1, 1, length) * 10.0 ** rng.integers(-6, 7, length)
    return out


ELEV_SHAPES = [(0, 0), (0, 5), (1, 1), (5, 58), (10, 53), (10, 54), (15, 100), (62, 1), (63, 1), (64, 1), (20, 200), (100, 100),
               (127, 129)]
MUL_SHAPES = [(0, 0), (0, 7), (7, 0), (3, 10), (10, 3), (31, 32), (32, 32), (40, 23), (63, 64), (100, 27), (100, 100)]
NORMSQ_SHAPES = [(1, 0), (1, 5), (2, 10), (3, 31), (3, 32), (2, 40), (3, 70)]
DIFF_DEGREES = [1, 2, 5, 63, 64, 65, 130]
DIFF_T = [1.0, 7.3, 0.013]
SPLIT_DEGREES = [0, 1, 2, 31, 63, 64, 65, 128, 200]
SPLIT_Z = [0.0, 1.0, 0.3, 0.5, 2.0 ** -30, 1.0 - 2.0 ** -30, -0.25, 1.5]


def split_z(n):
    return [0.3, 1.0 - 2.0 ** -30] if n == 200 else SPLIT_Z


EVAL_NC = [1, 2, 3, 64, 65, 124, 125]
EVAL_NTAU = [1, 63, 64, 65]                  # and 1001: Bezier.curve on its default grid
EVAL_SPANS = [(0.0, 1.0), (2.5, 9.75)]


def eval_tau(n_tau, t0, tf):
    """n_tau samples of [t0, tf]: both ends (n_tau >= 2), inner points, and -- from 5 samples on -- two outside the span"""
    if n_tau == 1:
        return np.array([t0 + 0.37 * (tf - t0)])
    tau = np.linspace(t0, tf, n_tau)
    if n_tau >= 5:
        tau[1], tau[-2] = t0 - 0.0625 * (tf - t0), tf + 0.125 * (tf - t0)
    return tau


RESTRICT_NC = [1, 6, 64, 65, 130]


def restrict_cases(rows):
    """One (span, target) per row, the five kinds in turn: head only, tail only, both, neither, a target 2^-20 of the span"""
    span, target = np.empty((rows, 2)), np.empty((rows, 2))
    for r in range(rows):
        t0, tf = 0.5 + 0.25 * r, 4.0 + 0.75 * r
        w = tf - t0
        span[r] = t0, tf
        target[r] = [(t0 + 0.3 * w, tf), (t0, t0 + 0.55 * w), (t0 + 0.2 * w, t0 + 0.9 * w), (t0, tf),
                     (t0 + 0.4 * w, t0 + 0.4 * w + w * 2.0 ** -20)][r % 5]
    return span, target


EUCLID_SHAPES = [(1, 2, 1), (7, 2, 9), (8, 2, 8), (13, 3, 5), (36, 3, 5)]          # 1, 63, 64, 65, 180 segments
# (n_veh, dim, deg, R) of the acceleration and jerk objectives
ENERGY_SHAPES = ([(nv, d, n, R) for (nv, d, n) in [(3, 2, 7), (5, 2, 10), (2, 2, 8), (4, 2, 15)] for R in (0, 30)] +
                 [(nv, d, n, R) for (nv, d, n) in [(2, 3, 5), (4, 3, 20), (3, 2, 6)] for R in (0, 3)] +
                 [(5, 2, 10, 100), (1, 2, 2, 0), (1, 3, 1, 0)])
ENERGY_TF = [1.0, 7.0]
ENERGY_B = 3


def iterates(seed, n_veh, dim, deg, B=ENERGY_B):
    """B distinct iterates [B][n_veh * dim][deg + 1], their rows of the four kinds of input_rows"""
    return input_rows(seed, deg + 1, B * n_veh * dim).reshape(B, n_veh * dim, deg + 1)
