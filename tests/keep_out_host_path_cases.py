"""What tests/test_gpu_keep_out_host_path.py and tests/golden/gen_keep_out_return_codes.py share: a caller of the 26 keep-out
entry points through ctypes (the Python wrappers never pass a null pointer) and the table of return-code cases.

Shapes are tiny: N = 3 vehicles of degree 3, d = 2 and 3, B = 2 rows; the obstacles of keep_out_ref.obstacles(d) (6 items a
row), the regions of pair_keep_out_ref (3 pairs a row), a motion of degree 1 for the first obstacle.  The layout of the
outputs below is written from include/obtg.h, not from the library's column table."""
import ctypes
import math

import numpy as np

import keep_out_ref as K
import pair_keep_out_ref as PK

N, DEG, B = 3, 3, 2
EPS = 1e-12
NODES = 100000
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5

# family -> (entry point without its _jac / _dev endings, Euclidean metric, moving obstacles, vehicle pairs)
FAMILIES = {"static": ("obtg_keep_out_true_min", False, False, False),
            "euclid": ("obtg_keep_out_euclid_true_min", True, False, False),
            "moving": ("obtg_keep_out_moving_true_min", False, True, False),
            "pair": ("obtg_pair_keep_out_true_min", False, False, True),
            "pair_euclid": ("obtg_pair_keep_out_euclid_true_min", True, False, True)}
FREE = {"free": ("obtg_bern_keep_out", False), "free_euclid": ("obtg_bern_keep_out_euclid", False),
        "free_moving": ("obtg_bern_keep_out_moving", True)}
FORMS = [(fam, jac, dev) for fam in FAMILIES for jac in (False, True) for dev in (False, True)]
FREE_FORMS = [(fam, dev) for fam in FREE for dev in (False, True)]


def entry(fam, jac=False, dev=False):
    stem = FAMILIES[fam][0] if fam in FAMILIES else FREE[fam][0]
    return stem + ("_jac" if jac else "") + ("_dev" if dev else "")


def columns(fam, jac, dim, deg=DEG):
    """the outputs of an entry point in the order of its arguments: (name, shape per item, dtype)"""
    _, eu, mv, pr = FAMILIES[fam]
    f8, i4 = np.float64, np.int32
    cols = [("val", (), f8), ("t_star", (), f8)]
    cols += [("faces", (3,), i4), ("dir", (dim,), f8)] if eu else [("face", (2,), i4), ("lam", (), f8)]
    cols += [("bound", (), f8), ("nodes", (), i4), ("status", (), i4)]
    if mv or pr:
        cols.append(("rel", (dim, deg + 1), f8))
    if jac:
        cols.append(("jac", (dim, deg + 1), f8))
        if mv:
            cols.append(("jac_tf", (), f8))
    return cols


def mandatory(fam, jac):
    """the pointers of an entry point that must not be null"""
    return ["Y"] + (["tf"] if FAMILIES[fam][2] else []) + ["val"] + (["jac"] if jac else []) + (["jac_tf"] if jac and FAMILIES[fam][2] else [])


def optional(fam, jac):
    return [name for name, _, _ in columns(fam, jac, 2) if name not in mandatory(fam, jac)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def region(dim):
    return PK.oblique_triangle() if dim == 2 else PK.box113()


def motion(dim):
    """a degree-1 motion of the first obstacle on a span of 2.5; the second stands still"""
    Q = np.array([[0.0, 0.75], [0.0, -0.5], [0.0, 0.25]][:dim]).reshape(-1)
    return Q, np.array([0, 2, 2], np.int32), np.array([2.5, 1.0])


def pyramid():
    """more than 128 features under the Euclidean metric: the 15-sided pyramid of tests/test_gpu_pair_keep_out.py (16 faces, d = 3)"""
    k = 15
    th = 2 * math.pi * np.arange(k) / k
    return np.vstack((np.column_stack((np.cos(th), np.sin(th), np.full(k, 0.5), np.ones(k))), [[0.0, 0.0, -1.0, 1.0]]))


def rows(dim, rows_=B, seed=7, n_veh=N, deg=DEG):
    return K.batch(deg, dim, 100 * dim + seed, n_veh=n_veh, B=rows_)


def spans(rows_=B):
    return 2.0 * (1.0 - 0.0625 * np.arange(rows_))


def make_context(_capi, dim, kind, n_veh=N, deg=DEG):
    """kind: 'plain' -- obstacle tables and a pair region; 'motion' -- and the motion; 'empty' -- nothing set; 'pyramid' -- the
    pyramid as the one obstacle of every vehicle and as the region (d = 3)"""
    ctx = _capi.Context(n_veh, dim, deg, 0, device=0)
    if kind in ("plain", "motion"):
        H, off, VO = K.tables(K.obstacles(dim), n_veh)
        ctx.set_keep_out(H, off, VO)
        ctx.set_pair_keep_out(region(dim))
        if kind == "motion":
            ctx.set_keep_out_motion(*motion(dim))
    elif kind == "pyramid":
        Hp = pyramid()
        ctx.set_keep_out(Hp, np.array([0, len(Hp)], np.int32), np.stack((np.arange(n_veh), np.zeros(n_veh, int)), axis=1).astype(np.int32))
        ctx.set_pair_keep_out(Hp)
    else:
        assert kind == "empty", kind
    return ctx


# ---------------------------------------------------------------------------------------------------------------- the caller
class Buffers(object):
    """Host (NumPy) or device (torch) arrays by name; ptr(name) is what the library takes"""

    def __init__(self, dev):
        self.dev, self.a = dev, {}
        if dev:
            import torch
            self.torch = torch

    def put(self, name, array):
        array = np.ascontiguousarray(array)
        self.a[name] = self.torch.from_numpy(array).to(self.torch.device("cuda", 0)) if self.dev else array
        return self

    def new(self, name, shape, dtype):
        fill = np.full(shape, -12345, dtype) if dtype == np.int32 else np.full(shape, -12345.5, dtype)     # (never a result)
        return self.put(name, fill)

    def ptr(self, name):
        x = self.a[name]
        return ctypes.c_void_p(x.data_ptr() if self.dev else x.ctypes.data)

    def numpy(self, name):
        x = self.a[name]
        return x.cpu().numpy() if self.dev else x


def call(ctx, fam, jac, dev, Y, tf=None, items=None, want=None, null=(), handle=True, **scalars):
    """One call of a context form.  Y[rows][.][.]; items: the items of a row (default: what the context holds); want: the optional
    outputs given a pointer (None: all of them); null: the mandatory pointers passed as null; scalars: B, margin, eps_rel,
    max_nodes in place of the defaults.  -> (return code, {output: array})"""
    rows_ = Y.shape[0]
    _, eu, mv, pr = FAMILIES[fam]
    if items is None:
        items = ctx.n_veh * (ctx.n_veh - 1) // 2 if pr else max(ctx.keep_out_items, 1)
    buf = Buffers(dev).put("Y", Y)
    if mv:
        buf.put("tf", spans(rows_) if tf is None else tf)
    cols = columns(fam, jac, ctx.dim, ctx.deg)
    given = [name for name, _, _ in cols if name in mandatory(fam, jac) or want is None or name in want]
    for name, shape, dtype in cols:
        if name in given:
            buf.new(name, (rows_, max(items, 1)) + shape, dtype)
    p = lambda name: None if name in null or name not in buf.a else buf.ptr(name)      # noqa: E731
    args = [ctx._h if handle else None, p("Y")] + ([p("tf")] if mv else [])
    args += [int(scalars.get("B", rows_)), float(scalars.get("margin", 0.0)), float(scalars.get("eps_rel", EPS)),
             int(scalars.get("max_nodes", NODES))]
    args += [p(name) for name, _, _ in cols]
    if dev:
        ctx.set_stream(buf.torch.cuda.current_stream().cuda_stream)
    try:
        rc = getattr(ctx._lib, entry(fam, jac, dev))(*args)
        if dev:
            buf.torch.cuda.synchronize()
    finally:
        if dev:
            ctx.use_own_stream()
    return rc, {name: buf.numpy(name) for name in given}


def free_inputs(dim, M=4, seed=3):
    """(curves[M][dim][DEG + 1], H of one obstacle, Q[dim][2], r[M])"""
    cv = K.batch(DEG, dim, 50 * dim + seed, n_veh=1, B=M).reshape(M, dim, DEG + 1)
    A, b = K.obstacles(dim)[1]
    H = np.hstack((np.asarray(A, dtype=float), np.asarray(b, dtype=float)[:, None]))
    Q = np.array([[0.0, 0.75], [0.0, -0.5], [0.0, 0.25]][:dim])
    return np.ascontiguousarray(cv), np.ascontiguousarray(H), np.ascontiguousarray(Q), np.linspace(0.5, 1.0, M)


def call_free(ctx, fam, dev, d, want=None, null=(), handle=True, **over):
    """One call of a free-curve form on the inputs of free_inputs(d); over: M, dim, K, F, Km in place of what the arrays say;
    null: of cv, H, Q, r, val.  -> (return code, {output: array})"""
    cv, H, Q, r = free_inputs(d)
    M = cv.shape[0]
    moving = FREE[fam][1]
    buf = Buffers(dev).put("cv", cv)
    host = Buffers(False).put("H", H).put("Q", Q)               # (H and Q are host arrays in both forms)
    (buf if dev else host).put("r", r)
    outs = [("val", np.float64), ("t_star", np.float64), ("status", np.int32)]
    given = [name for name, _ in outs if name == "val" or want is None or name in want]
    for name, dtype in outs:
        if name in given:
            buf.new(name, (M,), dtype)

    def p(name):
        if name in null:
            return None
        for b in (buf, host):
            if name in b.a:
                return b.ptr(name)
        return None
    args = [ctx._h if handle else None, p("cv"), int(over.get("M", M)), int(over.get("dim", d)), int(over.get("K", DEG + 1)), p("H"),
            int(over.get("F", H.shape[0]))]
    if moving:
        args += [p("Q"), int(over.get("Km", Q.shape[1])), p("r")]
    args += [float(over.get("eps_rel", EPS)), int(over.get("max_nodes", NODES))] + [p(name) for name, _ in outs]
    if dev:
        ctx.set_stream(buf.torch.cuda.current_stream().cuda_stream)
    try:
        rc = getattr(ctx._lib, entry(fam, dev=dev))(*args)
        if dev:
            buf.torch.cuda.synchronize()
    finally:
        if dev:
            ctx.use_own_stream()
    return rc, {name: buf.numpy(name) for name in given}


# ---------------------------------------------------------------------------------------------------------------- return codes
class ReturnCodeTable(object):
    """cases: [(case id, thunk -> return code)] over all 26 entry points; every case is either refused before any launch or a
    plainly valid call.  The contexts the thunks need are made on first use and closed by close()."""

    def __init__(self, _capi):
        self._capi, self.ctx, self.cases = _capi, {}, []
        for dim in (2, 3):
            for form in FORMS:
                self._context_form(dim, *form)
            for form in FREE_FORMS:
                self._free_form(dim, *form)

    def context(self, dim, kind, n_veh=N, deg=DEG):
        key = (dim, kind, n_veh, deg)
        if key not in self.ctx:
            self.ctx[key] = make_context(self._capi, dim, kind, n_veh, deg)
        return self.ctx[key]

    def close(self):
        for c in self.ctx.values():
            c.close()
        self.ctx = {}

    def add(self, name, dim, case, thunk):
        self.cases.append(("%s|d=%d|%s" % (name, dim, case), thunk))

    def _context_form(self, dim, fam, jac, dev):
        _, eu, mv, pr = FAMILIES[fam]
        name = entry(fam, jac, dev)
        home = "motion" if mv else "plain"              # the context on which the form's plain call is valid
        Y = rows(dim)

        def case(label, kind=home, Yc=Y, n_veh=N, deg=DEG, **kw):
            self.add(name, dim, label, lambda: call(self.context(dim, kind, n_veh, deg), fam, jac, dev, Yc, **kw)[0])
        case("valid")
        case("null context", handle=False)
        for ptr in mandatory(fam, jac):
            case("null " + ptr, null=(ptr,))
        case("every optional output null", want=())
        case("B=-1", B=-1)
        case("B=0", B=0)
        case("B=0 and null Y", B=0, null=("Y",))
        case("max_nodes=0", max_nodes=0)
        case("eps_rel=nan", eps_rel=float("nan"))
        case("eps_rel=-1", eps_rel=-1.0)
        case("margin=nan", margin=float("nan"))
        case("no tables", kind="empty")
        case("no tables and null Y", kind="empty", null=("Y",))
        if mv:
            case("no motion", kind="plain")
        if eu and not pr:
            case("a motion under the Euclidean call", kind="motion")
            case("a motion under the Euclidean call and null Y", kind="motion", null=("Y",))
        case("degree 32", deg=32, Yc=np.zeros((B, N * dim, 33)))
        case("degree 32 and null Y", deg=32, Yc=np.zeros((B, N * dim, 33)), null=("Y",))
        if dim == 2:                                    # (a context whose d is 1 takes no tables: listed once)
            self.add(name, 1, "d=1", lambda: call(self.context(1, "empty"), fam, jac, dev, np.zeros((B, N, DEG + 1)))[0])
        if dim == 3:
            case("more than 128 features", kind="pyramid")
            case("more than 128 features and null Y", kind="pyramid", null=("Y",))
            if jac:
                case("more than 128 features and null jac", kind="pyramid", null=("jac",))
        if pr:
            one = np.zeros((B, dim, DEG + 1))
            case("one vehicle", kind="plain", n_veh=1, Yc=one)
            case("one vehicle and null Y", kind="plain", n_veh=1, Yc=one, null=("Y",))
            case("one vehicle and null val", kind="plain", n_veh=1, Yc=one, null=("val",))

    def _free_form(self, dim, fam, dev):
        name = entry(fam, dev=dev)
        moving = FREE[fam][1]

        def case(label, **kw):
            self.add(name, dim, label, lambda: call_free(self.context(dim, "plain"), fam, dev, dim, **kw)[0])
        case("valid")
        case("every optional output null", want=())
        case("null context", handle=False)
        case("null cv", null=("cv",))
        case("null val", null=("val",))
        case("null H", null=("H",))
        case("M=0", M=0)
        case("M=0 with nulls", M=0, null=("cv", "val"))
        case("M=-1", M=-1)
        case("dim=4", dim=4)
        case("K=1", K=1)
        case("K=33", K=33)
        case("K=33 and null cv", K=33, null=("cv",))
        case("F=0", F=0)
        case("F=17", F=17)
        case("max_nodes=0", max_nodes=0)
        case("eps_rel=nan", eps_rel=float("nan"))
        case("eps_rel=-1", eps_rel=-1.0)
        if moving:
            case("null r", null=("r",))
            case("Km=0", Km=0)
            case("Km>K", Km=DEG + 2)
            case("null Q", null=("Q",))
            case("M=0 and Km>K", M=0, Km=DEG + 2)
            case("M=0 and Km=0", M=0, Km=0)
            case("M=0 and null Q", M=0, null=("Q",))
            case("null cv and Km>K", null=("cv",), Km=DEG + 2)
