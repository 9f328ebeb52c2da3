"""The inputs of the collision checks' "every kernel form" tests, built once for the CPU test
(tests/test_collcheck_cases_ref.py: the restatement alone, and what the cases must reach for the GPU test to mean something)
and the GPU test (tests/test_gpu_collcheck_forms.py: the device against the restatement).  Seeded and deterministic; needs
numpy and tests/collcheck_ref.py only.

A BASE per control-point count K: 16 planar random walks (`default_rng(7000 + K)`, spread 5.0), all 120 pairs, and eight
polygons of 1, 2, 3, 16, 1, 2, 7 and 16 vertices drawn after them (polygon 0's single vertex is curve 0's first control point),
every curve against every polygon, 128 pairs.  A base is PLACED in space in four ways:

    planar       as drawn, z = +0: the host picks the planar kernels
    minus_zero   z = -0.0: the host picks the 3-D machine; the results are `planar`'s bit for bit
    plane_z1     z = 1.0
    plane_yz     x = 0.5, the base's x in y and its y in z: the 3-D machine walked deep with a z that varies

and the polygons once more at z = 1 against planar curves ("mixed": every pair is apart at the root).  The restatement's
results per (K, placing) are computed once per process and shared (`ref_curve_group`, `ref_poly_group`).
"""
import functools

import numpy as np

import collcheck_ref as R

KS = (2, 3, 4, 5, 7, 10, 11, 12, 13, 14, 15, 16)      # 4, 11, 16: builds of their own; 12 .. 15: the any-count build's two-pass split; 10: its last one-pass count
PLACINGS = ("planar", "minus_zero", "plane_z1", "plane_yz")
POLY_PLACINGS = PLACINGS + ("mixed",)
POLY_SIZES = (1, 2, 3, 16, 1, 2, 7, 16)
N_CURVES = 16
MAX_NODES = 600
PARAM_K = 6


def walks(rng, n, K, dim, spread):
    """n curves [3][K]: a random walk of K control points from a random start in [0, spread]^dim; the other rows +0"""
    c = np.zeros((n, 3, K))
    c[:, :dim] = rng.uniform(0.0, spread, size=(n, dim, 1)) + np.cumsum(rng.normal(0.0, 4.0 / np.sqrt(K), size=(n, dim, K)), axis=2)
    return c


def pack(polys):
    return np.vstack(polys), np.concatenate(([0], np.cumsum([len(p) for p in polys]))).astype(np.int32)


@functools.lru_cache(maxsize=None)
def base(K):
    """-> (curves[16][3][K], polygons: list of [k][3]), planar, z = +0"""
    rng = np.random.default_rng(7000 + K)
    curves = walks(rng, N_CURVES, K, 2, 5.0)
    polys = []
    for k in POLY_SIZES:
        p = np.zeros((k, 3))
        p[:, :2] = rng.uniform(0.0, 5.0, size=(1, 2)) + rng.normal(0.0, 1.5, size=(k, 2))
        polys.append(p)
    polys[0][0] = curves[0, :, 0]
    curves.setflags(write=False)
    return curves, polys


def place(xyz, placing, axis):
    """xyz: planar data whose coordinate index is `axis` (curves [n][3][K]: 1; points [n][3]: 1)"""
    a = np.moveaxis(np.array(xyz, dtype=np.float64), axis, 0)
    out = np.empty_like(a)
    if placing == "planar":
        out[:] = a
    elif placing == "minus_zero":
        out[:2], out[2] = a[:2], -0.0
    elif placing == "plane_z1":
        out[:2], out[2] = a[:2], 1.0
    elif placing == "plane_yz":
        out[0], out[1], out[2] = 0.5, a[0], a[1]
    elif placing == "shear_zx":
        out[:2], out[2] = a[:2], a[0]
    else:
        raise ValueError(placing)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def all_pairs():
    pa, pb = np.triu_indices(N_CURVES, 1)
    return pa.astype(np.int32), pb.astype(np.int32)


def curve_group(K, placing):
    """-> dict(curves, pa, pb): the 120 pairs of the base of K, placed"""
    pa, pb = all_pairs()
    return dict(curves=place(base(K)[0], placing, 1), pa=pa, pb=pb)


def poly_group(K, placing):
    """-> dict(curves, pts, off, pc, pp): every curve of the base of K against its eight polygons, 128 pairs.  `mixed`: planar
    curves, the polygons at z = 1."""
    curves, polys = base(K)
    pts, off = pack(polys)
    pc, pp = np.repeat(np.arange(N_CURVES), len(polys)).astype(np.int32), np.tile(np.arange(len(polys)), N_CURVES).astype(np.int32)
    if placing == "mixed":
        return dict(curves=place(curves, "planar", 1), pts=place(pts, "plane_z1", 1), off=off, pc=pc, pp=pp)
    return dict(curves=place(curves, placing, 1), pts=place(pts, placing, 1), off=off, pc=pc, pp=pp)


def run_curves(fn, g, **kw):
    kw.setdefault("max_nodes", MAX_NODES)
    return fn(g["curves"], g["pa"], g["pb"], **kw)


def run_polys(fn, g, **kw):
    kw.setdefault("max_nodes", MAX_NODES)
    return fn(g["curves"], g["pts"], g["off"], g["pc"], g["pp"], **kw)


def _frozen(r):
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def ref_curve_group(K, placing):
    return _frozen(run_curves(R.coll_check_pairs, curve_group(K, placing)))


@functools.lru_cache(maxsize=None)
def ref_poly_group(K, placing):
    return _frozen(run_polys(R.coll_check2poly_pairs, poly_group(K, placing)))


# ------------------------------------------------------------------------------------------------ parameters
CURVE_PARAMS = [dict(eps=e) for e in (0.0, 0.5, 1.0, 2.0)] + [dict(max_iter=m) for m in (1, 3, 6)] + [dict(md_cap=m) for m in (1, 4, 16)]
POLY_PARAMS = [dict(max_iter=m) for m in (1, 3)] + [dict(md_cap=m) for m in (1, 4)]


@functools.lru_cache(maxsize=None)
def ref_curve_params(i):
    """the planar base of K = 6 under CURVE_PARAMS[i] (i = -1: the defaults)"""
    return _frozen(run_curves(R.coll_check_pairs, curve_group(PARAM_K, "planar"), **(CURVE_PARAMS[i] if i >= 0 else {})))


@functools.lru_cache(maxsize=None)
def ref_poly_params(i):
    return _frozen(run_polys(R.coll_check2poly_pairs, poly_group(PARAM_K, "planar"), **(POLY_PARAMS[i] if i >= 0 else {})))


# ------------------------------------------------------------------------------------------------ the node budget's edge
@functools.lru_cache(maxsize=None)
def budget_curve_case():
    """The pair of the planar K = 6 base that ends MD_OK after the most nodes -> dict(curves[2][3][6], pa, pb, N, depth)"""
    g, ref = curve_group(PARAM_K, "planar"), ref_curve_params(-1)
    ok = np.flatnonzero(ref["status"] == R.MD_OK)
    i = int(ok[np.argmax(ref["nodes"][ok])])
    return dict(curves=g["curves"][[g["pa"][i], g["pb"][i]]], pa=np.array([0], np.int32), pb=np.array([1], np.int32),
                N=int(ref["nodes"][i]), depth=int(ref["depth"][i]), res=float(ref["res"][i]))


@functools.lru_cache(maxsize=None)
def budget_poly_case():
    """Curve 0 of the planar K = 6 base against the triangle of its own first three control points: one walk down the
    left halves to cnt = 100"""
    c = curve_group(PARAM_K, "planar")["curves"][:1]
    tri = np.ascontiguousarray(c[0, :, :3].T)
    r = R.coll_check2poly(c[0], tri, max_nodes=MAX_NODES)
    return dict(curves=c, pts=tri, off=np.array([0, 3], np.int32), pc=np.array([0], np.int32), pp=np.array([0], np.int32),
                N=int(r["nodes"]), depth=int(r["depth"]), res=float(r["res"]), status=int(r["status"]))


def budgets(N):
    return (N + 1, N, N - 1, 1)


# ------------------------------------------------------------------------------------------------ non-finite input
NF_VALUES = (np.nan, np.inf, -np.inf)
NF_POINTS = (0, 3, 5)
NF_PAIRS = (np.array([0, 1, 1, 2, 1], np.int32), np.array([1, 0, 2, 3, 1], np.int32))
NF_UNTOUCHED = 3                       # (2, 3)


@functools.lru_cache(maxsize=None)
def _nf_base():
    rng = np.random.default_rng(5)
    curves = walks(rng, 8, 6, 2, 3.0)
    tri = np.zeros((3, 3))
    tri[:, :2] = rng.uniform(0.0, 3.0, size=(1, 2)) + rng.normal(0.0, 1.5, size=(3, 2))
    return curves, tri


def nonfinite_curve_cases():
    """27 plantings into curve 1 -> (name, curves[8][3][6]); the pairs are NF_PAIRS.  A planting in row z makes the call 3-D."""
    out = []
    for vn, v in zip(("nan", "pinf", "ninf"), NF_VALUES):
        for j in NF_POINTS:
            for row in range(3):
                c = _nf_base()[0].copy()
                c[1, row, j] = v
                out.append(("%s_p%d_%s" % (vn, j, "xyz"[row]), c))
    return out


def nonfinite_poly_cases():
    """-> (name, curves[1][3][6], triangle[3][3]): each planted curve against a clean triangle, then the clean curve 1 against
    the triangle with vertex 1 planted, 27 + 9 cases of one pair"""
    curves, tri = _nf_base()
    out = [(name, c[1:2], tri.copy()) for name, c in nonfinite_curve_cases()]
    for vn, v in zip(("nan", "pinf", "ninf"), NF_VALUES):
        for row in range(3):
            t = tri.copy()
            t[1, row] = v
            out.append(("tri_%s_%s" % (vn, "xyz"[row]), curves[1:2].copy(), t))
    return out


NF_TRI = dict(off=np.array([0, 3], np.int32), pc=np.array([0], np.int32), pp=np.array([0], np.int32))


@functools.lru_cache(maxsize=None)
def ref_nonfinite_curves():
    return [_frozen(R.coll_check_pairs(c, *NF_PAIRS, max_nodes=MAX_NODES)) for _, c in nonfinite_curve_cases()]


@functools.lru_cache(maxsize=None)
def ref_nonfinite_polys():
    return [_frozen(R.coll_check2poly_pairs(c, t, NF_TRI["off"], NF_TRI["pc"], NF_TRI["pp"], max_nodes=MAX_NODES))
            for _, c, t in nonfinite_poly_cases()]


# ------------------------------------------------------------------------------------------------ one list of everything
N_LIST_EXTRA = 10


@functools.lru_cache(maxsize=None)
def list_case(K):
    """The four placings of the base of K in ONE call (64 curves; the -0, the 1 and the plane_yz z's make it 3-D for all of
    them): every group's 120 pairs, the first ten of each once more, the same ten as (b, a), and four pairs a == a per
    group, permuted.  -> dict(curves, pa, pb), ref: the restatement per pair (the groups' own results where they have one)."""
    pa0, pb0 = all_pairs()
    curves, pa, pb, ref = [], [], [], []
    for gi, placing in enumerate(PLACINGS):
        g, o = curve_group(K, placing), gi * N_CURVES
        curves.append(g["curves"])
        r = ref_curve_group(K, placing if placing != "minus_zero" else "planar")
        e = N_LIST_EXTRA
        xa = np.concatenate((pb0[:e], np.arange(4))).astype(np.int32)
        xb = np.concatenate((pa0[:e], np.arange(4))).astype(np.int32)
        rx = R.coll_check_pairs(g["curves"], xa, xb, max_nodes=MAX_NODES)
        pa += [pa0 + o, pa0[:e] + o, xa + o]
        pb += [pb0 + o, pb0[:e] + o, xb + o]
        ref.append({k: np.concatenate((r[k], r[k][:e], rx[k])) for k in r})
    pa, pb = np.concatenate(pa).astype(np.int32), np.concatenate(pb).astype(np.int32)
    perm = np.random.default_rng(9000 + K).permutation(len(pa))
    ref = {k: np.concatenate([r[k] for r in ref])[perm] for k in ref[0]}
    return dict(curves=np.ascontiguousarray(np.concatenate(curves)), pa=pa[perm], pb=pb[perm]), _frozen(ref)


# ------------------------------------------------------------------------------------------------ what the reference is asked
N_RECORDED = 24


def sheared_case():
    """Six crossing pairs of the planar K = 4 base (the first six the restatement does not answer 1 for) in the plane z = x"""
    ref = ref_curve_group(4, "planar")
    pa, pb = all_pairs()
    i = np.flatnonzero((ref["status"] == R.MD_OK) & (ref["res"] != 1))[:6]
    return dict(curves=place(base(4)[0], "shear_zx", 1), pa=pa[i], pb=pb[i])


def recorded_groups():
    """The cases tests/golden/gen_collcheck_forms.py runs the reference on -> (cc: [(name, curves, pa, pb, planar)],
    cp: [(name, curves, polys, pc, pp, planar)]); `planar`: the reference is handed 2-D curves."""
    cc, cp = [], []
    nf = nonfinite_curve_cases()
    for rows, planar, name in (("xy", True, "nf_xy"), ("z", False, "nf_z")):
        sel = [c for n, c in nf if n[-1] in rows]
        curves = np.concatenate(sel)                        # 8 curves per planting
        pa = np.concatenate([NF_PAIRS[0] + 8 * k for k in range(len(sel))])
        pb = np.concatenate([NF_PAIRS[1] + 8 * k for k in range(len(sel))])
        cc.append((name, curves, pa, pb, planar))
    for K, placing in ((13, "planar"), (4, "plane_yz"), (13, "plane_yz")):
        g = curve_group(K, placing)
        cc.append(("%s_K%d" % (placing, K), g["curves"], g["pa"][:N_RECORDED], g["pb"][:N_RECORDED], placing == "planar"))
    g = sheared_case()
    cc.append(("shear_zx_K4", g["curves"], g["pa"], g["pb"], False))
    np_cases = nonfinite_poly_cases()
    for rows, planar, name in (("xy", True, "nf_poly_xy"), ("z", False, "nf_poly_z")):
        sel = [(c, t) for n, c, t in np_cases if n[-1] in rows]
        cp.append((name, np.concatenate([c for c, _ in sel]), [t for _, t in sel], np.arange(len(sel)), np.arange(len(sel)), planar))
    return cc, cp
