"""tests/keep_out_euclid_ref.py against itself, against an SLSQP projection and against the library's host geometry
(obtg_keep_out_features): no device.  DESIGN.md 4.26."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_out_euclid_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dim_of(name):
    return ref.OBSTACLES[name]().shape[1] - 1


def probe_points(name, seed, k=12):
    """points inside, near the faces and well outside, round the obstacle"""
    rng = np.random.default_rng(seed)
    d = dim_of(name)
    v = rng.normal(size=(k, d))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * rng.uniform(0.2, 3.5, size=(k, 1))


def slsqp_distance(Hn, p):
    from scipy.optimize import minimize
    A, b = Hn[:, :-1], Hn[:, -1]
    x0 = np.zeros(len(p)) if (b > 0).all() else p - A[0] * (A[0] @ p - b[0])
    r = minimize(lambda x: 0.5 * ((x - p) ** 2).sum(), x0, jac=lambda x: x - p, method="SLSQP",
                 constraints=[dict(type="ineq", fun=lambda x: b - A @ x, jac=lambda x: -A)], options=dict(ftol=1e-16, maxiter=500))
    return float(np.linalg.norm(r.x - p)), r


@pytest.mark.parametrize("name", sorted(ref.OBSTACLES))
def test_distance_against_all_subsets_and_projection(name):
    """D over the features equals D over ALL subsets of up to d faces (difference 0), and outside it is the distance to the
    SLSQP projection within 1e-12 (measured 2.8e-14 when the issue was written)."""
    Hn = ref.normalise(ref.OBSTACLES[name]())
    sets = [S for S, _ in ref.features(Hn)]
    worst = 0.0
    for p in probe_points(name, 11):
        a, b = ref.D_exact(Hn, p, sets), ref.D_exact_subsets(Hn, p)
        assert a["D"] == b["D"], (name, p, a["D"], b["D"])
        if not a["inside"]:
            dist, r = slsqp_distance(Hn, p)
            assert r.success or r.status == 8, r.message       # (8: the line search cannot improve a converged point)
            assert (Hn[:, :-1] @ r.x - Hn[:, -1]).max() <= 1e-12
            worst = max(worst, abs(dist - a["D"]))
            assert abs(np.linalg.norm(a["dir"]) - 1.0) <= 4 * 2.0 ** -52
    print("%s: largest |D - projection| %.3g" % (name, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("name,want", sorted(ref.FEATURE_COUNTS.items()))
def test_feature_counts(name, want):
    assert len(ref.features(ref.normalise(ref.OBSTACLES[name]()))) == want


@pytest.mark.parametrize("name", sorted(ref.OBSTACLES))
def test_library_features_against_the_yardstick(name):
    """obtg_keep_out_features: the same sets in the same order, Hn within 2 ulp, Gram^-1 within 16 c 2^-53 of the exact
    inverse of the library's own Hn, relative to its largest entry (c: the yardstick's conditioning figure)."""
    from optimalbeziertrajectorygeneration_amd import _capi
    H = ref.OBSTACLES[name]()
    got = _capi.keep_out_features(H)
    assert got["rc"] == 0
    Hn = ref.normalise(H)
    assert (np.abs(got["Hn"] - Hn) <= 2 * np.spacing(np.abs(Hn))).all()
    unit = np.array([sum(ref.fr(x) ** 2 for x in h[:-1]) == 1 for h in H])            # |a| = 1 exactly
    assert (got["Hn"][unit].view(np.int64) == H[unit].view(np.int64)).all()          # |a| = 1: bit for bit
    feats = ref.features(got["Hn"])
    assert [tuple(int(x) for x in r if x >= 0) for r in got["idx"]] == [tuple(S) for S, _ in feats]
    c = ref.conditioning(feats)
    for k, (S, _) in enumerate(feats):
        Gi = ref.gram_inverse_exact(got["Hn"], S)
        m = len(S)
        exact = [Gi[i][j] for i in range(m) for j in range(i, m)]
        mine = got["ginv"][k][:len(exact)]
        big = max(abs(float(x)) for x in exact)
        assert max(abs(float(ref.fr(a) - e)) for a, e in zip(mine, exact)) <= 16 * c * 2.0 ** -53 * big, (name, S)
        assert (got["ginv"][k][len(exact):] == 0).all()


def test_library_features_refusals():
    from optimalbeziertrajectorygeneration_amd import _capi
    from optimalbeziertrajectorygeneration_amd._capi import load
    assert _capi.keep_out_features(np.ones((17, 3)))["rc"] == _capi.ERR_UNSUPPORTED          # 17 faces
    assert _capi.keep_out_features(np.ones((2, 5)))["rc"] == -1                             # d = 4: OBTG_ERR_ARG
    n = C.c_int(0)
    assert load().obtg_keep_out_features(None, 1, 2, None, None, None, C.byref(n)) == -1
    # |a| = 0 and a non-finite entry: NaN faces, no feature
    H = ref.square()
    H[1, :2] = 0.0
    got = _capi.keep_out_features(H)
    assert got["rc"] == 0 and np.isnan(got["Hn"][1, :2]).all() and not np.isfinite(got["Hn"][1]).any() and np.isfinite(got["Hn"][[0, 2, 3]]).all()
    # a many-sided pyramid's apex: more than 128 features
    k = 15
    th = 2 * math.pi * np.arange(k) / k
    A = np.column_stack((np.cos(th), np.sin(th), np.full(k, 0.5)))
    H = np.vstack((np.column_stack((A, np.ones(k))), [[0.0, 0.0, -1.0, 1.0]]))
    got = _capi.keep_out_features(H)
    assert got["n"] > 128 and got["rc"] == _capi.ERR_UNSUPPORTED
    assert len(ref.features(ref.normalise(H))) == got["n"]


@pytest.mark.parametrize("name", ref.CORNERED)
def test_search_against_dense_sampling(name):
    Hn = ref.normalise(ref.OBSTACLES[name]())
    feats = ref.features(Hn)
    for P in ref.curves(5, dim_of(name), 5, M=4):
        r = ref.search(P, Hn, feats)
        t, D = ref.D_samples(P, Hn, feats, 4001)
        assert r["ok"] and r["val"] - r["bound"] <= r["tol"]
        assert r["bound"] <= D.min() + 1e-12 and r["val"] <= D.min() + 1e-12
        # D is 1-Lipschitz in the point and |c'| <= n max |P_(i+1) - P_i|: the grid's minimum sits within half a step of that
        lip = (P.shape[1] - 1) * np.linalg.norm(np.diff(P, axis=1), axis=0).max()
        assert D.min() - r["val"] <= lip * 0.5 / 4000


def campaign_batch(name, deg, seed):
    """(Hn, feats, curves[30], Euclidean rows, faces rows) for one (obstacle, degree) batch of the GPU campaign"""
    Hn = ref.normalise(ref.OBSTACLES[name]())
    feats = ref.features(Hn)
    cv = ref.curves(deg, dim_of(name), seed)
    eu = [ref.search(P, Hn, feats) for P in cv]
    fa = [ref.faces_search(P, Hn) for P in cv]
    return Hn, feats, cv, eu, fa


def test_campaign_conditions():
    """What the GPU campaign (tests/test_gpu_keep_out_euclid.py CAMPAIGN) must hold, confirmed on the yardstick first: no item
    meets a cap; each (obstacle with a corner, degree >= 3) batch holds at least 5 rows where Euclid exceeds faces by 1e-6;
    at least 3 rows <= 0 over the whole campaign; fewer than 1 item in 10 closer than 1e-6 s (where a direction is compared
    on value only); Euclid is never below faces."""
    from test_gpu_keep_out_euclid import CAMPAIGN
    non_positive = close = total = 0
    most_nodes = 0
    for name, deg, seed in CAMPAIGN:
        _, _, _, eu, fa = campaign_batch(name, deg, seed)
        assert all(r["ok"] for r in eu), (name, deg)
        most_nodes = max(most_nodes, max(r["nodes"] for r in eu))
        above = sum(1 for e, f in zip(eu, fa) if e["val"] > f["val"] + 1e-6)
        assert all(e["val"] >= f["val"] - f["tol"] for e, f in zip(eu, fa))
        if name in ref.CORNERED and deg >= 3:
            assert above >= 5, (name, deg, above)
        non_positive += sum(1 for e in eu if e["val"] <= 0.0)
        close += sum(1 for e in eu if abs(e["val"]) < 1e-6 * e["s"])
        total += len(eu)
    print("campaign: %d items, %d rows <= 0, %d close, most nodes %d" % (total, non_positive, close, most_nodes))
    assert non_positive >= 3 and 10 * close < total


@pytest.mark.parametrize("name", ref.CORNERED)
def test_block_against_forward_differences(name):
    """The block dir[c] B_i(t*) against forward differences of the searched row: h = 1e-6, eps_rel = 1e-12, acceptance 1e-4
    (4.24's figures)."""
    Hn = ref.normalise(ref.OBSTACLES[name]())
    feats = ref.features(Hn)
    sets = [S for S, _ in feats]
    worst = 0.0
    for P in ref.curves(3, dim_of(name), 21, M=4):
        r = ref.search(P, Hn, feats)
        if r["t"] in (0.0, 1.0) or abs(r["val"]) < 1e-3:
            continue                                           # (an end minimiser, or a row at the boundary's own kink)
        fd = ref.forward_difference(P, Hn, feats)
        gap = float(np.abs(ref.block(P, Hn, r["t"], r["tol"], sets) - fd).max())
        worst = max(worst, gap)
    print("%s: largest |block - forward difference| %.3g" % (name, worst))
    assert worst <= 1e-4


def test_host_geometry_stand_alone_under_sanitizers(tmp_path):
    """csrc/keepout_features.h with a main of its own (tests/native/keepout_features_host.cpp), built by g++ alone under the
    address and undefined-behaviour sanitizers and run as a program on every obstacle and on the many-sided pyramid (more
    features than the table's room): no report, and the yardstick's sets."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "the host compiler is part of the build"
    exe = str(tmp_path / "keepout_features_host")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(REPO, "tests", "native", "keepout_features_host.cpp"), "-o", exe])
    k = 15
    th = 2 * math.pi * np.arange(k) / k
    pyramid = np.vstack((np.column_stack((np.cos(th), np.sin(th), np.full(k, 0.5), np.ones(k))), [[0.0, 0.0, -1.0, 1.0]]))
    cases = [ref.OBSTACLES[name]() for name in sorted(ref.OBSTACLES)] + [pyramid]
    text = "".join("%d %d\n" % (len(H), H.shape[1] - 1) + "".join(" ".join("%.17g" % v for v in h) + "\n" for h in H) for H in cases)
    run = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    lines = iter(run.stdout.split("\n"))
    for H in cases:
        n = int(next(lines))
        rows = [tuple(int(v) for v in next(lines).split() if int(v) >= 0) for _ in range(min(n, 128))]
        want = [tuple(S) for S, _ in ref.features(ref.normalise(H))]
        assert n == len(want) and rows == want[:128]
