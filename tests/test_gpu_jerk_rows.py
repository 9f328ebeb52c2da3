"""The jerk-bound rows on the device (obtg_jerk[_dev], Context.jerk) against the exact-rational yardstick of
tests/jerk_rows_ref.py: every element inside K * 2^-53 * M, in every launch form the rows take -- the specialised body in
MODE 3 at R = 0 and elevated, the any-degree kernel -- and inside a finite-difference view."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jerk_rows_ref as AR  # noqa: E402
import constraint_rows_ref as C  # noqa: E402
from util import RTOL, assert_close  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    assert _capi.device_count() > 0, "these tests need the GPU"
    return _capi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("case", AR.JERK_CASES, ids=[c[0] for c in AR.JERK_CASES])
def test_jerk_rows(capi, case):
    """B = 3 rows, tf per row; the form a case names is the one the speed rows of the same shape take (constraint_rows_ref.speed_form)"""
    name, N, d, n, R, kind, form = case
    assert ("generic" in form) == (C.speed_form(d, n, R) == "generic") and ("ELEV" in form) == (C.speed_form(d, n, R) == "fast elevated")
    tf = np.array(AR.JERK_TF)
    B = tf.size
    Yb = C.rows_batch(900 + n + R, B, N, d, n, kind)
    ctx = capi.Context(N, d, n, R)
    try:
        got = ctx.jerk(Yb, tf, AR.JERK_BOUND).reshape(B, N, -1)
    finally:
        ctx.close()
    worst = 0.0
    for b in range(B):
        worst = max(worst, AR.assert_within(got[b], AR.jerk(Yb[b], N, d, R, tf[b], AR.JERK_BOUND), "%s row %d tf %r" % (name, b, tf[b])))
    print("\njerk, %s (%s): largest share of the bound used by the device %.3f" % (name, form, worst))
    if n == 1:
        assert np.array_equal(_bits(got), _bits(np.full(got.shape, AR.JERK_BOUND ** 2))), "degree 1: every row is bound**2"


def test_reference_fixture(capi, golden_dir):
    """What the reference's diff().diff().diff().normSquare().elev(R) returned (tests/golden/jerk_rows.npz) against bound**2 - rows,
    scale-aware within RTOL; degrees 3, 5, 10 on the specialised kernels, 4 and 6 on the any-degree one"""
    worst = 0.0
    ctxs = {}
    try:
        for name, Y, dim, deg, R, tf, c in AR.fixture_rows(golden_dir):
            N = Y.shape[0] // dim
            ctx = ctxs.get((dim, deg, R))
            if ctx is None:
                ctx = ctxs[(dim, deg, R)] = capi.Context(N, dim, deg, R)
            got = ctx.jerk(Y, tf, 0.0).reshape(N, -1)
            worst = max(worst, assert_close(-got, c, what=name))
    finally:
        for ctx in ctxs.values():
            ctx.close()
    print("reference fixture: largest scaled |device - reference| = %.3e" % worst)


@pytest.mark.parametrize("deg", [5, 6], ids=["fused deg 5", "generic deg 6"])
def test_rows_inside_a_finite_difference_view(capi, deg):
    """Between obtg_fd_view_begin and _end with dY = NULL the rows are the bits of the call on the batch obtg_fd_batch_dev
    writes: B = n_x + 1 rows of N = 3 vehicles -- formed while staging by the specialised kernel, from the batch the library
    writes once for the any-degree one."""
    import torch
    N, dim, fixed, h = 3, 2, 1, 1.4901161193847656e-08
    nc = deg + 1
    B = N * dim * (nc - 2 * fixed) + 1
    assert bool(capi.fast_kernels(dim, deg) & 1) == (deg == 5)
    Y0 = C.swarm(77, N, dim, deg)
    tf = np.linspace(0.8, 2.9, B)
    ctx = capi.Context(N, dim, deg, 0)
    try:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        d0, dtf = torch.from_numpy(Y0).cuda(), torch.from_numpy(tf).cuda()
        dY = torch.empty((B,) + Y0.shape, dtype=torch.float64, device="cuda")
        ctx.fd_batch_dev(d0.data_ptr(), fixed, h, B, dY.data_ptr())
        L = ctx.len_speed
        a = torch.full((B, L), float("nan"), dtype=torch.float64, device="cuda")
        v = torch.full((B, L), float("nan"), dtype=torch.float64, device="cuda")
        ctx.jerk_dev(dY.data_ptr(), dtf.data_ptr(), B, AR.JERK_BOUND, a.data_ptr())
        ctx.fd_view_begin(d0.data_ptr(), fixed, h, B)
        try:
            ctx.jerk_dev(None, dtf.data_ptr(), B, AR.JERK_BOUND, v.data_ptr())
        finally:
            ctx.fd_view_end()
        torch.cuda.synchronize()
        ctx.use_own_stream()
        a, v, Yb = a.cpu().numpy(), v.cpu().numpy(), dY.cpu().numpy()
        host = ctx.jerk(Yb, tf, AR.JERK_BOUND)
    finally:
        ctx.close()
    assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(v)) and np.array_equal(_bits(a), _bits(host))
    assert int((a[1:] != a[:1]).any(axis=1).sum()) == B - 1, "every row differs from row 0"
    for b in (0, 1, B - 1):
        AR.assert_within(a[b].reshape(N, -1), AR.jerk(Yb[b], N, dim, 0, tf[b], AR.JERK_BOUND), "view row %d" % b)
