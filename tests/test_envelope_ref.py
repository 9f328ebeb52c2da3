"""CPU side of the envelope Jacobian (obtg_temporal_sep_true_min_jac): the exact-rational yardstick of envelope_ref.py held
to the oracle -- which pins KAPPA = d -- the tie / gap figures the GPU comparison with the finite-difference provider
rests on, and the ABI bookkeeping.  No GPU."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envelope_ref as E  # noqa: E402
import extrema_ref as R  # noqa: E402
from util import assert_close  # noqa: E402

# the three-vehicle problem of test_gpu_extrema.test_true_min_rows_in_bezoptimization at generateGuess(std=0.6, seed=4)
FD_PROBLEM = dict(numVeh=3, dimension=2, degree=5, maxSep=0.8, initPoints=[(0, 0), (1, 5), (9, 2)],
                  finalPoints=[(10, 1), (8, 8), (0, 7)], tf=1.0, separationRows='true_min')
FD_SEED = 4
TIE_SHIFT = 1e-3            # an entry whose yardstick minimiser moves by more than this between x and x + h e_k is a tie
MAX_LEFT_OUT = 0.05
MEASURED_GAP = 3.3e-9       # largest |envelope - central difference of certified minima| on this x (test below: 3.22e-9)


def _row(n_obj, dim, deg, seed):
    """control points on a 2^-12 grid in (-8, 8): y +- 0.5 is exact"""
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(-8.0, 8.0, (n_obj * dim, deg + 1)) * 4096.0) / 4096.0


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("deg", [3, 5, 7, 10])
def test_yardstick_against_the_oracle(deg, dim):
    """KAPPA * B_i^n(t) * Delta_c(t) equals sum_k B_k^2n(t) d c_k / d y of the oracle's R = 0 coefficients: vehicle pairs and
    a vehicle against a point obstacle, t at both ends and inside."""
    n_veh, n_obs = 2, 1
    y = _row(n_veh, dim, deg, seed=100 * deg + dim)
    obs = _row(n_obs, dim, 0, seed=7 + deg)[:, 0].reshape(n_obs, dim)
    full = E.full_row(y, obs)
    worst = 0.0
    for (a, b) in ((0, 1), (0, 2), (1, 2)):
        for t in (0.0, 1.0, 0.3125, 0.7):
            ref = E.oracle_block(full, n_veh + n_obs, dim, a, b, t)
            got = np.array([[float(v) for v in r] for r in E.envelope_block(full, dim, n_veh, a, b, t)])
            worst = max(worst, assert_close(got, ref, what="deg %d dim %d pair (%d, %d) t %g" % (deg, dim, a, b, t)))
            if t in (0.0, 1.0):
                keep = 0 if t == 0.0 else deg
                assert (np.delete(got, keep, axis=1) == 0.0).all() and (got[:, keep] != 0.0).any()
    print("deg %d dim %d: largest scaled |yardstick - oracle| = %.3e" % (deg, dim, worst))
    # KAPPA is pinned: d / 2 or 2 d would miss by a factor of two
    assert E.kappa(dim) == dim
    # obstacle against obstacle: no variable
    z = E.envelope_block(E.full_row(y, np.vstack([obs, obs + 1.0])), dim, n_veh, 2, 3, 0.5)
    assert all(v == 0 for r in z for v in r)


def test_basis_is_a_partition_of_unity():
    for n in (1, 5, 20):
        for t in (Fraction(0), Fraction(1), Fraction(3, 16), Fraction(float(0.7))):
            w = E.basis(n, t)
            assert sum(w) == 1 and all(v >= 0 for v in w)


def _fd_problem():
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    bo = BezOptimization(**FD_PROBLEM)
    return bo, bo.generateGuess(std=0.6, seed=FD_SEED)


def certified(bo, x, rel=R.REL):
    co = R.separation_coeffs(bo.reshapeVector(x), 3, 2, FD_PROBLEM['maxSep'])
    return [R.certified_min(co[p], rel) for p in range(co.shape[0])]


def ties(bo, x, h):
    """[P][n_x] bool: the yardstick minimiser of the pair moves by more than TIE_SHIFT between x and x + h e_k"""
    t0 = np.array([float(r["t"]) for r in certified(bo, x)])
    out = np.zeros((t0.size, x.size), bool)
    for k in range(x.size):
        xk = x.copy()
        xk[k] += h
        out[:, k] = np.abs(np.array([float(r["t"]) for r in certified(bo, xk)]) - t0) > TIE_SHIFT
    return out


def test_fd_comparison_point_is_smooth_and_its_gap():
    """The x of the GPU comparison with the finite-difference provider: at most 5 % of the entries are ties, and the largest
    gap between the yardstick's envelope entries (at its own minimiser, bracket 1e-20 s) and central differences (step 2^-17)
    of its certified minima is MEASURED_GAP -- the figure the GPU bound is four times of."""
    from optimalbeziertrajectorygeneration_amd import optimization as opt
    bo, x = _fd_problem()
    out = ties(bo, x, opt.FD_STEP)
    print("ties: %d of %d entries" % (out.sum(), out.size))
    assert out.mean() <= MAX_LEFT_OUT
    rel = Fraction(1, 10 ** 20)
    y0 = certified(bo, x, rel)
    blk = E.envelope_blocks(bo.reshapeVector(x), 2, 3, 3, [float(r["t"]) for r in y0])
    J = E.scatter(blk, 3, 3, 2, 1, 4)
    assert J.shape == (3, x.size)
    hc = 2.0 ** -17
    Cd = np.zeros(J.shape)
    for k in range(x.size):
        xp, xm = x.copy(), x.copy()
        xp[k] += hc
        xm[k] -= hc
        gp, gm = certified(bo, xp, rel), certified(bo, xm, rel)
        Cd[:, k] = [float(gp[p]["H"] - gm[p]["H"]) / (xp[k] - xm[k]) for p in range(3)]
    gap = float(np.abs(J - Cd)[~out].max())
    print("largest |envelope - central difference| = %.3e (entries up to %.3f)" % (gap, np.abs(J).max()))
    assert gap <= MEASURED_GAP


def test_library_exports_the_envelope_jacobian():
    """The two names are in the header, the library, obtg_abi_symbols and the binding table; ABI revision 7, K_COUNT 9."""
    import ctypes as C
    from optimalbeziertrajectorygeneration_amd import _capi, build
    lib = C.CDLL(build.build())
    lib.obtg_abi_symbols.restype = C.POINTER(C.c_char)
    p, syms, i = lib.obtg_abi_symbols(), [], 0
    while True:
        s = b""
        while p[i] != b"\0":
            s += p[i]
            i += 1
        i += 1
        if not s:
            break
        syms.append(s.decode())
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "obtg.h")).read()
    for name in ("obtg_temporal_sep_true_min_jac", "obtg_temporal_sep_true_min_jac_dev"):
        assert hasattr(lib, name), name
        assert name in syms, name
        assert name in _capi.abi_symbol_names(), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "Later, still 7: new: the envelope Jacobian" in header
    lib.obtg_abi_version.restype = C.c_int
    assert lib.obtg_abi_version() == 7
    assert _capi.K_COUNT == 9
    from optimalbeziertrajectorygeneration_amd.optimization import BezOptimization
    assert callable(BezOptimization.trueMinSeparationJacobian)
