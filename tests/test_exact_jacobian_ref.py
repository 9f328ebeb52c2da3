"""CPU checks of the exact-derivative feature: the rational yardstick (tests/exact_jacobian_ref.py) is held to the NumPy
restatement of the reference (oracle.numpy_port) -- values, and derivatives against central differences of the port --
and the built library exports the exact-derivative entry points of ABI 7.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_jacobian_ref as X  # noqa: E402

from oracle import numpy_port as NP  # noqa: E402

NEW_SYMBOLS = ("obtg_temporal_sep_jac", "obtg_temporal_sep_jac_dev", "obtg_speed_jac", "obtg_speed_jac_dev",
               "obtg_ang_rate_jac", "obtg_ang_rate_jac_dev", "obtg_euclidean_grad", "obtg_deriv_energy_grad")


def _Y(nveh, dim, deg, seed):
    rng = np.random.default_rng(seed)
    base = np.linspace(0.0, 6.0, deg + 1)
    Y = np.empty((nveh * dim, deg + 1))
    for r in range(nveh * dim):
        Y[r] = base * rng.uniform(0.5, 1.5) + rng.normal(0, 0.7, deg + 1) + r
    return Y


def _close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    scale = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= tol * scale, (np.abs(a - b).max(), scale)


def _central(f, Y, h):
    """[len f][rows][nc] central differences of f at Y"""
    out = []
    for r in range(Y.shape[0]):
        for i in range(Y.shape[1]):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[r, i] += h
            Ym[r, i] -= h
            out.append((np.asarray(f(Yp)) - np.asarray(f(Ym))) / (2 * h))
    return np.array(out).T.reshape(-1, Y.shape[0], Y.shape[1])


@pytest.mark.parametrize("dim,deg,R", [(2, 5, 0), (3, 5, 3), (2, 8, 10)])
def test_separation_yardstick_matches_the_port(dim, deg, R):
    Y = _Y(2, dim, deg, seed=deg + R)
    val = np.array([float(v) for v in X.temporal_sep(Y, 2, dim, R, 0.9)])
    _close(val, NP.temporal_sep(Y, 2, dim, R, 0.9), 1e-13)
    J = np.array(X.temporal_sep_jac(Y, 2, dim, R), dtype=float)[0]            # [L][dim][nc], the a side
    fd = _central(lambda Yq: NP.temporal_sep(Yq, 2, dim, R, 0.9), Y, 1e-3)     # [L][2 dim][nc]
    _close(J, fd[:, :dim, :], 1e-8)
    _close(-J, fd[:, dim:, :], 1e-8)


@pytest.mark.parametrize("is_max", [True, False])
def test_speed_yardstick_matches_the_port(is_max):
    dim, deg, R, tf = 2, 6, 4, 7.5
    Y = _Y(2, dim, deg, seed=3)
    val = np.array([float(v) for v in X.speed(Y, 2, dim, R, tf, 2.0, is_max)])
    _close(val, NP.speed(Y, 2, dim, R, tf, 2.0, is_max), 1e-13)
    J, Jt = X.speed_jac(Y, 2, dim, R, tf, is_max)
    J, Jt = np.array(J, dtype=float), np.array(Jt, dtype=float)
    fd = _central(lambda Yq: NP.speed(Yq, 2, dim, R, tf, 2.0, is_max), Y, 1e-3)
    L = J.shape[1]
    for v in range(2):
        _close(J[v], fd[v * L:(v + 1) * L, v * dim:(v + 1) * dim, :], 1e-8)
    h = 1e-5
    ft = (NP.speed(Y, 2, dim, R, tf + h, 2.0, is_max) - NP.speed(Y, 2, dim, R, tf - h, 2.0, is_max)) / (2 * h)
    _close(Jt.ravel(), ft, 1e-7)


@pytest.mark.parametrize("deg,R", [(5, 0), (5, 2)])
def test_angular_rate_yardstick_matches_the_port(deg, R):
    tf = 9.0
    Y = _Y(1, 2, deg, seed=11)
    val = np.array([float(v) for v in X.ang_rate(Y, 1, R, tf, 1.0)])
    _close(val, NP.ang_rate(Y, 1, R, tf, 1.0), 1e-11)
    J, Jt = X.ang_rate_jac(Y, 1, R, tf)
    J, Jt = np.array(J, dtype=float)[0], np.array(Jt, dtype=float)[0]
    fd = _central(lambda Yq: NP.ang_rate(Yq, 1, R, tf, 1.0), Y, 1e-5)
    _close(J, fd, 1e-5)
    h = 1e-5
    ft = (NP.ang_rate(Y, 1, R, tf + h, 1.0) - NP.ang_rate(Y, 1, R, tf - h, 1.0)) / (2 * h)
    _close(Jt, ft, 1e-6)


def test_energy_yardstick_matches_central_differences():
    dim, deg, R, tf = 2, 6, 3, 4.0
    Y = _Y(2, dim, deg, seed=5)

    def f(Yq, T=tf):
        return sum(NP._elev(NP._normsq(NP._diff(NP._diff(Yq[v * dim:(v + 1) * dim], T), T)), R).sum() for v in range(2))
    assert abs(float(X.deriv_energy(Y, 2, dim, R, tf, 2)) - f(Y)) <= 1e-12 * abs(f(Y))
    g, gt = X.deriv_energy_grad(Y, 2, dim, R, tf, 2)
    _close(np.array(g, dtype=float), _central(lambda Yq: [f(Yq)], Y, 1e-3)[0], 1e-8)
    h = 1e-5
    assert abs(float(gt) - (f(Y, tf + h) - f(Y, tf - h)) / (2 * h)) <= 1e-6 * abs(float(gt))


def test_library_exports_the_exact_derivatives():
    """ABI 7: the exact-derivative entry points exist in the library, the header and the binding table."""
    import ctypes
    from optimalbeziertrajectorygeneration_amd import _capi, build
    lib = ctypes.CDLL(build.build())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.abi_symbol_names(), name
    lib.obtg_abi_version.restype = ctypes.c_int
    assert lib.obtg_abi_version() == 7
    lib.obtg_kernel_name.restype = ctypes.c_char_p
    assert lib.obtg_kernel_name(_capi.K_JAC) == b"jac"
    assert _capi.K_COUNT == 9
