"""Curves on different time spans, the CPU side: tests/aligned_ref.py (the NumPy restatement of the reference's
`_temporalAlignment` -> sub -> normSquare -> elev -> min) against every value of tests/golden/aligned.npz, which the reference
wrote; the fixture's own make-up; and what the library and the package must export for the device path.  No GPU call."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aligned_ref as A  # noqa: E402
from util import assert_close  # noqa: E402

NEW_SYMBOLS = ("obtg_one_vs_many_min_spans", "obtg_one_vs_many_min_spans_dev", "obtg_bern_restrict")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "aligned.npz"))


def groups(fx):
    return [(str(g), int(d), int(n)) for g, d, n in zip(fx["groups"], fx["dims"], fx["degs"])]


def test_fixture_make_up(fx):
    """every group: 20..45 % of the pairs without overlap, at least 100 with; the wanted shapes; the no-split branches hit"""
    shapes = {(d, n) for _, d, n in groups(fx)}
    assert {(2, 5), (3, 5), (3, 3), (2, 10)} <= shapes and any(n == 4 for _, n in shapes)
    for g, dim, deg in groups(fx):
        none, s1, s2 = fx[g + "_none"], fx[g + "_s1"], fx[g + "_s2"]
        assert 0.20 <= none.mean() <= 0.45, g
        assert (~none).sum() >= 100, g
        assert (s1[:, 0] < s1[:, 1]).all() and (s2[:, 0] < s2[:, 1]).all()
        over = ~none
        assert ((s1[:, 0] == s2[:, 0]) & (s1[:, 1] != s2[:, 1]) & over).any(), g + ": equal starts"
        assert ((s1[:, 0] != s2[:, 0]) & (s1[:, 1] == s2[:, 1]) & over).any(), g + ": equal ends"
        assert ((s1 == s2).all(axis=1) & over).any(), g + ": equal spans"
        assert (((s1[:, 1] == s2[:, 0]) | (s2[:, 1] == s1[:, 0])) & none).any(), g + ": touching spans"
        assert fx[g + "_c1"].shape == (len(none), dim, deg + 1)
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligned.npz")) < 1000000


def test_restatement_against_the_reference(fx):
    """alignment, sum, separation rows and minimum: 1e-9 (tests/util.py) on every fixture value; the None mask identical,
    the span ends exactly equal"""
    max_sep = float(fx["max_sep"])
    for g, dim, deg in groups(fx):
        c1, c2, s1, s2, none = (fx[g + k] for k in ("_c1", "_c2", "_s1", "_s2", "_none"))
        for i in range(len(none)):
            al = A.align(c1[i], s1[i], c2[i], s2[i])
            assert (al is None) == bool(none[i]), "%s pair %d: None mask" % (g, i)
            if al is None:
                assert A.sep_rows(c1[i], s1[i], c2[i], s2[i], 10) is None
                assert A.sep_min(c1[i], s1[i], c2[i], s2[i], 10, max_sep, 123.0) == 123.0
                continue
            assert tuple(fx[g + "_ends"][i]) == al[2], "%s pair %d: span ends" % (g, i)
            what = "%s pair %d " % (g, i)
            assert_close(al[0], fx[g + "_a1"][i], what=what + "aligned c1")
            assert_close(al[1], fx[g + "_a2"][i], what=what + "aligned c2")
            assert_close(al[0] + al[1], fx[g + "_add"][i], what=what + "add")
            for R in fx["elevs"]:
                R = int(R)
                assert_close(A.sep_rows(c1[i], s1[i], c2[i], s2[i], R), fx["%s_rows%d" % (g, R)][i], what=what + "rows R=%d" % R)
        for R in fx["elevs"]:
            R = int(R)
            got = np.array([A.sep_min(c1[i], s1[i], c2[i], s2[i], R, max_sep) for i in range(len(none))])
            assert (np.isinf(got) == none).all()
            assert_close(got[~none], fx["%s_min%d" % (g, R)][~none], what="%s minima R=%d" % (g, R))


def test_library_and_binding_export_the_new_entries():
    from optimalbeziertrajectorygeneration_amd import _capi, build
    lib = ctypes.CDLL(build.build())
    lib.obtg_abi_symbols.restype = ctypes.c_void_p
    p, names = lib.obtg_abi_symbols(), []
    while True:
        s = ctypes.string_at(p)
        if not s:
            break
        names.append(s.decode())
        p += len(s) + 1
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libobtg_hip.so does not export " + name
        assert name in names, name + " missing from obtg_abi_symbols"
        assert name in _capi.abi_symbol_names(), name + " missing from the binding table"
    lib.obtg_abi_version.restype = ctypes.c_int
    assert lib.obtg_abi_version() == 7
    assert _capi.K_COUNT == 9
    for m in ("one_vs_many_min_spans", "one_vs_many_min_spans_dev", "bern_restrict"):
        assert callable(getattr(_capi.Context, m))


def test_align_keyword_and_operators():
    from optimalbeziertrajectorygeneration_amd import bezier, sequential
    for m in (bezier.Bezier.sub, bezier.Bezier.add):
        assert inspect.signature(m).parameters["align"].default is False
    assert callable(bezier._temporalAlignment)
    a = bezier.Bezier([[0.0, 1.0, 2.0]], t0=0.0, tf=10.0)
    b = bezier.Bezier([[1.0, 1.0, 0.0]], t0=3.0, tf=12.5)
    for op in (lambda: a - b, lambda: a + b, lambda: a.sub(b), lambda: a.add(b)):
        with pytest.raises(NotImplementedError, match="align=True"):
            op()
    # spans without overlap (touching ones too) need no device: None, as in the reference
    c = bezier.Bezier([[1.0, 1.0, 0.0]], t0=10.0, tf=12.0)
    assert a.sub(c, align=True) is None and a.add(c, align=True) is None and c.sub(a, align=True) is None
    # the planner's keywords
    assert "spans" in inspect.signature(sequential.new_vs_all).parameters
    assert "new_span" in inspect.signature(sequential.new_vs_all).parameters
    for f in (sequential.temporalSeparationConstraints, sequential.nonlcon, sequential.nonlcon_jac, sequential.plan):
        assert "spans" in inspect.signature(f).parameters
    p = sequential.Parameters(3, 3, 5, 10.0, 0.9, t0s=[0.0, 1.0, 2.0], tfs=[5.0, 6.0, 7.0])
    assert p.t0s.tolist() == [0.0, 1.0, 2.0] and sequential.Parameters(3, 3, 5, 10.0, 0.9).t0s is None
    assert np.isfinite(sequential.NO_OVERLAP) and sequential.NO_OVERLAP > 0
