"""tests/collcheck_ref.py -- the collision checks restated over the oracle's gjkNew and split -- against the values and
gjkNew-call counts the reference returned (tests/golden/collcheck.npz, written by tests/golden/gen_collcheck.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collcheck_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collcheck.npz")
# node budget for the cases the reference did not finish: far above every finished case's count (at most a few hundred calls)
UNFINISHED_BUDGET = 20000


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _cases(gold, kind):
    for name in gold[kind + "_groups"]:
        name = str(name)
        g = {k[len(name) + 1:]: gold[k] for k in gold.files if k.startswith(name + "_") and k[len(name) + 1:] in
             ("curves", "pa", "pb", "pts", "off", "pc", "pp", "fin", "val", "calls")}
        yield name, g


def _one(kind, g, i, **kw):
    if kind == "cc":
        return R.coll_check(g["curves"][g["pa"][i]], g["curves"][g["pb"][i]], **kw)
    o = g["off"]
    p = g["pp"][i]
    return R.coll_check2poly(g["curves"][g["pc"][i]], g["pts"][o[p]:o[p + 1]], **kw)


@pytest.mark.parametrize("kind", ["cc", "cp"])
def test_restatement_is_the_reference_on_every_finished_case(gold, kind):
    n = 0
    for name, g in _cases(gold, kind):
        for i in np.flatnonzero(g["fin"] == 0):
            r = _one(kind, g, i)
            what = "%s[%d]" % (name, i)
            assert r["status"] == R.MD_OK, what
            assert r["res"] == g["val"][i], "%s: %r, the reference returned %r" % (what, r["res"], g["val"][i])
            assert r["gjk_calls"] == g["calls"][i], "%s: %d gjkNew calls, the reference made %d" % (what, r["gjk_calls"], g["calls"][i])
            assert r["nodes"] == r["gjk_calls"] and 1 <= r["depth"] <= 100, what
            n += 1
    assert n >= 20


@pytest.mark.parametrize("kind", ["cc", "cp"])
def test_restatement_stops_with_a_status_where_the_reference_does_not_finish(gold, kind):
    for name, g in _cases(gold, kind):
        for i in np.flatnonzero(g["fin"] != 0):
            r = _one(kind, g, i, max_nodes=UNFINISHED_BUDGET)
            assert r["status"] in (R.MD_NODE_CAP, R.MD_GJK_CAP) and r["res"] == 0.0, "%s[%d]: %r" % (name, i, r)


def test_random_groups_are_at_least_95_percent_finished(gold):
    for kind in ("cc", "cp"):
        for name, g in _cases(gold, kind):
            if name.startswith("usage"):
                continue
            assert (g["fin"] != 0).mean() <= 0.05, name


def test_usage_example_known_values(gold):
    """Examples/BezierUsageExamples.py: c3.collCheck(c4) is 0.0 after 5 gjkNew calls; c1.collCheck2Poly(poly2) is the case the
    reference does not come back from."""
    g = dict(_cases(gold, "cc"))["usage"]
    i = int(np.flatnonzero((g["pa"] == 2) & (g["pb"] == 3))[0])
    assert g["fin"][i] == 0 and g["val"][i] == 0.0 and g["calls"][i] == 5
    p = dict(_cases(gold, "cp"))["usage_poly"]
    i = int(np.flatnonzero((p["pc"] == 0) & (p["pp"] == 1))[0])
    assert p["fin"][i] != 0


def test_library_exports_the_collision_checks():
    """Both names are in the library, in obtg_abi_symbols and in the binding table; new symbols alone do not move the ABI
    revision, and the launches are timed under the _minDist family's id: no new kernel-stats id."""
    import ctypes as C
    from optimalbeziertrajectorygeneration_amd import _capi, build
    lib = C.CDLL(build.build())
    lib.obtg_abi_symbols.restype = C.POINTER(C.c_char)
    p, syms, i = lib.obtg_abi_symbols(), [], 0
    while True:                               # NUL-separated names, ended by an empty one
        s = b""
        while p[i] != b"\0":
            s += p[i]
            i += 1
        i += 1
        if not s:
            break
        syms.append(s.decode())
    for name in ("obtg_coll_check", "obtg_coll_check2poly"):
        assert hasattr(lib, name), name
        assert name in syms, name
        assert name in _capi.abi_symbol_names(), name
    assert "obtg_min_dist" in syms and len(syms) > 50
    lib.obtg_abi_version.restype = C.c_int
    assert lib.obtg_abi_version() == 7
    assert _capi.K_COUNT == 9
