"""The curvature and space-curvature families share one search body and one host path: every entry point of both --
*_poly, *_true_min, *_true_min_jac, their _dev twins, obtg_bern_[space_]curvature[_dev] -- reproduces, bit for bit, the
arrays tests/golden/curvature_one_body.npz recorded on the last commit that had a body per family (values, t_star, status,
Jacobian blocks, polynomial rows).  tests/golden/gen_curvature_one_body.py says what the batches are and which condition
their inputs meet (in every wave the search runs on one item at least and the first step answers one at least); the calls
are replayed with the generator's own replay(), nothing is generated here."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import gen_curvature_one_body as G  # noqa: E402

pytestmark = pytest.mark.gpu

_Z = np.load(G.PATH)
BATCHES = [str(b).split() for b in _Z["batches"]]


def test_the_file_holds_every_batch_the_issue_names():
    names = set(b[0] for b in BATCHES)
    for fam in ("planar", "space"):
        for deg in (3, 10, 15, 20, 4):
            assert "%s_rows_d%d_B2" % (fam, deg) in names
        for deg in (3, 10, 20, 4):
            assert "%s_rows_d%d_B%d" % (fam, deg, G.WIDE_B[fam]) in names
        for K in (2, 4, 5, 11, 16, 21, 32):
            assert "%s_free_K%d_M6" % (fam, K) in names
        cap = _Z["%s_cap_d3_B2/true_min_jac/status" % fam]
        assert (cap == 1).any()            # MD_NODE_CAP is among the recorded statuses


@pytest.mark.parametrize("name,kind,fam,max_nodes", BATCHES, ids=[b[0] for b in BATCHES])
def test_bits_of_the_recorded_outputs(name, kind, fam, max_nodes):
    x = _Z[name + ("/c" if kind == "free" else "/Y")]
    want = dict((k[len(name) + 1:], _Z[k]) for k in _Z.files if k.startswith(name + "/") and k[len(name) + 1:] not in ("c", "Y"))
    got = G.replay(kind, fam, x, int(max_nodes))
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype == np.float64:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, k, np.argwhere(a.view(np.uint64) != b.view(np.uint64))[:4])
        else:
            assert np.array_equal(a, b), (name, k)
