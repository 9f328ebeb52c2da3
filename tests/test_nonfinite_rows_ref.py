"""tests/nonfinite_rows_ref.py held to the reference on the CPU (tests/golden/nonfinite_rows.npz, written by
tests/golden/gen_nonfinite_rows.py from the reference's own functions): the expectation the device tests use --
`where(isfinite(row).all(), row.min(), nan)` -- is what the reference's reduced form returns, and the planting function
touches nothing but what it says."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite_rows_ref as NF  # noqa: E402


@pytest.fixture(scope="module")
def fix(golden_dir):
    return np.load(os.path.join(golden_dir, "nonfinite_rows.npz"))


def test_the_fixture_was_taken_on_these_inputs(fix):
    assert list(fix["plantings"]) == ["none"] + list(NF.PLANTINGS)
    assert float(fix["max_sep_rows"]) == NF.MAX_SEP
    assert np.array_equal(fix["rows_Y"], NF.fixture_rows_input(None))
    one, many = NF.fixture_seq_input(None)
    assert np.array_equal(fix["seq_one"], one) and np.array_equal(fix["seq_many"], many)


def test_planting_leaves_batch_row_0_and_the_other_vehicles_bit_identical():
    f = NF.FIX_ROWS
    Yb = NF.fixture_rows_input(None)
    before = Yb.copy()
    for what in NF.PLANTINGS:
        P = NF.plant(Yb, what, f["dim"])
        assert np.array_equal(Yb, before), "plant() changed its argument"
        assert P[0].tobytes() == Yb[0].tobytes(), what
        veh1 = slice(f["dim"], 2 * f["dim"])
        rest = np.ones(Yb.shape[1], bool)
        rest[veh1] = False
        assert P[1][rest].tobytes() == Yb[1][rest].tobytes(), what
        changed = P[1][veh1] != Yb[1][veh1]                       # (NaN != anything)
        assert changed.any(), what
        if what == "two control points of +-1e200":
            assert np.isfinite(P).all() and int(changed.sum()) == 2
        else:
            assert not np.isfinite(P[1][veh1][changed]).any(), what
        if what != "whole vehicle nan" and "1e200" not in what:
            assert int(changed.sum()) == 1, what
    one, many = NF.fixture_seq_input(None)
    for what in NF.PLANTINGS:
        o, m = NF.fixture_seq_input(what)
        for keep in (0, 2):
            assert o[keep].tobytes() == one[keep].tobytes(), what
        for keep in (0, 1, 3, 4):
            assert m[keep].tobytes() == many[keep].tobytes(), what
        assert o[1].tobytes() != one[1].tobytes() and m[2].tobytes() != many[2].tobytes(), what
    obs = np.arange(6.0).reshape(3, 2)
    po = NF.plant_obstacle(obs)
    assert np.isnan(po[0, -1]) and int(np.isnan(po).sum()) == 1 and np.array_equal(po[1:], obs[1:])


@pytest.mark.parametrize("R", NF.FIX_ROWS["elevs"])
def test_reference_rows_with_a_non_finite_element_have_a_nan_minimum(fix, R):
    """The reference's elev is a dense np.dot (R = 0: with the identity), so its row is NaN throughout as soon as one
    coefficient is not finite, and ndarray.min() of it is NaN: the expectation applied to the reference's full rows IS the
    reference's own reduction of them.  Vehicle 1 of batch row 1 is in pairs 0, 3 and 4 of (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)."""
    rows = fix["rows_R%d" % R]
    assert rows.shape == (1 + len(NF.PLANTINGS), NF.B, 6, 2 * NF.FIX_ROWS["deg"] + R + 1)
    assert np.isfinite(rows[0]).all()
    for i, what in enumerate(NF.PLANTINGS, 1):
        dirty = ~NF.clean(rows[i])
        assert not dirty[0].any(), what
        assert dirty[1].tolist() == [True, False, False, True, True, False], what
        assert np.isnan(rows[i][dirty]).all(), "%s: the reference's dirty rows are NaN in every element" % what
        want = rows[i].min(-1)                                      # ndarray.min(): what SequentialSwarm.py:65 takes
        assert np.isnan(want[dirty]).all(), what
        assert NF.same(NF.reduced_min(rows[i]), want), what
        assert NF.same(rows[i][0], rows[0][0]) and NF.same(rows[i][~dirty], rows[0][~dirty]), "%s: a clean row moved" % what
        for k in (1, 2, 3, 4):
            val, idx = NF.reduced_active(rows[i], k)
            assert np.isnan(val[dirty]).all() and (idx[dirty] == np.arange(k)).all(), (what, k)
            order = np.argsort(rows[i][~dirty], axis=-1, kind="stable")[:, :k]
            assert np.array_equal(idx[~dirty], np.sort(order, axis=-1)), (what, k)
            assert NF.same(val[~dirty], np.take_along_axis(rows[i][~dirty], idx[~dirty].astype(np.int64), axis=-1)), (what, k)
            assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < rows.shape[-1]
        assert NF.same(NF.reduced_active(rows[i], 1)[0][..., 0], NF.reduced_min(rows[i])), "%s: k = 1 is the minimum" % what


def test_the_reference_s_own_reduced_form_is_nan_exactly_on_the_planted_pairs(fix):
    """Examples/SequentialSwarm.py:43-70 on three candidates against five fixed trajectories, candidate 1 and trajectory 2
    planted: NaN for every pair with a planted curve, the unplanted value bit for bit elsewhere.  One exception, which the
    rule covers: +-1e200 planted in BOTH curves of a pair cancels in their difference, and that pair is clean."""
    out = fix["seq_out"]
    assert out.shape == (1 + len(NF.PLANTINGS), 3, 5) and np.isfinite(out[0]).all()
    planted = np.zeros((3, 5), bool)
    planted[1, :] = True
    planted[:, 2] = True
    for i, what in enumerate(NF.PLANTINGS, 1):
        want = planted.copy()
        if "1e200" in what:
            want[1, 2] = False
            one, many = NF.fixture_seq_input(what)
            d = one[1] - many[2]
            assert np.isfinite(d).all() and np.isfinite(out[i][1, 2])
        assert np.array_equal(np.isnan(out[i]), want), what
        assert not np.isinf(out[i]).any(), what
        keep = ~planted
        assert NF.same(out[i][keep], out[0][keep]), what


def test_the_expectation_on_rows_the_reference_never_produces():
    """The device's full rows may be dirty in FEWER elements than the reference's (band-limited sums skip the 0 * nan terms of
    np.dot): one +-inf or NaN element among finite ones still makes the row dirty."""
    rows = np.array([[3.0, 1.0, 2.0], [3.0, np.inf, 2.0], [-np.inf, 1.0, 2.0], [3.0, 1.0, np.nan], [np.nan] * 3, [1.0, 1.0, 0.5]])
    assert NF.same(NF.reduced_min(rows), [1.0, np.nan, np.nan, np.nan, np.nan, 0.5])
    val, idx = NF.reduced_active(rows, 2)
    assert NF.same(val, [[1.0, 2.0], [np.nan] * 2, [np.nan] * 2, [np.nan] * 2, [np.nan] * 2, [1.0, 0.5]])
    assert idx.tolist() == [[1, 2], [0, 1], [0, 1], [0, 1], [0, 1], [0, 2]]
