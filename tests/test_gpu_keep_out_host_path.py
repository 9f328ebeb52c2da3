"""The one host path of the keep-out entry points: what a caller can observe of it that the families' own tests
do not pin -- the return code of every refusal in its order, against a record taken on the commit before the entry points were
put on one path; that an output comes out the same whichever other outputs are asked for; and that a context's workspaces,
grown and shrunk by calls of every form in turn, give what a fresh context gives.  Tiny shapes: N = 3, degree 3, d = 2 and 3,
B = 2 (tests/keep_out_host_path_cases.py)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_out_host_path_cases as cases  # noqa: E402
from util import assert_identical  # noqa: E402

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keep_out_return_codes_parent.json")


# ------------------------------------------------------------------------------------------------ 1. return codes
@pytest.mark.gpu
def test_return_codes_are_the_parents():
    """Every case of the table -- all 26 entry points; each step of the refusal order of the context forms and of the free-curve
    forms, the precedence cases among them (a region or obstacle with more than 128 features together with a null Y; an empty
    call with a null pointer; a bad motion in an empty free-curve call) -- answers the code the parent commit's library gave.
    The codes are read from the record, not written here; a case without a record fails."""
    from optimalbeziertrajectorygeneration_amd import _capi
    with open(RECORD) as f:
        record = json.load(f)
    want = record["codes"]
    table = cases.ReturnCodeTable(_capi)
    try:
        ids = [case_id for case_id, _ in table.cases]
        assert len(set(ids)) == len(ids)
        assert {cases.entry(*f) for f in cases.FORMS} | {cases.entry(fam, dev=dev) for fam, dev in cases.FREE_FORMS} == \
            {case_id.split("|")[0] for case_id in ids} and len(cases.FORMS) + len(cases.FREE_FORMS) == 26
        missing = [case_id for case_id in ids if case_id not in want]
        assert not missing, "no record from %s for %d cases, the first: %s" % (record["parent_commit"], len(missing), missing[:3])
        wrong = []
        for case_id, thunk in table.cases:
            got = int(thunk())
            if got != want[case_id]:
                wrong.append((case_id, got, want[case_id]))
        assert not wrong, "%d of %d cases answer another code than %s, (case, now, then): %s" % (
            len(wrong), len(ids), record["parent_commit"], wrong[:5])
        # the record itself holds what it is meant to pin
        assert {cases.OK, cases.ERR_ARG, cases.ERR_UNSUPPORTED} == set(want[i] for i in ids)
        assert want["obtg_pair_keep_out_euclid_true_min|d=3|more than 128 features and null Y"] == cases.ERR_UNSUPPORTED
        assert want["obtg_keep_out_euclid_true_min_jac|d=3|more than 128 features and null jac"] == cases.ERR_UNSUPPORTED
        assert want["obtg_keep_out_true_min|d=2|B=0 and null Y"] == cases.ERR_ARG
        assert want["obtg_bern_keep_out|d=2|M=0 with nulls"] == cases.OK
        assert want["obtg_bern_keep_out_moving|d=2|M=0 and Km>K"] == cases.ERR_UNSUPPORTED
    finally:
        table.close()


# ------------------------------------------------------------------------------------------------ 2. optional outputs
def _ok(rc, what):
    assert rc == cases.OK, (what, rc)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", (2, 3))
def test_an_output_does_not_depend_on_which_others_are_asked_for(dim):
    """Every host entry point: the call with every output is the reference; with every optional output null, val (and jac and
    jac_tf where they are mandatory) is the same bits; with each optional output alone, that output is.  rel is optional in
    the forms that have it and jac comes with the _jac forms, so both states of the two columns whose device storage comes and
    goes are here."""
    from optimalbeziertrajectorygeneration_amd import _capi
    Y = cases.rows(dim)
    ctxs = {kind: cases.make_context(_capi, dim, kind) for kind in ("plain", "motion")}
    try:
        for fam, jac, dev in cases.FORMS:
            if dev:
                continue
            ctx, what = ctxs["motion" if cases.FAMILIES[fam][2] else "plain"], cases.entry(fam, jac)
            rc, ref = cases.call(ctx, fam, jac, False, Y)
            _ok(rc, what)
            assert (ref["status"] == 0).all() and np.isfinite(ref["val"]).all() and (ref["nodes"] >= 1).all(), what
            must = [k for k in cases.mandatory(fam, jac) if k in ref]
            for alone in [None] + cases.optional(fam, jac):
                rc, r = cases.call(ctx, fam, jac, False, Y, want=() if alone is None else (alone,))
                _ok(rc, (what, alone))
                assert sorted(r) == sorted(must + ([] if alone is None else [alone]))
                for k in r:
                    assert_identical(r[k], ref[k], "%s, %s alone: %s" % (what, alone, k))
        for fam, dev in cases.FREE_FORMS:
            if dev:
                continue
            what = cases.entry(fam)
            rc, ref = cases.call_free(ctxs["plain"], fam, False, dim)
            _ok(rc, what)
            assert (ref["status"] == 0).all() and np.isfinite(ref["val"]).all(), what
            for alone in (None, "t_star", "status"):
                rc, r = cases.call_free(ctxs["plain"], fam, False, dim, want=() if alone is None else (alone,))
                _ok(rc, (what, alone))
                assert sorted(r) == sorted(["val"] + ([] if alone is None else [alone]))
                for k in r:
                    assert_identical(r[k], ref[k], "%s, %s alone: %s" % (what, alone, k))
    finally:
        for c in ctxs.values():
            c.close()


# ------------------------------------------------------------------------------------------------ 3. workspace reuse
@pytest.mark.gpu
@pytest.mark.parametrize("dim", (2, 3))
def test_one_context_through_every_form_gives_what_a_fresh_one_gives(dim):
    """All 20 context forms on ONE context, the families interleaved, host and _dev calls alternating, B = 2, 5, 1, 2, 5, ... (the
    workspaces grow, then a smaller call reuses them): every output of every call is, bit for bit, what the same call gives on
    a context made for it alone.  The motion is set before a moving call and cleared before a static Euclidean one (which
    refuses a context with a motion); the tables and the region stay."""
    from optimalbeziertrajectorygeneration_amd import _capi
    order = ("static", "pair_euclid", "moving", "euclid", "pair")
    steps = [(order[k % 5], k >= 10, k % 2 == 1, (2, 5, 1)[k % 3]) for k in range(20)]
    assert sorted(s[:3] for s in steps) == sorted(cases.FORMS)
    ctx = cases.make_context(_capi, dim, "plain")
    has_motion = False
    try:
        for k, (fam, jac, dev, rows_) in enumerate(steps):
            moving = cases.FAMILIES[fam][2]
            if moving and not has_motion:
                ctx.set_keep_out_motion(*cases.motion(dim))
                has_motion = True
            elif fam == "euclid" and has_motion:
                ctx.set_keep_out_motion(np.zeros(0), np.zeros(0, np.int32), np.zeros(0))
                has_motion = False
            Y = cases.rows(dim, rows_, seed=k)
            rc, got = cases.call(ctx, fam, jac, dev, Y)
            _ok(rc, (k, fam, jac, dev))
            fresh = cases.make_context(_capi, dim, "motion" if moving else "plain")
            try:
                rc, want = cases.call(fresh, fam, jac, dev, Y)
            finally:
                fresh.close()
            _ok(rc, (k, fam, jac, dev, "fresh"))
            assert (want["status"] == 0).all() and np.isfinite(want["val"]).all()
            assert sorted(got) == sorted(want)
            for name in want:
                assert_identical(got[name], want[name], "step %d, %s: %s" % (k, cases.entry(fam, jac, dev), name))
    finally:
        ctx.close()
