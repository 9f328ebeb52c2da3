#!/usr/bin/env python3
"""Generate tests/golden/nonfinite_rows.npz by RUNNING THE REFERENCE on control points that hold NaN, +-inf or values whose
products overflow.

    python -B tests/golden/gen_nonfinite_rows.py

Two parts, both on the inputs and plantings of tests/nonfinite_rows_ref.py (index 0 of every array: nothing planted):

  seq_out[1 + plantings][3][5]        Examples/SequentialSwarm.py:43-70 `temporalSeparationConstraints` -- the reference's own
                                      reduced form, `dv.normSquare().elev(10).cpts.min() - maxSep**2` -- for each of three
                                      candidates against five fixed trajectories (3-D, degree 5), candidate 1 and fixed
                                      trajectory 2 planted
  rows_R0, rows_R6[1 + plantings][2][6][2 * 5 + R + 1]
                                      optimization.py:311-346 `_temporalSeparationConstraints` with DEG_ELEV 0 and 6: the full
                                      rows of 4 vehicles (2-D, degree 5), vehicle 1 of batch row 1 planted

and the unplanted inputs (rows_Y, seq_one, seq_many), so that the test can tell a changed random stream from a changed
reference.  gen_golden.py is imported for its injections (it makes the reference importable); nothing of the reference is
copied.  Exits cleanly where the reference is absent (gen_golden does).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.argv = [sys.argv[0], "none"]
import gen_golden as GG  # noqa: E402  (exits when the reference is absent)

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import nonfinite_rows_ref as NF  # noqa: E402

import SequentialSwarm as SS  # noqa: E402  (reference)

opt = GG.opt


def full_rows(Yb, R):
    f = NF.FIX_ROWS
    opt.DEG_ELEV = R
    try:
        with np.errstate(all="ignore"):
            out = np.stack([np.asarray(opt._temporalSeparationConstraints(Y, f["n_veh"], f["dim"], NF.MAX_SEP), dtype=float) for Y in Yb])
    finally:
        opt.DEG_ELEV = 0
    return out.reshape(len(Yb), f["n_veh"] * (f["n_veh"] - 1) // 2, 2 * f["deg"] + R + 1)


def seq_out(one, many):
    f = NF.FIX_SEQ
    out = []
    with np.errstate(all="ignore"):
        for b in range(one.shape[0]):
            y = np.concatenate([one[b], many.reshape(-1, many.shape[-1])])
            out.append(np.asarray(SS.temporalSeparationConstraints(y, f["n_traj"], f["dim"], f["max_sep"]), dtype=float))
    return np.stack(out)


def main():
    whats = (None,) + NF.PLANTINGS
    d = {"plantings": np.array(["none"] + list(NF.PLANTINGS)), "max_sep_rows": np.float64(NF.MAX_SEP)}
    d["rows_Y"] = NF.fixture_rows_input(None)
    d["seq_one"], d["seq_many"] = NF.fixture_seq_input(None)
    for R in NF.FIX_ROWS["elevs"]:
        d["rows_R%d" % R] = np.stack([full_rows(NF.fixture_rows_input(w), R) for w in whats])
    d["seq_out"] = np.stack([seq_out(*NF.fixture_seq_input(w)) for w in whats])
    for k in ("rows_R0", "rows_R6", "seq_out"):
        a = d[k]
        print("  %-8s %s, %d non-finite of %d" % (k, a.shape, int((~np.isfinite(a)).sum()), a.size))
    path = os.path.join(HERE, "nonfinite_rows.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    if os.path.getsize(path) >= 64 * 1024:
        raise SystemExit("nonfinite_rows.npz is meant to stay small")


if __name__ == "__main__":
    main()
