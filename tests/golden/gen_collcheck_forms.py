#!/usr/bin/env python3
"""Generate tests/golden/collcheck_forms.npz by RUNNING THE REFERENCE's two collision checks on a subset of
tests/collcheck_cases.py: the forms tests/golden/collcheck.npz does not hold.

    python -B tests/golden/gen_collcheck_forms.py

  nf_xy, nf_z            the 27 non-finite plantings x 5 pairs (rows x and y: 2-D curves; row z: 3-D curves)
  nf_poly_xy, nf_poly_z  a planted curve against a triangle, a curve against a triangle with a planted vertex
  planar_K13             the first 24 pairs of the planar base of 13 control points
  plane_yz_K4, _K13      the first 24 pairs of the bases of 4 and 13 control points in the plane x = 0.5
  shear_zx_K4            six crossing pairs of the base of 4 control points in the plane z = x

As gen_collcheck.py: gen_golden.py is imported for its injections and for `guarded`; the file holds the inputs, the value
each call returned, the number of gjkNew calls it made and whether the reference finished (0), ran out of its time budget
(1) or overflowed its stack (2).  Nothing of the reference is copied.  Exits cleanly where the reference is absent.
A search tests/collcheck_ref.py ends with MD_GJK_CAP or MD_NODE_CAP is one the reference does not come back from; those
are recorded as unfinished and held by status alone, so no share of finished cases is asked for here.
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.argv = [sys.argv[0], "none"]
import gen_collcheck as GC  # noqa: E402  (imports gen_golden, which exits when the reference is absent)

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import collcheck_cases as C  # noqa: E402

GC.BUDGET = 30.0           # seconds per case: every case the reference finishes takes well under a second
# gen_golden's support-index trace looks a support point up by `==`, which a NaN row never answers; nothing here reads
# the trace, so the reference's own supportPts goes back in (the gjkNew-call counter stays)
GC.GG.G.supportPts = GC.GG._orig_supportPts


def main():
    warnings.simplefilter("ignore")
    d = {"cc_groups": [], "cp_groups": []}
    cc, cp = C.recorded_groups()
    for name, curves, pa, pb, planar in cc:
        GC.cc_group(d, name, curves, pa, pb, planar=planar, exempt=True)
    for name, curves, polys, pc, pp, planar in cp:
        GC.cp_group(d, name, curves, polys, pc, pp, planar=planar, exempt=True)
    d["cc_groups"], d["cp_groups"] = np.array(d["cc_groups"]), np.array(d["cp_groups"])
    path = os.path.join(HERE, "collcheck_forms.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes; collcheck.npz has %d)" % (path, os.path.getsize(path), os.path.getsize(os.path.join(HERE, "collcheck.npz"))))


if __name__ == "__main__":
    main()
