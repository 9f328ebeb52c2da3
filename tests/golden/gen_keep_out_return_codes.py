#!/usr/bin/env python3
"""Record tests/golden/keep_out_return_codes_parent.json: the return code of every case of tests/keep_out_host_path_cases.py's
table, answered by the library of the commit BEFORE the keep-out entry points were put on one host path.  Needs a GPU.

    OBTG_LIB=<libobtg_hip.so built from that commit> python -B tests/golden/gen_keep_out_return_codes.py --commit <its hash> [--out PATH]

tests/test_gpu_keep_out_host_path.py holds every later build to this record, case by case; a case the table has and the record
lacks fails there, so a new case means a new record taken on that same commit's library."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import keep_out_host_path_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under OBTG_LIB was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "keep_out_return_codes_parent.json"))
    a = ap.parse_args()
    from optimalbeziertrajectorygeneration_amd import _capi
    assert os.environ.get("OBTG_LIB"), "OBTG_LIB must name the parent commit's library"
    table = cases.ReturnCodeTable(_capi)
    try:
        codes = {}
        for case_id, thunk in table.cases:
            assert case_id not in codes, case_id
            codes[case_id] = int(thunk())
    finally:
        table.close()
    with open(a.out, "w") as f:
        json.dump({"parent_commit": a.commit, "library_source_hash": _capi.source_hash("all"), "cases": len(codes), "codes": codes}, f,
                  indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, codes %s" % (a.out, len(codes), sorted(set(codes.values()))))


if __name__ == "__main__":
    main()
