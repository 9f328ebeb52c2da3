"""csrc/sweep_shape.h -- the grid of the planar hull-pair sweeps (k_gjk_swarm_planar, k_pair_sweep: workgroups per row,
passes per workgroup, hull pairs per pass, dynamic LDS) and the index rule by which a workgroup finds its pairs -- compiled
for the HOST.  The grid depends on the card's CU count, which a partitioned card reports as a fraction of 256, so the
shapes of such cards are walked here, where no GPU is needed: every workgroup of a row through every pass, counting how
often each hull pair is taken.  CPU only.

tests/golden/sweep_shape_parent.json pins every field to the arithmetic as it stood inside gjk_kernels.hip before it moved
into the header: the text of planar_lds_bytes, lds_share, the kLds* constants, tile_height, SweepShape and sweep_shape,
cut by line range from that file and put unchanged behind a five-integer stand-in for the context (n_hull_pairs, n_veh,
n_poly, n_obs, n_cus) in a stand-alone program, printed one record per case of CASES below; the program read the switches
from its environment as the launcher did, so it ran once per set of switches."""
import ctypes as C
import json
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSET = -2 ** 31
KNOB_ENV = ("OBTG_SWEEP_WGS", "OBTG_SWEEP_PASSES", "OBTG_TILE_A")
FIELDS = ("wgs", "passes", "chunk", "per_cu", "lds", "tile_height")
# (waves per SIMD, pairs per workgroup of a large batch): launch_gjk_swarm's plain sweep and pair_sweep_plan's
KINDS = {"plain": (5, 864), "pair": (4, 1280)}
CU_COUNTS = (0, 32, 64, 128, 256)         # 0: a device that reports none; 32 .. 128: partitioned compute modes of 256
BATCHES = (1, 2, 8, 37, 145, 289, 577)
# name -> N, degree, polygons, point obstacles, B: tests/test_gpu_sweep_shapes.py
TOYS = {"refill_deg5": (24, 5, 2, 0, 3), "c3_like": (36, 10, 3, 0, 9), "deg3": (30, 3, 0, 0, 8), "deg7": (30, 7, 2, 0, 1),
        "deg8": (30, 8, 2, 0, 1), "deg15": (36, 15, 2, 0, 2), "deg20": (26, 20, 0, 0, 2), "point_obs": (23, 10, 3, 5, 8),
        "tiled_deg15": (256, 15, 5, 0, 3), "tiled_dups": (603, 5, 2, 0, 2)}
TOY_PAIRS = {"refill_deg5": 324, "c3_like": 738, "deg3": 435, "deg7": 495, "deg8": 495, "deg15": 702, "deg20": 325, "point_obs": 322}

Case = namedtuple("Case", "id np n_obj nc n_cus B kind env")


def forced_sets(n_pairs):
    """name -> environment: the switches unset, and the (workgroups, passes) that tests/test_gpu_sweep_shapes.py forces."""
    sets = {"default": {}}
    for W, Q in ((1, 1), (1, 2), (1, 3), (2, 1), (3, 2), (5, 1), (n_pairs, 1), (n_pairs + 7, 1)):
        name = "W%sQ%d" % ("np" if W == n_pairs else "np7" if W == n_pairs + 7 else str(W), Q)
        sets[name] = {"OBTG_SWEEP_WGS": str(W), "OBTG_SWEEP_PASSES": str(Q)}
    return sets


def named_shapes():
    """name -> (hull pairs, staged objects, points per hull, batch sizes): synth.CONFIGS at the bench's B = N d (n - 1) + 1
    rows and at the small batches of a row-sharded step, and the toy shapes."""
    from optimalbeziertrajectorygeneration_amd import synth
    shapes = {}
    for name, cfg in synth.CONFIGS.items():
        n_curve = cfg.get("n_curve_obs", 0)
        n_pairs = len(synth.all_pairs(cfg["N"] + n_curve)[0]) if n_curve else len(synth.swarm_pairs(cfg["N"], cfg["n_poly"])[0])
        bench_B = cfg["N"] * cfg["d"] * (cfg["n"] - 1) + 1
        shapes[name] = (n_pairs, cfg["N"] + cfg["n_poly"] + n_curve, cfg["n"] + 1, (bench_B,) + BATCHES)
    for name, (N, n, M, n_obs, B) in TOYS.items():
        n_pairs = len(synth.swarm_pairs(N, M)[0]) + (4000 if name == "tiled_dups" else 0)
        assert TOY_PAIRS.get(name, n_pairs) == n_pairs
        shapes[name] = (n_pairs, N + M + n_obs, n + 1, (B,))
    return shapes


def make_cases():
    cases = []
    for name, (n_pairs, n_obj, nc, batches) in named_shapes().items():
        for B in batches:
            for n_cus in CU_COUNTS:
                for kind in KINDS:
                    for kname, env in forced_sets(n_pairs).items():
                        cases.append(Case("%s-B%d-cu%d-%s-%s" % (name, B, n_cus, kind, kname), n_pairs, n_obj, nc, n_cus, B, kind, env))
    for nc in (4, 6, 8, 9, 11, 16, 21):       # the tiled forms' tile height under OBTG_TILE_A
        for ta in ("4", "8", "32", "3", "40"):
            cases.append(Case("tile-nc%d-A%s" % (nc, ta), 1, 2, nc, 256, 1, "pair", {"OBTG_TILE_A": ta}))
    return cases


CASES = make_cases()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/sweep_shape.h compiled for the host with g++ (tests/native/sweep_shape_host.cpp)."""
    so = str(tmp_path_factory.mktemp("sweep_shape") / "libsweep_shape_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "native", "sweep_shape_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.ss_bytes.restype = C.c_longlong
    return lib


def knobs_of(host, monkeypatch, env):
    """the switches as a launch reads them: through the environment"""
    for k in KNOB_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    knobs = (C.c_int * 3)()
    host.ss_knobs_from_env(knobs)
    return knobs


def shape_of(host, knobs, n_pairs, n_obj, nc, n_cus, B, kind):
    waves, target = KINDS[kind]
    out = (C.c_longlong * 6)()
    host.ss_shape((C.c_int * 7)(n_pairs, n_obj, nc, n_cus, B, waves, target), knobs, out)
    return dict(zip(FIELDS, out))


def check_shape(host, s, n_pairs, n_obj, nc, what):
    """What the kernels rely on, whatever the shape: every hull pair of a row is taken exactly once by the workgroups
    w < wgs walking `passes` chunks each, none of them is idle from the start, a position within a chunk fits the
    unsigned short the history order is kept in, and the row is in LDS wherever the planar kernels are launched."""
    assert s["wgs"] >= 1 and s["passes"] >= 1 and s["chunk"] >= 1, what
    out = (C.c_int * 4)()
    host.ss_walk(n_pairs, s["wgs"], s["passes"], s["chunk"], out)
    assert (out[0], out[1]) == (1, 1), (what, "pairs taken min / max times", out[0], out[1])
    assert out[2] == 0, (what, "workgroups without a pair", out[2])
    assert s["chunk"] <= 65535, what
    launch_max, fixed = host.ss_bytes(1, 0, 0), host.ss_bytes(3, n_obj, nc)
    assert s["lds"] == fixed + 14 * s["chunk"], what
    # The launchers take the planar sweep only while lds <= kLdsLaunchMax (the one-launch pair sweep: kLdsDefaultMax), so
    # nothing above the limit is ever launched; what the shape owes them is a row that FITS wherever its objects leave room
    # for 256 pairs: per_cu workgroups in a CU's 160 KB, or one within the launch limit.  (Two per CU may be given up to
    # 80 KB -- 272 objects of 11 points, 2213 pairs: 65 546 bytes -- which the launchers then turn down for the tiled or
    # the general kernel: a slower form, not a wrong one, and as the parent had it.)
    assert 1 <= s["per_cu"] <= 5, what
    if s["per_cu"] > 1:
        assert s["per_cu"] * s["lds"] <= 160 * 1024, what
        assert s["lds"] <= host.ss_bytes(2, s["per_cu"], 0), what      # ... with the workgroups' static LDS beside it
    elif fixed + 14 * 256 <= launch_max:
        assert s["lds"] <= launch_max, what
    return out[3]


def test_unset_switches_read_as_unset(host, monkeypatch):
    assert list(knobs_of(host, monkeypatch, {})) == [UNSET] * 3
    assert list(knobs_of(host, monkeypatch, {"OBTG_SWEEP_WGS": "3", "OBTG_TILE_A": "12"})) == [3, UNSET, 12]
    assert list(knobs_of(host, monkeypatch, {"OBTG_SWEEP_PASSES": "2"})) == [UNSET, 2, UNSET]
    assert host.ss_bytes(0, 0, 0) == 48 * 1024 and host.ss_bytes(1, 0, 0) == 64 * 1024 and host.ss_bytes(2, 4, 0) == 40 * 1024 - 1280


def test_every_hull_pair_is_taken_once_at_the_named_shapes(host, monkeypatch):
    ragged = 0
    for case in CASES:
        knobs = knobs_of(host, monkeypatch, case.env)
        s = shape_of(host, knobs, case.np, case.n_obj, case.nc, case.n_cus, case.B, case.kind)
        ragged += check_shape(host, s, case.np, case.n_obj, case.nc, case.id) > 0
        assert 4 <= s["tile_height"] <= 32, case.id
    assert ragged > len(CASES) // 10          # (shapes whose last chunk is short or whose last passes are empty are among them)


def test_every_hull_pair_is_taken_once_over_a_grid_of_sizes(host, monkeypatch):
    knobs = knobs_of(host, monkeypatch, {})
    sizes, v = [], 1
    while v <= 40000:                         # 1, 2, 3, 5, 7, 10, 14, ... 40 000: uneven steps, ~1.37 x
        sizes.append(v)
        v = v + max(1, (v * 3) // 8)
    sizes += [127, 128, 129, 255, 256, 257, 863, 864, 865, 1280, 1281, 2528, 32640, 40000]
    assert len(sizes) > 40
    for n_pairs in sizes:
        n_all = int(np.ceil((1 + np.sqrt(1 + 8 * n_pairs)) / 2))      # objects of an all-pairs list of this length
        for n_obj in (n_all, n_all + 8, 4 * n_all):
            for B in (1, 7, 8, 9, 1153):
                for nc in (4, 6, 8, 9, 11, 16, 21):
                    for n_cus in CU_COUNTS:
                        for kind in KINDS:
                            s = shape_of(host, knobs, n_pairs, n_obj, nc, n_cus, B, kind)
                            check_shape(host, s, n_pairs, n_obj, nc, (n_pairs, n_obj, B, nc, n_cus, kind))


def test_forced_shapes_are_what_was_asked_for_where_lds_allows(host, monkeypatch):
    """OBTG_SWEEP_WGS = W, OBTG_SWEEP_PASSES = Q on the toy shapes: ceil(ceil(np / W) / Q) pairs per pass, and only as many
    workgroups as have a pair -- (np + 7, 1) is np workgroups of one pair."""
    for name, (n_pairs, n_obj, nc, batches) in named_shapes().items():
        if name not in TOY_PAIRS:
            continue
        for W, Q in ((1, 1), (1, 2), (1, 3), (2, 1), (3, 2), (5, 1), (n_pairs, 1), (n_pairs + 7, 1)):
            knobs = knobs_of(host, monkeypatch, {"OBTG_SWEEP_WGS": str(W), "OBTG_SWEEP_PASSES": str(Q)})
            for kind in KINDS:
                s = shape_of(host, knobs, n_pairs, n_obj, nc, 256, batches[0], kind)
                per_wg = -(-n_pairs // W)
                assert (s["passes"], s["chunk"]) == (Q, -(-per_wg // Q)), (name, W, Q, kind)
                assert s["wgs"] == -(-n_pairs // (s["passes"] * s["chunk"])) <= W, (name, W, Q, kind)


def test_the_small_batch_rule_follows_the_cu_count(host, monkeypatch):
    """tests/test_gpu_parity.py's C3 at B = 37 (2528 hull pairs) on a whole card: 19 workgroups of 134 pairs -- no lane of a
    256-lane workgroup ever refills.  A quarter of the card gives the same row 4 workgroups of 632."""
    knobs = knobs_of(host, monkeypatch, {})
    whole = shape_of(host, knobs, 2528, 72, 11, 256, 37, "pair")
    assert (whole["wgs"], whole["passes"], whole["chunk"]) == (19, 1, 134)
    quarter = shape_of(host, knobs, 2528, 72, 11, 64, 37, "pair")
    assert quarter["chunk"] > 256 and quarter["wgs"] < whole["wgs"]
    assert shape_of(host, knobs, 2528, 72, 11, 0, 37, "pair")["wgs"] == 2       # no CU count: the large batch's two per row


def test_every_field_is_the_parent_launchers(host, monkeypatch):
    with open(os.path.join(REPO, "tests", "golden", "sweep_shape_parent.json")) as f:
        golden = json.load(f)
    assert golden["fields"] == list(FIELDS)
    records = golden["records"]
    assert sorted(records) == sorted(c.id for c in CASES)
    for case in CASES:
        knobs = knobs_of(host, monkeypatch, case.env)
        s = shape_of(host, knobs, case.np, case.n_obj, case.nc, case.n_cus, case.B, case.kind)
        assert [s[k] for k in FIELDS] == records[case.id], case.id
