"""csrc/struct_layout.h -- the launch layout of the structured FD step (k_step_fd_structured) and the decode of its block
ids -- compiled for the HOST.  Every output element of the step is written exactly once only if the host's split and the
kernel's decode agree, so every block id of a layout is walked through the decode here and what it writes is counted: at
the toy shapes of tests/test_gpu_structured_dynamic_rows.py and at the bench shapes that no GPU test can afford (C4's
"more groups than half the slots", C5's elevated form with split D streams).  CPU only.

tests/golden/struct_layout_parent.json pins every field to the launcher's arithmetic as it stood inside
launch_step_fd_structured before it moved into the header: that text, copied verbatim into a stand-alone program, printed
one record per case of CASES below."""
import ctypes as C
import json
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSET = -2 ** 31
KNOB_ENV = ("OBTG_STRUCT_DYNAMIC_ROWS", "OBTG_STRUCT_DYNAMIC_SHARE", "OBTG_STRUCT_TICKET_ROWS", "OBTG_STRUCT_SEP_WGS", "OBTG_STRUCT_GJK_WGS")
SHAPE_KEYS = ("deg", "R", "n_veh", "n_pairs", "n_hull_pairs", "n_cus", "row0", "wpc", "gjk_chunk_pairs", "dyn_split")
S, F, G, D = 0, 1, 2, 3


class Layout(C.Structure):
    """StructLayout, field for field."""
    _fields_ = [(k, C.c_int) for k in ("n_sep_groups", "sep_rows_per", "gjk_chunks", "gjk_chunk_pairs", "gjk_rows_per", "fix_chunk")] + \
               [("n_kind", C.c_int * 4), ("per16", C.c_int * 4), ("pat", C.c_ubyte * 16), ("rank", C.c_ubyte * 16)] + \
               [(k, C.c_int) for k in ("dyn_groups_per_row", "dyn_rows_per", "dyn_streams", "dyn_fix_groups", "dyn_split", "first_pert",
                                       "sep_ticket_rows", "gjk_ticket_rows", "sep_static_ranges", "sep_static_rows",
                                       "gjk_static_ranges", "gjk_static_rows", "grid", "sep_sweepers", "gjk_sweepers", "tickets",
                                       "B", "n_veh", "n_hull_pairs")]

    def record(self):
        return {k: (list(getattr(self, k)) if isinstance(getattr(self, k), C.Array) else getattr(self, k)) for k, _ in self._fields_}


Case = namedtuple("Case", "id shape B env")


def shape(N, n, R, n_poly=0, n_curve_obs=0, wpc=4, dyn_split=0, n_cus=256, row0=0):
    """What launch_step_fd_structured hands struct_layout for a context of N vehicles of degree n (obtg_ctx_create: the
    separation block holds every pair of vehicles) with synth's hull pair list.  wpc and dyn_split are the plan's
    (step_fd_structured_plan: four workgroups per CU for flat rows of up to 40 KB of LDS, one for C4's 70 KB, two with
    DEG_ELEV > 0, where C5's D streams are split); the G chunk is 80 hull pairs, 64 where 16 bytes x objects x (n + 1 | 1)
    pass 40 KB."""
    from optimalbeziertrajectorygeneration_amd import synth
    n_hull = len(synth.all_pairs(N + n_curve_obs)[0]) if n_curve_obs else len(synth.swarm_pairs(N, n_poly)[0])
    chunk = 64 if 16 * (N + n_poly + n_curve_obs) * ((n + 1) | 1) > 40 * 1024 else 80
    return dict(deg=n, R=R, n_veh=N, n_pairs=N * (N - 1) // 2, n_hull_pairs=n_hull, n_cus=n_cus, row0=row0, wpc=wpc,
                gjk_chunk_pairs=chunk, dyn_split=dyn_split)


def config_shape(name, **kw):
    from optimalbeziertrajectorygeneration_amd import synth
    cfg = synth.CONFIGS[name]
    return shape(cfg["N"], cfg["n"], cfg["R"], cfg.get("n_poly", 0), cfg.get("n_curve_obs", 0), **kw)


def make_cases():
    # the hard forms of tests/test_gpu_structured_dynamic_rows.py: every row by ticket, 4 / 8 rows per ticket
    dynamic = {"OBTG_STRUCT_DYNAMIC_ROWS": "1", "OBTG_STRUCT_DYNAMIC_SHARE": "100", "OBTG_STRUCT_TICKET_ROWS": "4"}
    knob_sets = {"share_100": dynamic, "share_0_100": dict(dynamic, OBTG_STRUCT_DYNAMIC_SHARE="0,100"),
                 "ticket_1": dict(dynamic, OBTG_STRUCT_TICKET_ROWS="1"), "ticket_100": dict(dynamic, OBTG_STRUCT_TICKET_ROWS="100"),
                 "workers_1": dict(dynamic, OBTG_STRUCT_SEP_WGS="1", OBTG_STRUCT_GJK_WGS="1"),
                 "workers_256": dict(dynamic, OBTG_STRUCT_SEP_WGS="256", OBTG_STRUCT_GJK_WGS="256"),
                 "fixed_ranges": {"OBTG_STRUCT_DYNAMIC_ROWS": "0"}}
    small = {"3veh_deg3": dict(N=3, n=3, R=0, n_poly=2), "5veh_deg5": dict(N=5, n=5, R=0, n_poly=2)}
    sizes = (1, 2, 3, 4, 5, 7, 8, 9, 37)
    cases = []
    for name, sh in small.items():
        for B in sizes:
            cases.append(Case("%s-B%d" % (name, B), shape(**sh), B, {}))
            cases.append(Case("%s-row0_5-B%d" % (name, B), shape(row0=5, **sh), B, {}))
            for kname, env in knob_sets.items():
                cases.append(Case("%s-%s-B%d" % (name, kname, B), shape(**sh), B, env))
        cases.append(Case("%s-no_cu_count-B37" % name, shape(n_cus=0, **sh), 37, {}))
    cases.append(Case("C3-B1153", config_shape("C3"), 1153, {}))
    cases.append(Case("C3-fixed_ranges-B1153", config_shape("C3"), 1153, {"OBTG_STRUCT_DYNAMIC_ROWS": "0"}))
    cases.append(Case("C3-B145", config_shape("C3"), 145, {}))
    cases.append(Case("C3-no_cu_count-B1153", config_shape("C3", n_cus=0), 1153, {}))
    cases.append(Case("C4-B7169", config_shape("C4", wpc=1), 7169, {}))
    cases.append(Case("C5-B1153", config_shape("C5", wpc=2, dyn_split=1), 1153, {}))
    return cases


CASES = make_cases()


@pytest.fixture(scope="module")
def host_layout(tmp_path_factory):
    """csrc/struct_layout.h compiled for the host with g++ (tests/native/struct_layout_host.cpp)."""
    so = str(tmp_path_factory.mktemp("struct_layout") / "libstruct_layout_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "native", "struct_layout_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    assert lib.sl_sizeof_layout() == C.sizeof(Layout)
    return lib


@pytest.fixture
def layout_of(host_layout, monkeypatch):
    """case -> (lib, Layout): the case's switches go through the environment, as a launch reads them."""
    def run(case):
        for k in KNOB_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
        knobs = (C.c_int * 6)()
        host_layout.sl_knobs_from_env(knobs)
        sh = (C.c_int * len(SHAPE_KEYS))(*[case.shape[k] for k in SHAPE_KEYS])
        l = Layout()
        host_layout.sl_layout(sh, C.c_int(case.B), knobs, C.byref(l))
        return host_layout, l
    return run


def header_of(lib, l):
    buf = C.create_string_buffer(256)
    lib.sl_header(C.byref(l), buf, 256)
    return buf.value.decode()


def test_unset_switches_read_as_unset(host_layout, monkeypatch):
    for k in KNOB_ENV:
        monkeypatch.delenv(k, raising=False)
    knobs = (C.c_int * 6)()
    host_layout.sl_knobs_from_env(knobs)
    assert list(knobs) == [UNSET] * 6
    monkeypatch.setenv("OBTG_STRUCT_DYNAMIC_ROWS", "0")
    monkeypatch.setenv("OBTG_STRUCT_DYNAMIC_SHARE", "30,70")
    monkeypatch.setenv("OBTG_STRUCT_GJK_WGS", "256")
    host_layout.sl_knobs_from_env(knobs)
    assert list(knobs) == [0, 30, 70, UNSET, UNSET, 256]
    monkeypatch.setenv("OBTG_STRUCT_DYNAMIC_SHARE", "50")      # one number: both kinds
    host_layout.sl_knobs_from_env(knobs)
    assert list(knobs)[1:3] == [50, 50]


def stream_kind_written_once(lib, l, kind, ids, what):
    """S or G: per unit (separation group / hull-pair chunk) the fixed ranges tile [0, static_rows) and the tickets, drawn in
    sequence until the counter passes the end, [static_rows, B); sweepers exist exactly where swept rows do."""
    B = l.B
    units, rows_per, static_ranges, static_rows, ticket_rows, sweepers = \
        (l.n_sep_groups, l.sep_rows_per, l.sep_static_ranges, l.sep_static_rows, l.sep_ticket_rows, l.sep_sweepers) if kind == S else \
        (l.gjk_chunks, l.gjk_rows_per, l.gjk_static_ranges, l.gjk_static_rows, l.gjk_ticket_rows, l.gjk_sweepers)
    assert 0 <= static_rows <= B and static_ranges * rows_per >= static_rows, what
    assert len(ids) == units * (static_ranges + sweepers) == l.n_kind[kind], what
    written = np.zeros((units, B), dtype=np.int32)
    n_sweepers = np.zeros(units, dtype=np.int64)
    out = (C.c_int * 5)()
    for i in ids:
        lib.sl_worker(C.byref(l), kind, int(i), out)
        unit, rng, sweeper, b0, b1 = out
        assert 0 <= unit < units and 0 <= rng < static_ranges + sweepers, (what, i)
        if sweeper:
            assert l.tickets and rng >= static_ranges, (what, i)
            n_sweepers[unit] += 1
        else:
            assert rng < static_ranges and 0 <= b0 < b1 <= static_rows, (what, i, b0, b1)
            written[unit, b0:b1] += 1
    assert (written[:, :static_rows] == 1).all() and (written[:, static_rows:] == 0).all(), what
    assert (n_sweepers == sweepers).all(), what
    assert (sweepers > 0) == (l.tickets != 0 and static_rows < B), what
    if not l.tickets:
        assert static_rows == B and sweepers == 0, what
        return
    # the tickets of one unit (every unit's counter hands out the same rows): whoever draws them, in this order
    assert ticket_rows >= 1, what
    swept = np.zeros(B, dtype=np.int32)
    cur, rows = 0, (C.c_int * 2)()
    while cur < B - static_rows:
        lib.sl_ticket(C.byref(l), kind, cur, rows)
        assert static_rows <= rows[0] < rows[1] <= B, (what, cur)
        swept[rows[0]:rows[1]] += 1
        cur += ticket_rows
    assert (swept[static_rows:] == 1).all() and (swept[:static_rows] == 0).all(), what


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_element_is_written_once(layout_of, case):
    lib, l = layout_of(case)
    B, what = case.B, case.id
    assert l.B == B and l.grid > 0 and l.grid % 16 == 0
    # the 16-slot pattern
    assert sum(l.per16) == 16
    seen = [0, 0, 0, 0]
    for i in range(16):
        assert l.rank[i] == seen[l.pat[i]], what
        seen[l.pat[i]] += 1
    assert seen == list(l.per16), what
    # every block id -> (kind, id): the ids below n_kind[k] exactly once, the others return
    blocks = np.zeros((l.grid, 3), dtype=np.int32)
    lib.sl_blocks(C.byref(l), blocks.ctypes.data_as(C.c_void_p))
    ids = {}
    for k in range(4):
        of_kind = blocks[blocks[:, 0] == k]
        assert ((of_kind[:, 1] < l.n_kind[k]) == (of_kind[:, 2] != 0)).all(), what
        ids[k] = np.sort(of_kind[of_kind[:, 2] != 0, 1])
        assert np.array_equal(ids[k], np.arange(l.n_kind[k])), (what, k)
    assert ((blocks[:, 0] >= 0) & (blocks[:, 0] < 4) & (blocks[:, 1] >= 0)).all(), what
    # S and G
    stream_kind_written_once(lib, l, S, ids[S], (what, "S"))
    stream_kind_written_once(lib, l, G, ids[G], (what, "G"))
    assert l.n_sep_groups == (case.shape["n_pairs"] + 63) // 64, what
    pairs, out2 = np.zeros(case.shape["n_hull_pairs"], dtype=np.int32), (C.c_int * 2)()
    for c in range(l.gjk_chunks):
        lib.sl_chunk_pairs(C.byref(l), c, out2)
        assert 0 < out2[1] <= l.gjk_chunk_pairs, (what, c)
        pairs[out2[0]:out2[0] + out2[1]] += 1
    assert (pairs == 1).all(), what
    # F: rows first_pert .. B-1 once each
    assert l.first_pert == (0 if case.shape["row0"] > 0 else 1), what
    assert sorted(lib.sl_fix_row(C.byref(l), int(i)) for i in ids[F]) == list(range(l.first_pert, B)), what
    # D: the streams tile rows x vehicle groups (x 4 subgroups of 16 vehicles with dyn_split), the fix-up groups the perturbed
    # rows in 64s, the own-tf groups rows 1 .. B-1 in 8s per vehicle group
    n_veh, gd = case.shape["n_veh"], l.dyn_groups_per_row
    assert gd == (n_veh + 63) // 64 and l.dyn_split == case.shape["dyn_split"], what
    streamed = np.zeros((B, n_veh), dtype=np.int32)
    fixed = np.zeros(B, dtype=np.int32)
    own_tf = np.zeros((B, gd), dtype=np.int32)
    out6 = (C.c_int * 6)()
    for i in ids[D]:
        lib.sl_dyn(C.byref(l), int(i), out6)
        part, group, sub, b0, b1, live = out6
        assert 0 <= group and 0 <= b0 <= b1 <= B, (what, i)
        if part == 0:
            assert i < l.dyn_streams and group < gd and b0 < b1 <= b0 + min(64, l.dyn_rows_per), (what, i)
            if l.dyn_split:
                assert 0 <= sub < 4 and bool(live) == (64 * group + 16 * sub < n_veh), (what, i)
                v0, v1 = 64 * group + 16 * sub, min(n_veh, 64 * group + 16 * sub + 16)
            else:
                assert sub == -1 and live, (what, i)
                v0, v1 = 64 * group, min(n_veh, 64 * group + 64)
            if live:
                streamed[b0:b1, v0:v1] += 1
        elif part == 1:
            assert l.dyn_streams <= i < l.dyn_streams + l.dyn_fix_groups and b1 - b0 <= 64 and b0 == l.first_pert + 64 * group, (what, i)
            fixed[b0:b1] += 1
        else:
            assert part == 2 and i >= l.dyn_streams + l.dyn_fix_groups and group < gd and b1 - b0 <= 8, (what, i)
            own_tf[b0:b1, group] += 1
    assert (streamed == 1).all(), what
    assert (fixed[l.first_pert:] == 1).all() and (fixed[:l.first_pert] == 0).all(), what
    assert (own_tf[1:] == 1).all() and (own_tf[:1] == 0).all(), what


def test_the_bench_shapes_take_the_branches_they_are_here_for(layout_of):
    by_id = {c.id: c for c in CASES}
    _, c3 = layout_of(by_id["C3-B1153"])
    assert c3.tickets and c3.sep_sweepers > 0 and c3.n_kind[S] == 32 * (54 + 32) and (c3.sep_ticket_rows, c3.gjk_ticket_rows) == (4, 9)
    _, c4 = layout_of(by_id["C4-B7169"])
    assert not c4.tickets and 2 * (c4.n_sep_groups + c4.gjk_chunks) > 256 * 1       # tickets off by shape
    _, c5 = layout_of(by_id["C5-B1153"])
    assert not c5.tickets and c5.dyn_split and c5.dyn_streams == 4 * c5.dyn_groups_per_row * -(-1153 // c5.dyn_rows_per)


def test_recorded_launches(layout_of):
    """The first line of the workgroup timelines recorded at C3 with and without the sweepers.  The parent's was taken
    before the header carried the ticket sizes: with the tickets off today's header ends in ` ticket_rows 0 0` behind the
    recorded text."""
    by_id = {c.id: c for c in CASES}
    prof = os.path.join(REPO, "profiles", "struct_dynamic_rows")
    with open(os.path.join(prof, "timeline_child_c3.txt")) as f:
        child = f.readline().rstrip("\n")
    with open(os.path.join(prof, "timeline_parent_c3.txt")) as f:
        parent = f.readline().rstrip("\n")
    assert header_of(*layout_of(by_id["C3-B1153"])) == child
    assert header_of(*layout_of(by_id["C3-fixed_ranges-B1153"])) == parent + " ticket_rows 0 0"
    # two older recordings that today's arithmetic still reproduces: C4's timeline, and C5's final tree of round 4
    with open(os.path.join(REPO, "profiles", "r03_experiments", "timeline_structured_c4.txt")) as f:
        assert header_of(*layout_of(by_id["C4-B7169"])) == f.readline().rstrip("\n") + " ticket_rows 0 0"
    with open(os.path.join(REPO, "profiles", "r04_experiments", "structured_c5_coop_kinds.txt")) as f:
        final_tree = f.read().split("== final tree")[1].splitlines()[1]
    assert header_of(*layout_of(by_id["C5-B1153"])) == final_tree + " ticket_rows 0 0"


def test_every_field_is_the_parent_launchers(layout_of):
    with open(os.path.join(REPO, "tests", "golden", "struct_layout_parent.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(c.id for c in CASES)
    for case in CASES:
        lib, l = layout_of(case)
        got = dict(l.record(), header=header_of(lib, l))
        want = golden[case.id]
        assert {k: got[k] for k in want} == want, case.id
        assert sorted(want) == sorted(set(got) - {"n_veh", "n_hull_pairs"}), case.id      # (the two are the shape's, echoed for the decode)
