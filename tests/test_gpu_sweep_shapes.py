"""The gjkNew hull-pair sweeps (k_gjk_swarm_planar, k_pair_sweep, k_pair_sweep_tiled) against the ORACLE in every launch
shape: toy shapes just large enough that a 256-lane workgroup must refill its lanes, launched in the default grid and in
grids forced through OBTG_SWEEP_WGS / OBTG_SWEEP_PASSES (one workgroup per row, several passes on one staging, ragged last
chunks, one pair per workgroup), the tiled forms at four tile heights, and -- one fresh process each -- the switches read
once per process.  Every case holds every row and every pair to the oracle; every forced shape is bit for bit the default
shape; every call is made twice and the second launch (ordered by the first's trip counts) is bit for bit the first; and
ctx.sweep_shape (obtg_sweep_shape) must say that the intended form and grid are in effect before anything is compared.
Shapes, inputs and calls: tests/sweep_shape_child.py.  Needs a real MI355X: `pytest -m gpu`.

Child time limit: the default child (all eight toy shapes, every call twice) measured 2.77 s on an MI355X, start of the
interpreter to exit (2.47 s when run again); the limit is five times that, 13.85 s, rounded up to a multiple of 10 s: 20 s."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sweep_shape_child as S
from util import assert_close, assert_identical

pytestmark = pytest.mark.gpu

RTOL = 1e-9
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_MEASURED_S = 2.77      # the default child on an MI355X (see above)
CHILD_TIMEOUT_S = 20         # 5 x CHILD_MEASURED_S, rounded up to 10 s
SWITCHES = ("OBTG_SWEEP_WGS", "OBTG_SWEEP_PASSES", "OBTG_TILE_A", "OBTG_REFILL_MIN", "OBTG_HIST_SHIFT", "OBTG_FOLD_DYNAMICS",
            "OBTG_SEP_DYN_ELEV", "OBTG_ELEV_COOP")
FORCED = ((1, 1), (1, 2), (1, 3), (2, 1), (3, 2), (5, 1), ("np", 1), ("np+7", 1))


@pytest.fixture(scope="module")
def capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    assert _capi.device_count() > 0, "these tests need the GPU"
    return _capi


@pytest.fixture(scope="module")
def synth():
    from optimalbeziertrajectorygeneration_amd import synth
    return synth


@pytest.fixture
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ------------------------------------------------------------------------------------------------ inputs and the oracle
_INPUTS, _REFS, _DEFAULTS = {}, {}, {}


def inputs_of(name):
    if name not in _INPUTS:
        _INPUTS[name] = S.inputs(name)
    return _INPUTS[name]


def reference(oracle, synth, name, rows=None, max_iter=128, md_cap=256, deg_elev=0):
    """The oracle on the shape's two batches, computed once and left unchanged: gjkNew of every hull pair of every row (or of
    `rows`), the separation block (point obstacles: constant curves behind the vehicles, optimization.py:86-98), the speed and
    angular-rate rows."""
    key = (name, rows, max_iter, md_cap, deg_elev)
    if key in _REFS:
        return _REFS[key]
    inp = inputs_of(name)
    N, n, B = inp["N"], inp["n"], inp["B"]
    rows_ = list(range(B)) if rows is None else list(rows)
    ref = dict(rows=rows_)
    for batch in ("Yb", "Yfd"):
        Yr = inp[batch][rows_]
        ref[batch + "/gjk"] = [oracle.gjk_pairs(*synth.pack_polys(synth.hulls_from_Y(Yr[k], 2) + inp["polys"]), inp["pa"], inp["pb"],
                                                max_iter=max_iter, md_cap=md_cap, nthreads=4) for k in range(len(rows_))]
        Yo, n_sep = Yr, N
        if inp["obs"] is not None:
            n_obs = len(inp["obs"])
            const = np.repeat(inp["obs"].reshape(-1)[:, None], n + 1, 1)
            Yo, n_sep = np.concatenate([Yr, np.broadcast_to(const[None], (len(rows_), 2 * n_obs, n + 1))], axis=1), N + n_obs
        ref[batch + "/sep"] = oracle.eval_batch(Yo, 10.0, n_sep, 2, deg_elev, S.MAX_SEP, S.SPEED_BOUND, S.MAX_RATE, want=("sep",), nthreads=4)[0]
    _, ref["speed"], ref["ang"] = oracle.eval_batch(inp["Yb"][rows_], inp["tf"][rows_], N, 2, deg_elev, S.MAX_SEP, S.SPEED_BOUND, S.MAX_RATE,
                                                    want=("speed", "ang"), nthreads=4)
    _REFS[key] = ref
    return ref


def check_inputs(ref):
    """What makes the shape a test of the refill and of the history sort, asserted on the ORACLE's results: both flag
    values, at least four trip-count classes in one row, every pair finished (status 0) within md_cap = 256."""
    for batch in ("Yb", "Yfd"):
        rows = ref[batch + "/gjk"]
        assert all((o["status"] == 0).all() for o in rows), batch
        assert len(set(np.concatenate([o["flag"] for o in rows]).tolist())) >= 2, batch
        assert max(len(set(o["n_support"].tolist())) for o in rows) >= 4, batch


def check_against_oracle(out, ref, what, capped=False):
    """test_pair_sweep_at_bench_shape_vs_oracle's assertion on every row in ref["rows"] and every pair: flags, support counts
    and statuses equal, distances and closest points identical where the hulls are apart, the separation block (and the
    speed / angular-rate rows) within 1e-9."""
    calls = sorted(set(k.split("/")[0] for k in out if "#" not in k))
    assert calls, what
    for call in calls:
        batch = "Yfd" if call.startswith("pair_sweep_fd") else "Yb"
        for r, o in zip(ref["rows"], ref[batch + "/gjk"]):
            w = (what, call, "row", r)
            assert np.array_equal(out[call + "/flag"][r], o["flag"]), w
            assert np.array_equal(out[call + "/n_support"][r], o["n_support"]), w
            assert np.array_equal(out[call + "/status"][r], o["status"]), w
            if not capped:
                assert (o["status"] == 0).all(), w
            apart = (o["flag"] == 1) & (o["status"] == 0)
            for key in ("dist", "c1", "c2"):
                assert_identical(out[call + "/" + key][r][apart], o[key][apart], "%s %s" % (w, key))
        if call + "/sep" in out:
            assert_close(out[call + "/sep"][ref["rows"]], ref[batch + "/sep"], RTOL, "%s %s separation block" % (what, call))
        if call + "/speed" in out:
            assert_close(out[call + "/speed"][ref["rows"]], ref["speed"], RTOL, "%s %s speed rows" % (what, call))
            assert_close(out[call + "/ang"][ref["rows"]], ref["ang"], RTOL, "%s %s angular-rate rows" % (what, call))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_second_launch_and_view(out, what):
    for k in out:
        if "#2/" in k:
            assert np.array_equal(bits(out[k]), bits(out[k.replace("#2", "")])), (what, k, "second launch differs from the first")
        if k.startswith("pair_sweep_fd_view"):
            assert np.array_equal(bits(out[k]), bits(out[k.replace("fd_view", "fd_batch")])), (what, k, "FD view differs from its batch")


def check_same_bits(out, base, what):
    assert sorted(out) == sorted(base), what
    for k in out:
        assert np.array_equal(bits(out[k]), bits(base[k])), (what, k, "differs from the default shape's output")


def report(name, shapes, tag=""):
    for call, s in sorted(shapes.items()):
        print("SHAPE %s%s %s: form %s wgs %d passes %d chunk %d tile_height %d refill_min %d hist_shift %d fold_dyn %d"
              % (name, tag, call, s["form"], s["wgs"], s["passes"], s["chunk"], s["tile_height"], s["refill_min"], s["hist_shift"], s["fold_dyn"]))


def default_of(capi, name, deg_elev=0):
    """the default shape's outputs of this process (no switch set), made once"""
    import torch
    key = (name, deg_elev)
    if key not in _DEFAULTS:
        saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
        try:
            _DEFAULTS[key] = S.run_calls(capi, torch, inputs_of(name), deg_elev)
        finally:
            os.environ.update(saved)
    return _DEFAULTS[key]


def expected_forms(name):
    """The toy rows fit LDS: one launch of the planar sweep for every call, the speed / angular-rate groups in its grid up to
    11 points per hull; with de-duplication on, its own sequence."""
    if name in S.PLAIN_ONLY:
        return {"plain": "one_launch", "dedup": "dedup"}
    return {"plain": "one_launch", "pair": "one_launch", "all": "one_launch", "dedup": "dedup" if inputs_of(name)["B"] > 1 else "one_launch"}


# ------------------------------------------------------------------------------------------------ the toy shapes, in process
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_default_shape_vs_oracle(capi, oracle, synth, no_switches, name):
    ref = reference(oracle, synth, name)
    check_inputs(ref)
    out, launches, shapes = default_of(capi, name)
    report(name, shapes)
    assert {k: s["form"] for k, s in shapes.items()} == expected_forms(name)
    n_pairs = len(inputs_of(name)["pa"])
    for s in shapes.values():
        assert s["wgs"] * s["passes"] * s["chunk"] >= n_pairs > (s["wgs"] - 1) * s["passes"] * s["chunk"]
        assert (s["refill_min"], s["hist_shift"]) == (32, 0)
    if "all" in shapes:
        assert shapes["all"]["fold_dyn"] == (inputs_of(name)["n"] + 1 <= 11)
        n_launches = sum(launches["constraint_sweep"].values())
        assert n_launches == 1 if shapes["all"]["fold_dyn"] else n_launches >= 2, launches["constraint_sweep"]
        assert launches["pair_sweep"] == {"pair_sweep": 1} and launches["pair_sweep_fd_view"] == {"pair_sweep": 1}
    check_against_oracle(out, ref, name)
    check_second_launch_and_view(out, name)


@pytest.mark.parametrize("WQ", FORCED, ids=lambda wq: "W%s_Q%d" % wq)
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_forced_shape_vs_oracle_and_default(capi, oracle, synth, no_switches, name, WQ):
    import torch
    inp = inputs_of(name)
    n_pairs = len(inp["pa"])
    W = {"np": n_pairs, "np+7": n_pairs + 7}.get(WQ[0], WQ[0])
    Q = WQ[1]
    ref = reference(oracle, synth, name)
    base = default_of(capi, name)[0]
    no_switches.setenv("OBTG_SWEEP_WGS", str(W))
    no_switches.setenv("OBTG_SWEEP_PASSES", str(Q))
    out, launches, shapes = S.run_calls(capi, torch, inp)
    report(name, shapes, "[W%s,Q%d]" % WQ)
    # the forced grid is in effect: ceil(ceil(np / W) / Q) pairs per pass, Q passes, as many workgroups as have a pair
    chunk = -(-(-(-n_pairs // W)) // Q)
    want = dict(wgs=-(-n_pairs // (Q * chunk)), passes=Q, chunk=chunk)
    assert {k: s["form"] for k, s in shapes.items()} == expected_forms(name)
    for call, s in shapes.items():
        assert {k: s[k] for k in want} == want, (name, WQ, call, s)
    if WQ == (1, 1):
        assert want["chunk"] == n_pairs > 256        # one workgroup's lanes take more than one pair each
    check_against_oracle(out, ref, (name, WQ))
    check_second_launch_and_view(out, (name, WQ))
    check_same_bits(out, base, (name, WQ))


def test_without_the_shortcut(capi, oracle, synth, no_switches):
    """max_iter = 2, md_cap = 2: the sweeps' shortcut is off (it needs max_iter >= 3 and md_cap >= 2) and most pairs end at
    a cap: flags, support counts and STATUSES are the oracle's under the same caps, in the default grid and in one workgroup
    per row of two passes."""
    import torch
    name = "c3_like"
    inp = inputs_of(name)
    ref = reference(oracle, synth, name, max_iter=2, md_cap=2)
    assert any((o["status"] != 0).any() for o in ref["Yb/gjk"])
    calls = ["gjk_swarm", "pair_sweep", "constraint_sweep"]
    base, _, shapes = S.run_calls(capi, torch, inp, max_iter=2, md_cap=2, calls=calls)
    check_against_oracle(base, ref, "caps of 2", capped=True)
    check_second_launch_and_view(base, "caps of 2")
    no_switches.setenv("OBTG_SWEEP_WGS", "1")
    no_switches.setenv("OBTG_SWEEP_PASSES", "2")
    out, _, shapes = S.run_calls(capi, torch, inp, max_iter=2, md_cap=2, calls=calls)
    assert all((s["wgs"], s["passes"], s["chunk"]) == (1, 2, 369) for s in shapes.values()), shapes
    check_against_oracle(out, ref, "caps of 2, forced", capped=True)
    check_same_bits(out, base, "caps of 2, forced")


# ------------------------------------------------------------------------------------------------ the tiled forms
def default_tile_height(nc):
    """the tallest tile of which four workgroups' LDS (16 bytes per point of its TA + 64 objects at an odd pitch, 8 per object,
    14 per pair) fits a CU's 160 KB beside 1280 bytes of static LDS each: restated from DESIGN.md, not read from the header"""
    ta = 8
    while ta < 32 and 16 * (ta + 1 + 64) * (nc | 1) + 8 * (ta + 1 + 64) + 14 * (ta + 1) * 64 <= 160 * 1024 // 4 - 1280:
        ta += 1
    return ta


@pytest.mark.parametrize("tile_a", ["unset", "4", "8", "32"])
@pytest.mark.parametrize("name", list(S.TILED))
def test_tiled_forms_at_every_tile_height(capi, oracle, synth, no_switches, name, tile_a):
    """A fresh context per tile height (the chunk tables are cached per context).  The oracle on rows 0 and B - 1 (its CPU time
    is the test's); all rows of the second launch and of every forced height are held to the first launch / the default height."""
    import torch
    inp = inputs_of(name)
    B, nc = inp["B"], inp["n"] + 1
    assert all(len(p) <= nc for p in inp["polys"])
    ref = reference(oracle, synth, name, rows=(0, B - 1))
    assert all((o["status"] == 0).all() for o in ref["Yb/gjk"]) and len(set(ref["Yb/gjk"][0]["flag"].tolist())) >= 2
    calls = ["gjk_swarm", "pair_sweep", "constraint_sweep"]
    if tile_a != "unset":
        no_switches.setenv("OBTG_TILE_A", tile_a)
    out, launches, shapes = S.run_calls(capi, torch, inp, calls=calls)
    report(name, shapes, "[TILE_A %s]" % tile_a)
    height = default_tile_height(nc) if tile_a == "unset" else int(tile_a)
    assert (shapes["plain"]["form"], shapes["plain"]["tile_height"]) == ("tiled", height), shapes["plain"]
    assert shapes["plain"]["chunk"] <= 64 * height and shapes["plain"]["passes"] == 1
    if name == "tiled_dups":             # a tile cut into two chunks: the tiles cannot carry the separation rows
        assert shapes["pair"]["form"] == shapes["all"]["form"] == "two_launches"
    else:
        # The tiled pair sweep transposes its separation rows in the LDS behind a chunk's objects: 14 bytes per pair and 8
        # per object of a full TA x 64 tile must hold four waves x 8 rows x odd(2 n + 1) doubles.  Tiles of height 4 and 8
        # do not (4128 and 7744 bytes against 7936 at degree 15): the plan refuses them for two launches, and says so.
        behind, need = 14 * 64 * height + 8 * (height + 64), 4 * 8 * ((2 * inp["n"] + 1) | 1) * 8
        assert (behind >= need) == (tile_a in ("unset", "32"))
        if behind >= need:
            assert (shapes["pair"]["form"], shapes["pair"]["tile_height"]) == ("tiled", height), shapes["pair"]
            assert shapes["all"]["form"] == "tiled" and launches["pair_sweep"] == {"pair_sweep": 1}
        else:
            assert shapes["pair"]["form"] == shapes["all"]["form"] == "two_launches", shapes
            assert shapes["pair"]["tile_height"] == height and "pair_sweep" not in launches["pair_sweep"], (shapes, launches)
    check_against_oracle(out, ref, (name, tile_a))
    check_second_launch_and_view(out, (name, tile_a))
    if tile_a == "unset":
        _DEFAULTS[(name, "tiled")] = out
    else:
        if (name, "tiled") not in _DEFAULTS:
            for k in SWITCHES:
                no_switches.delenv(k, raising=False)
            _DEFAULTS[(name, "tiled")] = S.run_calls(capi, torch, inp, calls=calls)[0]
        check_same_bits(out, _DEFAULTS[(name, "tiled")], (name, tile_a))


# ------------------------------------------------------------------------------------------------ once-per-process switches
_CHILD_FAULT = []            # the first child that ended by a signal, an abort or its time limit: nothing more is started


def run_child(tmp_path, env_set, args=()):
    assert not _CHILD_FAULT, "an earlier child faulted (%s): no further process is started on the GPU" % _CHILD_FAULT[0]
    path = str(tmp_path / "child.npz")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_set)
    try:
        p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "sweep_shape_child.py"), path] + list(args), env=env,
                           timeout=CHILD_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        _CHILD_FAULT.append("time limit of %d s, %s" % (CHILD_TIMEOUT_S, env_set))
        raise
    if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
        _CHILD_FAULT.append("exit %d, %s" % (p.returncode, env_set))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:])
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files if k != "meta"}
        meta = json.loads(bytes(z["meta"]).decode())
    assert {k: v for k, v in meta["env"].items() if k in SWITCHES} == env_set
    return arrays, meta


def check_child_bits(capi, arrays, names, deg_elev=0):
    for name in names:
        base = default_of(capi, name, deg_elev)[0]
        got = {k[len(name) + 1:]: v for k, v in arrays.items() if k.startswith(name + "/")}
        check_same_bits(got, base, ("child", name))


@pytest.mark.parametrize("env_set,field,value", [
    ({"OBTG_REFILL_MIN": "1"}, "refill_min", 1),
    ({"OBTG_REFILL_MIN": "64"}, "refill_min", 64),
    ({"OBTG_HIST_SHIFT": "3"}, "hist_shift", 3),
    ({"OBTG_REFILL_MIN": "1", "OBTG_SWEEP_WGS": "1", "OBTG_SWEEP_PASSES": "2"}, "refill_min", 1),
], ids=["refill_min_1", "refill_min_64", "hist_shift_3", "refill_min_1_one_workgroup_two_passes"])
def test_child_with_a_once_per_process_switch(capi, no_switches, tmp_path, env_set, field, value):
    """Lanes refill one by one / only in whole waves; coarser trip-count bins; and the refill of single lanes inside passes of
    one workgroup per row: the same bits as this process's default shape."""
    arrays, meta = run_child(tmp_path, env_set)
    for name in S.SHAPES:
        shapes = meta[name]["shapes"]
        report(name, shapes, "[child %s]" % " ".join("%s=%s" % kv for kv in sorted(env_set.items())))
        assert all(s[field] == value for s in shapes.values()), (name, shapes)
        if "OBTG_SWEEP_WGS" in env_set:
            assert all((s["wgs"], s["passes"]) == (1, 2) for s in shapes.values()), (name, shapes)
    check_child_bits(capi, arrays, list(S.SHAPES))


def test_child_without_folded_dynamics(capi, no_switches, tmp_path):
    """OBTG_FOLD_DYNAMICS=0: the speed / angular-rate groups leave the sweep's grid for a launch of their own."""
    arrays, meta = run_child(tmp_path, {"OBTG_FOLD_DYNAMICS": "0"})
    for name in S.SHAPES:
        if name in S.PLAIN_ONLY:
            continue
        assert not meta[name]["shapes"]["all"]["fold_dyn"], name
        n_child, n_default = (sum(l["constraint_sweep"].values()) for l in (meta[name]["launches"], default_of(capi, name)[1]))
        assert n_child >= 2 and (n_child > n_default == 1 or inputs_of(name)["n"] + 1 > 11), (name, n_child, n_default)
    check_child_bits(capi, arrays, list(S.SHAPES))


@pytest.mark.parametrize("switch", ["OBTG_SEP_DYN_ELEV", "OBTG_ELEV_COOP"])
def test_child_with_degree_elevation(capi, oracle, synth, no_switches, tmp_path, switch):
    """DEG_ELEV = 2 on c3_like (two launches: the gjkNew sweep, and the separation rows with the dynamics groups among
    them).  OBTG_SEP_DYN_ELEV=0 gives the separation rows and the dynamics a launch each; so does OBTG_ELEV_COOP=0, which
    takes the cooperative-tile form of the elevated separation rows away -- the shared launch's separation workgroups are
    that form's (launch_sep_dynamics_elev) -- and leaves the per-wave form in a launch of its own."""
    arrays, meta = run_child(tmp_path, {switch: "0"}, args=["--elev", "2", "c3_like"])
    base = default_of(capi, "c3_like", 2)
    assert meta["c3_like"]["shapes"]["all"]["form"] == base[2]["all"]["form"] == "two_launches"
    n_default, n_child = (sum(l["constraint_sweep"].values()) for l in (base[1], meta["c3_like"]["launches"]))
    assert n_default == 2 and n_child == 3, (n_default, n_child)
    # (the elevated angular-rate rows of a vehicle almost at rest differ by up to 1e-8 between any two orders of operations,
    # the oracle's included -- DESIGN.md 4.2b --: they are held to the default's bits, everything else to the oracle too)
    check_against_oracle({k: v for k, v in base[0].items() if not k.endswith(("/ang", "/speed"))},
                         reference(oracle, synth, "c3_like", deg_elev=2), "DEG_ELEV = 2")
    check_child_bits(capi, arrays, ["c3_like"], 2)
