"""obtg_constraint_sweep_dev(dY = NULL) inside an FD view routes to the structured step (k_step_fd_structured) where that
kernel applies and the brute-force form is one launch.  The independent side of every comparison here is the brute-force
sweep of the MATERIALISED batch (obtg_fd_batch_dev + obtg_constraint_sweep_dev(dY, ...)), which never routes: the rows of
the view written to memory and evaluated in full, row by row."""
import re
import os

import numpy as np
import pytest

from util import assert_close, assert_identical

RTOL = 1e-9
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    assert _capi.device_count() > 0, "these tests need the GPU"
    return _capi


@pytest.fixture(scope="module")
def synth():
    from optimalbeziertrajectorygeneration_amd import synth
    return synth


# the DEG_ELEV = 0 shapes of test_structured_fd_step_is_bit_identical_to_the_brute_force_sweep: (N, n, M, fixed)
R0_SHAPES = {"C3_full_batch": (64, 10, 8, 1), "deg7_two_fixed": (20, 7, 2, 2), "deg8_two_fixed": (21, 8, 3, 2),
             "three_vehicles": (3, 10, 1, 1), "deg5_no_polys": (12, 5, 0, 1), "one_row": (10, 7, 2, 1),
             "C4_like_large_rows": (256, 15, 0, 1), "rows_of_96KB": (558, 10, 2, 1), "with_point_obstacles": (20, 10, 2, 1),
             "example1_class_path": (2, 10, 1, 2)}
POINT_OBS = {"with_point_obstacles": [[20.0, 30.0], [55.5, 41.0], [70.0, 12.5]], "example1_class_path": [[3.0, 2.0], [6.0, 7.0]]}
ROWS = {"one_row": 1, "C4_like_large_rows": 130, "rows_of_96KB": 24}
KEYS = ("sep", "flag", "p1", "p2", "dist", "ns", "st", "sp", "sp2", "an")


def tf_pattern(tf_rows, B):
    tf = np.linspace(3.0, 9.0, B)
    if tf_rows != "every_row_its_own_tf":
        tf[:] = 6.5
    if tf_rows == "a_few_rows_with_their_own_tf":
        for k in (1, 2, 9, 64, 65, 700, B - 1):
            if 0 < k < B:
                tf[k] = 6.5 + 1e-3 * k
        if B > 12:
            tf[11] = np.nextafter(6.5, 7.0)       # one ulp off is its own tf
    return tf


class Case:
    """A context with its pair list, the view's one row on the device, and buffers for B rows."""

    def __init__(self, capi, synth, N, d, n, R, M, fixed, B=None, pobs=None, seed=41, h=1e-3):
        import torch
        self.torch, self.synth = torch, synth
        self.N, self.d, self.n, self.R, self.M, self.fixed, self.h, self.seed = N, d, n, R, M, fixed, h, seed
        self.Y = synth.swarm_control_points(N, d, n, seed=seed)
        self.n_x = N * d * (n + 1 - 2 * fixed)
        self.B = B if B else self.n_x + 1
        self.ctx = capi.Context(N, d, n, R, point_obs=np.array(pobs) if pobs else None)
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.polys = synth.polygon_obstacles(M, seed=seed) if M else []
        if d == 3:
            self.polys = [np.concatenate([q[:, :2], 3.0 * np.arange(len(q))[:, None]], axis=1) for q in self.polys]
        self.pa, self.pb = synth.swarm_pairs(N, M)
        self.ctx.set_polygons(*(synth.pack_polys(self.polys) if M else (None, [0])))
        self.ctx.set_hull_pairs(self.pa, self.pb)
        self.d0 = torch.from_numpy(self.Y).cuda()
        self.L = 2 * n + R + 1

    def bufs(self, B, want_ang=True):
        torch, ctx = self.torch, self.ctx
        f64, i32, Ps = torch.float64, torch.int32, len(self.pa)

        def nan(*sh):
            return torch.full(sh, float("nan"), dtype=f64, device="cuda")
        return dict(sep=nan(B, ctx.num_pairs * self.L), flag=torch.full((B, Ps), -7, dtype=i32, device="cuda"), p1=nan(B, Ps, 3),
                    p2=nan(B, Ps, 3), dist=nan(B, Ps), ns=torch.full((B, Ps), -7, dtype=i32, device="cuda"),
                    st=torch.full((B, Ps), -7, dtype=i32, device="cuda"), sp=nan(B, ctx.len_speed), sp2=nan(B, ctx.len_speed),
                    an=nan(B, ctx.len_ang_rate) if want_ang else None)

    def sweep(self, src, dtf, B, o, with_ns_st=True):
        """obtg_constraint_sweep_dev with the second speed bound on; returns the launches per kernel name."""
        ctx = self.ctx
        ctx.set_second_speed_bound(0.4, False, o["sp2"].data_ptr())
        ctx.reset_kernel_stats(); ctx.set_profiling(True)
        ctx.constraint_sweep_dev(src, dtf.data_ptr(), B, 0.9, o["sep"].data_ptr(), 4.0, True, 1.5, o["sp"].data_ptr(),
                                 o["an"].data_ptr() if o["an"] is not None else None, o["flag"].data_ptr(), o["p1"].data_ptr(),
                                 o["p2"].data_ptr(), o["dist"].data_ptr(), o["ns"].data_ptr() if with_ns_st else None,
                                 o["st"].data_ptr() if with_ns_st else None, 128, 500)
        self.torch.cuda.synchronize()
        ks = {k: v[1] for k, v in ctx.kernel_stats().items() if v[1]}
        ctx.set_profiling(False)
        ctx.set_second_speed_bound(0.0, False, None)
        return ks

    def in_view(self, dtf, B, o, row_begin=0, **kw):
        self.ctx.fd_view_begin(self.d0.data_ptr(), self.fixed, self.h, B, row_begin=row_begin)
        try:
            return self.sweep(None, dtf, B, o, **kw)
        finally:
            self.ctx.fd_view_end()

    def materialised(self, B):
        """Rows 0 .. B-1 of the view's batch in memory (obtg_fd_batch_dev)."""
        dY = self.torch.empty((B,) + self.Y.shape, dtype=self.torch.float64, device="cuda")
        self.ctx.fd_batch_dev(self.d0.data_ptr(), self.fixed, self.h, B, dY.data_ptr())
        return dY

    def close(self):
        self.ctx.use_own_stream()
        self.ctx.close()


def same_bits(torch, a, b, what, keys=KEYS):
    for key in keys:
        if a[key] is None:
            assert b[key] is None
            continue
        assert torch.equal(a[key].contiguous().view(torch.uint8), b[key].contiguous().view(torch.uint8)), (what, key)


def r0_case(capi, synth, shape, **kw):
    N, n, M, fixed = R0_SHAPES[shape]
    return Case(capi, synth, N, 2, n, 0, M, fixed, B=ROWS.get(shape), pobs=POINT_OBS.get(shape),
                h=synth.FD_STEP if shape == "C3_full_batch" else 1e-3, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(R0_SHAPES))
@pytest.mark.parametrize("tf_rows", ["one_tf", "a_few_rows_with_their_own_tf", "every_row_its_own_tf"])
def test_routed_view_sweep_equals_the_brute_force_sweep_of_the_materialised_batch(capi, synth, shape, tf_rows):
    """Every output array of the routed in-view call -- separation, both speed bounds, angular rate, gjkNew's flag, points,
    distance, support count and status -- equals, bit for bit, the brute-force sweep of the same rows in memory; the in-view
    call is ONE launch booked as pair_sweep and writes no batch."""
    import torch
    c = r0_case(capi, synth, shape)
    B = c.B
    dtf = torch.from_numpy(tf_pattern(tf_rows, B)).cuda()
    ref, got = c.bufs(B), c.bufs(B)
    dY = c.materialised(B)
    c.sweep(dY.data_ptr(), dtf, B, ref)
    del dY
    ks = c.in_view(dtf, B, got)
    assert ks == {"pair_sweep": 1}, ks
    same_bits(torch, ref, got, (shape, tf_rows))
    # d_nsup / d_status are optional: without them the other arrays are the same
    got2 = c.bufs(B)
    ks = c.in_view(dtf, B, got2, with_ns_st=False)
    assert ks == {"pair_sweep": 1}, ks
    same_bits(torch, ref, got2, (shape, tf_rows, "no ns/st"), keys=[k for k in KEYS if k not in ("ns", "st")])
    assert (got2["ns"] == -7).all() and (got2["st"] == -7).all()
    c.close()


@pytest.mark.gpu
def test_switch_off_env_off_and_switch_on_give_the_same_bits(capi, synth, monkeypatch):
    """obtg_ctx_set_fd_view_structured(0), a context created under OBTG_FD_VIEW_STRUCTURED=0, and the default: one launch
    each, the same bits, equal to the materialised brute-force sweep; the switch turns an env-off context back on."""
    import torch
    shape = "deg8_two_fixed"
    c = r0_case(capi, synth, shape)
    B = c.B
    dtf = torch.from_numpy(tf_pattern("a_few_rows_with_their_own_tf", B)).cuda()
    ref = c.bufs(B)
    dY = c.materialised(B)
    c.sweep(dY.data_ptr(), dtf, B, ref)
    outs = {}
    outs["on"] = c.bufs(B)
    assert c.in_view(dtf, B, outs["on"]) == {"pair_sweep": 1}
    c.ctx.set_fd_view_structured(False)
    outs["off"] = c.bufs(B)
    assert c.in_view(dtf, B, outs["off"]) == {"pair_sweep": 1}
    c.ctx.set_fd_view_structured(True)
    outs["on_again"] = c.bufs(B)
    assert c.in_view(dtf, B, outs["on_again"]) == {"pair_sweep": 1}
    monkeypatch.setenv("OBTG_FD_VIEW_STRUCTURED", "0")
    e = r0_case(capi, synth, shape)
    monkeypatch.delenv("OBTG_FD_VIEW_STRUCTURED")
    outs["env_off"] = e.bufs(B)
    assert e.in_view(dtf, B, outs["env_off"]) == {"pair_sweep": 1}
    e.ctx.set_fd_view_structured(True)
    outs["env_off_then_on"] = e.bufs(B)
    assert e.in_view(dtf, B, outs["env_off_then_on"]) == {"pair_sweep": 1}
    for name, o in outs.items():
        same_bits(torch, ref, o, name)
    e.close()
    c.close()


FALL_THROUGH = {   # (N, d, n, R, M, fixed, B): shapes the router leaves to the brute-force launches
    "space3d": (9, 3, 5, 0, 2, 1, 40), "space3d_many": (36, 3, 5, 0, 2, 1, 25), "elevated": (40, 2, 10, 12, 2, 1, 7),
    "fd_dedup_on": (20, 2, 10, 0, 2, 1, 30), "ang_exact_elevated": (12, 2, 10, 7, 2, 1, 20), "no_ang_output": (20, 2, 10, 0, 2, 1, 30),
    "degree_20": (6, 2, 20, 0, 1, 1, 15)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(FALL_THROUGH))
def test_shapes_outside_the_structured_step_fall_through_unchanged(capi, synth, shape):
    """3-D rows, DEG_ELEV > 0, de-duplication on, ang_rate_order exact with DEG_ELEV > 0, no angular-rate output, degree 20:
    the in-view call returns OK with the routing on, launches exactly what it launches with the routing off (the
    brute-force path: nothing spent on a refused structured launch), and gives the bits of the materialised sweep."""
    import torch
    N, d, n, R, M, fixed, B = FALL_THROUGH[shape]
    c = Case(capi, synth, N, d, n, R, M, fixed, B=B, seed=23)
    if shape == "fd_dedup_on":
        c.ctx.set_fd_dedup(True)
    if shape == "ang_exact_elevated":
        c.ctx.set_ang_rate_order(2)
    want_ang = d == 2 and shape != "no_ang_output"
    dtf = torch.from_numpy(tf_pattern("a_few_rows_with_their_own_tf", B)).cuda()
    ref, on, off = c.bufs(B, want_ang), c.bufs(B, want_ang), c.bufs(B, want_ang)
    dY = c.materialised(B)
    c.sweep(dY.data_ptr(), dtf, B, ref)
    c.ctx.set_fd_view_structured(False)
    ks_off = c.in_view(dtf, B, off)
    c.ctx.set_fd_view_structured(True)
    ks_on = c.in_view(dtf, B, on)
    assert ks_on == ks_off, (ks_on, ks_off)
    if shape == "elevated":      # gjkNew sweep + (separation rows with the dynamics groups among them)
        assert ks_on.get("gjk") == 1 and ks_on.get("temporal_sep") == 1 and "pair_sweep" not in ks_on, ks_on
    same_bits(torch, ref, off, (shape, "off"))
    same_bits(torch, ref, on, (shape, "on"))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["C3_full_batch", "deg7_two_fixed", "C4_like_large_rows"])
def test_routed_row_range_views_equal_the_rows_of_the_materialised_batch(capi, synth, shape):
    """obtg_fd_view_begin_rows: ranges with and without the batch's row 0, one launch each, against the same rows of the
    brute-force sweep of the full materialised batch."""
    import torch
    c = r0_case(capi, synth, shape)
    B = min(c.B, 300)
    tf = tf_pattern("a_few_rows_with_their_own_tf", B)
    dtf = torch.from_numpy(tf).cuda()
    ref = c.bufs(B)
    dY = c.materialised(B)
    c.sweep(dY.data_ptr(), dtf, B, ref)
    del dY
    for r0, cnt in ((0, 3), (0, B), (1, 1), (B // 3, B - B // 3), (B - 2, 2), (5, min(64, B - 5))):
        got = c.bufs(cnt)
        ks = c.in_view(dtf[r0:r0 + cnt].contiguous(), cnt, got, row_begin=r0)
        assert ks == {"pair_sweep": 1}, (r0, cnt, ks)
        same_bits(torch, {k: v[r0:r0 + cnt] for k, v in ref.items()}, got, (shape, r0, cnt))
    c.close()


@pytest.mark.gpu
def test_brute_force_sweep_after_routed_calls_equals_a_fresh_context(capi, synth):
    """The sweep's trip-count history after routed calls: a brute-force sweep of a batch of the caller's gives the bits it
    gives on a context that never ran anything else."""
    import torch
    a, b = r0_case(capi, synth, "C3_full_batch"), r0_case(capi, synth, "C3_full_batch")
    B = 200
    dtf = torch.from_numpy(tf_pattern("one_tf", B)).cuda()
    scratch = a.bufs(B)
    for _ in range(3):
        assert a.in_view(dtf, B, scratch) == {"pair_sweep": 1}
    dY = a.materialised(B)
    dY[B // 2] += 0.25 * torch.randn_like(dY[B // 2])       # a batch that is no view's: one genuinely different row
    after, fresh = a.bufs(B), b.bufs(B)
    a.sweep(dY.data_ptr(), dtf, B, after)
    b.sweep(dY.data_ptr(), dtf, B, fresh)
    same_bits(torch, fresh, after, "brute force after routed calls")
    again = a.bufs(B)
    assert a.in_view(dtf, B, again) == {"pair_sweep": 1}
    same_bits(torch, scratch, again, "routed call after a brute-force sweep")
    a.close()
    b.close()


@pytest.mark.gpu
def test_routed_c3_step_against_the_oracle_on_sampled_rows(capi, synth, oracle):
    """C3, B = n_x + 1 = 1153: the routed call's own buffers against the CPU oracle on rows 0, 1, the last row and one row
    per residue mod 8 (consecutive rows go to the 8 XCDs round-robin)."""
    import torch
    c = r0_case(capi, synth, "C3_full_batch")
    B = c.B
    assert B == 1153
    tf = tf_pattern("one_tf", B)
    dtf = torch.from_numpy(tf).cuda()
    got = c.bufs(B)
    assert c.in_view(dtf, B, got) == {"pair_sweep": 1}
    rows = sorted(set([0, 1, B - 1] + [min(B - 1, (k * (B - 1)) // 9 // 8 * 8 + k % 8) for k in range(1, 9)]))
    assert {r % 8 for r in rows} == set(range(8))
    ncol = c.n + 1 - 2 * c.fixed
    for r in rows:
        Yr = c.Y.copy()
        if r:
            rr, cc = divmod(r - 1, ncol)
            Yr[rr, c.fixed + cc] = c.Y[rr, c.fixed + cc] + c.h            # the view's row r: x + h e_r
        o_sep, o_sp, o_an = oracle.eval_batch(Yr[None], float(tf[r]), c.N, 2, 0, 0.9, 4.0, 1.5, nthreads=8)
        assert_close(got["sep"][r].cpu().numpy(), o_sep[0], RTOL, "routed step, separation rows of batch row %d vs oracle" % r)
        assert_close(got["sp"][r].cpu().numpy(), o_sp[0], RTOL, "routed step, speed rows of batch row %d" % r)
        assert_close(got["sp2"][r].cpu().numpy(), (4.0 ** 2 - o_sp[0]) - 0.4 ** 2, 1e-9, "routed step, second speed bound of batch row %d" % r)
        assert_close(got["an"][r].cpu().numpy(), o_an[0], RTOL, "routed step, angular rate of batch row %d" % r)
        hp, ho = synth.pack_polys(synth.hulls_from_Y(Yr, 2) + c.polys)
        og = oracle.gjk_pairs(hp, ho, c.pa, c.pb, md_cap=500)
        assert (got["flag"][r].cpu().numpy() == og["flag"]).all() and (got["ns"][r].cpu().numpy() == og["n_support"]).all(), r
        sepd = og["flag"] == 1
        assert_identical(got["dist"][r].cpu().numpy()[sepd], og["dist"][sepd], "routed step, row %d dist" % r)
    c.close()


# ---- which kernels every sweep entry point launches, per branch of the pair sweep's plan (gjk_kernels.hip pair_sweep_plan)
# name: (N, d, n, R, M, point obstacles, option, row counts); the one polygon of seed 21 has 5 vertices: no more than n + 1
ROUTING_CASES = {
    "planar_16x5": (16, 2, 5, 0, 1, None, None, (1, 9)),                           # one-launch planar
    "planar_16x5_point_obstacles": (16, 2, 5, 0, 1, [[20.0, 30.0], [55.5, 41.0]], None, (1, 9)),
    "elevated_16x5": (16, 2, 5, 3, 1, None, None, (1, 9)),                         # DEG_ELEV > 0
    "dedup_16x5": (16, 2, 5, 0, 1, None, "dedup", (1, 9)),
    "history_off_16x5": (16, 2, 5, 0, 1, None, "history_off", (1, 9)),
    "tiled_256x15": (256, 2, 15, 0, 0, None, None, (1,)),                          # rows beyond 48 KB: the tiled form
    "tiled_partial_603x5": (603, 2, 5, 0, 1, None, "partial", (1, 9)),             # ... whose tiles cannot carry the separation rows
    "tiled_duplicates_603x5": (603, 2, 5, 0, 1, None, "duplicates", (1, 9)),       # ... a tile cut into two chunks
    "space3d_9x5": (9, 3, 5, 0, 1, None, None, (1, 9)),
    "degree12_6": (6, 2, 12, 0, 1, None, None, (1, 9)),                            # no fixed-count kernel
}
ROUTING_OPS = ("gjk_swarm_batch", "pair_sweep_batch", "pair_sweep_view", "constraint_sweep_batch",
               "constraint_sweep_view_structured_on", "constraint_sweep_view_structured_off")


def routing_case(capi, synth, name):
    """{"fly": fd_forms_on_the_fly(), "B<rows>": {operation: {kernel name: launches}}} of one ROUTING_CASES entry."""
    import torch
    N, d, n, R, M, pobs, option, row_counts = ROUTING_CASES[name]
    c = Case(capi, synth, N, d, n, R, M, 1, B=max(row_counts), pobs=pobs, seed=21)
    if option == "partial":          # (test_pair_sweep_one_launch_equals_separate_kernels' lists)
        keep = np.random.default_rng(5).random(len(c.pa)) < 0.7
        c.pa, c.pb = c.pa[keep], c.pb[keep]
    if option == "duplicates":
        c.pa, c.pb = np.concatenate([c.pa, c.pa[:4000]]), np.concatenate([c.pb, c.pb[:4000]])
    if option in ("partial", "duplicates"):
        c.ctx.set_hull_pairs(c.pa, c.pb)
    if option == "dedup":
        c.ctx.set_fd_dedup(True)
    if option == "history_off":
        c.ctx.set_gjk_history(False)
    ctx, want_ang = c.ctx, d == 2

    def launches(call):
        ctx.reset_kernel_stats(); ctx.set_profiling(True)
        call()
        torch.cuda.synchronize()
        ks = {k: v[1] for k, v in ctx.kernel_stats().items() if v[1]}
        ctx.set_profiling(False)
        return ks

    def in_view(B, call):
        ctx.fd_view_begin(c.d0.data_ptr(), c.fixed, c.h, B)
        try:
            return call()
        finally:
            ctx.fd_view_end()

    out = {"fly": list(ctx.fd_forms_on_the_fly())}
    for B in row_counts:
        o = c.bufs(B, want_ang)
        dY = c.materialised(B)
        dtf = torch.from_numpy(tf_pattern("one_tf", B)).cuda()
        gjk = (o["flag"].data_ptr(), o["p1"].data_ptr(), o["p2"].data_ptr(), o["dist"].data_ptr(), o["ns"].data_ptr(), o["st"].data_ptr(), 128, 500)
        t = {}
        t["gjk_swarm_batch"] = launches(lambda: ctx.gjk_swarm_dev(dY.data_ptr(), B, *gjk))
        t["pair_sweep_batch"] = launches(lambda: ctx.pair_sweep_dev(dY.data_ptr(), B, 0.9, o["sep"].data_ptr(), *gjk))
        t["pair_sweep_view"] = in_view(B, lambda: launches(lambda: ctx.pair_sweep_dev(None, B, 0.9, o["sep"].data_ptr(), *gjk)))
        t["constraint_sweep_batch"] = c.sweep(dY.data_ptr(), dtf, B, o)
        t["constraint_sweep_view_structured_on"] = c.in_view(dtf, B, o)
        ctx.set_fd_view_structured(False)
        t["constraint_sweep_view_structured_off"] = c.in_view(dtf, B, o)
        ctx.set_fd_view_structured(True)
        out["B%d" % B] = t
        del o, dY
    c.close()
    return out


# The answers of the library BEFORE the pair sweep's plan (commit ca17e6b: the three hand-written copies of the routing),
# not of the tree under test.  NOT RECORDED: no GPU could be had when this was written, so the table is a reading of that
# commit's source (launch_gjk_swarm, launch_pair_sweep, launch_dynamics, launch_sep_dynamics_elev, with_batch), the way
# test_bernstein_host_return_codes' table was made; a launch counts once per ScopedKernelTimer.  Every case answers the same
# for every row count it runs.
_P, _G, _GT = {"pair_sweep": 1}, {"gjk": 1}, {"gjk": 1, "temporal_sep": 1}
_GTA = {"gjk": 1, "temporal_sep": 1, "ang_rate": 1}


def _ops(gjk, pair, pair_view, sweep, sweep_view):
    return dict(zip(ROUTING_OPS, (gjk, pair, pair_view, sweep, sweep_view, sweep_view)))


_ROUTING_BY_CASE = {
    # one launch everywhere; the view's one-call sweep is the structured step or, switched off, the folded pair sweep
    "planar_16x5": ([True, True], _ops(_G, _P, _P, _P, _P)),
    "planar_16x5_point_obstacles": ([True, True], _ops(_G, _P, _P, _P, _P)),
    "history_off_16x5": ([True, True], _ops(_G, _P, _P, _P, _P)),
    # DEG_ELEV > 0: gjkNew sweep + separation rows; 120 pairs are two 64-pair groups, too few for k_sep_dynamics_elev, so
    # the dynamics are k_dynamics_elev's launch
    "elevated_16x5": ([False, True], _ops(_G, _GT, _GT, _GTA, _GTA)),
    # de-duplication compares rows in memory: a view is materialised first
    "dedup_16x5": ([False, True], _ops(_G, _GT, dict(_GT, fd_batch=1), _GTA, dict(_GTA, fd_batch=1))),
    "tiled_256x15": ([False, True], _ops(_G, _P, _P, _P, _P)),
    # the tiles cannot carry the separation rows: tiled gjkNew sweep + separation rows + dynamics
    "tiled_partial_603x5": ([False, True], _ops(_G, _GT, _GT, _GTA, _GTA)),
    "tiled_duplicates_603x5": ([False, True], _ops(_G, _GT, _GT, _GTA, _GTA)),
    # 3-D: the sweep folds the separation rows; with a second speed bound set the two speed launches stay separate
    "space3d_9x5": ([False, False], _ops(_G, _P, _P, {"pair_sweep": 1, "speed": 2}, {"pair_sweep": 1, "speed": 2})),
    # any-degree kernels read their rows from memory
    "degree12_6": ([False, False], _ops(_G, _GT, dict(_GT, fd_batch=1), {"gjk": 1, "temporal_sep": 1, "speed": 2, "ang_rate": 1},
                                        {"gjk": 1, "temporal_sep": 1, "speed": 2, "ang_rate": 1, "fd_batch": 1})),
}
ROUTING_EXPECTED = {name: dict({"fly": fly}, **{"B%d" % B: ops for B in ROUTING_CASES[name][7]})
                    for name, (fly, ops) in _ROUTING_BY_CASE.items()}


@pytest.mark.gpu
def test_sweep_routing_table(capi, synth):
    """What must not move when the launch side of the sweeps is rearranged: per plan branch (one-launch planar, with point
    obstacles, DEG_ELEV > 0, de-duplication, history off, tiled, tiled with a partial / a duplicated pair list, 3-D, a degree
    without a fixed-count kernel) and row count, the launches per kernel name of obtg_gjk_swarm_dev, obtg_pair_sweep_dev (batch
    and view) and obtg_constraint_sweep_dev (batch, view with the structured switch on and off), and obtg_fd_forms_on_the_fly."""
    assert sorted(ROUTING_EXPECTED) == sorted(ROUTING_CASES)
    for name in sorted(ROUTING_CASES):
        got = routing_case(capi, synth, name)
        want = ROUTING_EXPECTED[name]
        assert sorted(got) == sorted(want), name
        assert got["fly"] == want["fly"], (name, "fd_forms_on_the_fly", got["fly"], want["fly"])
        for rows in (k for k in sorted(want) if k != "fly"):
            assert sorted(got[rows]) == sorted(ROUTING_OPS)
            for op in ROUTING_OPS:
                assert got[rows][op] == want[rows][op], (name, rows, op, got[rows][op], want[rows][op])


def test_header_export_list_and_binding_table_agree_on_the_switch():
    """obtg_ctx_set_fd_view_structured is declared in include/obtg.h, exported by the library, named by obtg_abi_symbols
    and bound in _capi.py with a wrapper on Context; a new symbol alone does not move the ABI revision.  No GPU needed."""
    import ctypes as C
    from optimalbeziertrajectorygeneration_amd import _capi, build
    name = "obtg_ctx_set_fd_view_structured"
    header = open(os.path.join(REPO, "include", "obtg.h")).read()
    assert re.search(r"^int %s\(obtg_ctx\*, int on\);" % name, header, re.M)
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
    assert hasattr(lib, name) and name in syms and name in _capi.abi_symbol_names()
    assert sorted(syms) == _capi.abi_symbol_names()        # the two tables name the same symbols
    assert all(re.search(r"\b%s\(" % s, header) for s in syms)
    assert hasattr(_capi.Context, "set_fd_view_structured")
    lib.obtg_abi_version.restype = C.c_int
    assert lib.obtg_abi_version() == 7
