"""The constraint rows SLSQP evaluates on every iteration -- obtg_temporal_sep, obtg_speed, obtg_ang_rate, their reduced and
fused forms -- against exact rationals, in every launch form: each assertion is the element-wise forward bound
|device - exact| <= K * 2^-53 * M of tests/constraint_rows_ref.py (the angular rate: its quotient test), which
tests/test_constraint_rows_ref.py holds honest on the CPU.  Every element of every row is checked; B <= 3 rows per case.
Each test prints the largest share of the bound the device used, per form (pytest -s).

Which form a case reaches, and by which line (bern_kernels.hip unless named; the arithmetic is restated in
constraint_rows_ref.sep_form / speed_form / ang_form, and test_constraint_rows_ref.py asserts it of every case below):

  separation, R = 0 (launch_temporal_sep -> plan_temporal_sep -> dispatch_ns<0, false> -> launch_ns_t -> k_normsq_elev<.., false, false>)
    pairs 63 | 64 | 65         1 | 1 | 2 waves                 plan_temporal_sep `p.waves = groups_total >= 4 ? 4 : groups_total`
    pairs 255 | 256 | 257      4 waves, 1 | 1 | 2 workgroups   `while (gpw > p.waves && B * ... < 4096) gpw >>= 1`, `p.wgs_per_row = ...`
    64-row tile                N = 12, deg 10                  launch_ns_t `for (tr = kWave; tr >= 16; tr >>= 1)` stops at 64
    N = 20, deg 20             64-row tile as well: 190 pairs are 3 groups, 3 waves x 64 x 41 doubles + 20 objects = 68 KB <= 76 KB
    32-row tile                N = 21, deg 20 (4 waves: 64 rows would need 89 KB)           the same loop stops at 32
    N = 100, deg 20            32-row tile: 34 KB of objects + 41 KB = 74.6 KB <= 76 KB
    16-row tile                N = 110, deg 20 (37 KB of objects + 41 KB > 76 KB)           the same loop stops at 16
    slot staging               N = 300, deg 3, pairs [250, 1750)   `p.stage_all = c->n_obj <= slots ? 1 : 0` -> 0; the others: 1
    tiled                      N = 140, deg 10                 `if (row_bytes <= 24 * 1024 || c->n_obj <= 2 * kWave)` false: row-window tiles
    nc in OBTG_NC_SEP x {2, 3}-D with point obstacles          dispatch_ns `OBTG_NC_SEP(OBTG_CASE_D)`; stage_objects `obs[(obj - n_veh) * DIM + ..]`
  separation, R > 0 (launch_ns_t `if (const size_t lc = sep_elev_coop_lds<NC, DIM>(p)) kern = k_sep_elev_coop`)
    R = 1; L + R = 16 | 17; 128     k_sep_elev_coop (sep_elev_coop_lds: staged whole, L + R <= 64 * kCoopNTW = 128)
    L + R = 129                k_normsq_elev<.., false, true> -> elev_rows_mfma        `LR > 64 * kCoopNTW` -> 0
    elevated, slot staging | tiled  k_normsq_elev<.., false, true>                     `!p.stage_all || p.tiling` -> 0
    R = 512 | 513              k_normsq_elev<ELEV> | k_generic_normsq_elev<0>          fast_shape `c->R <= 512`
    every L = 2 deg + 1 is odd: the last MFMA k-step of elev_table_frag is zero padded in every elevated case
  separation, any degree (launch_temporal_sep -> launch_generic_rows<0> -> k_generic_normsq_elev<0>)
    dim 1; deg 2, 12, 31       fast_shape `nc_in_sep(nc) && (dim == 2 || dim == 3)` false
    2 n + R + 1 = 1024         n = 2, R = 1019: launch_generic_rows `2 * c->deg + R + 1 > kMaxGenericLen` not yet
  reduced and fused forms
    temporal_sep_min[_range]   dispatch_ns<0, true>: k_normsq_elev<.., true, ELEV> (elev_at per column when R > 0); any degree: min_only of the tail
    temporal_sep_active        the same kernels' Smallest4 epilogue (`p.sel_k > 0`); any degree: launch_temporal_sep `k_select_smallest`
    temporal_sep_fd            launch_temporal_sep_fd -> k_tsep_fd
    one_vs_many_min[_spans]    launch_one_vs_many_min[_spans] -> k_one_vs_many | k_one_vs_many_spans (equal spans: no cut)
  speed (launch_speed -> dispatch_ns<1, false> -> k_normsq_elev<NC, DIM, 1, false, ELEV> | launch_generic_rows<1>)
    N = 1, 64, 65; every nc x {2, 3}-D; R = 1, 100, 512 | 513, dim 1, deg 12, 31; both signs; tf = 7.3, 0.013, 1 per row
    dynamics_dev, speed only   launch_dynamics -> launch_dyn_t `k_dynamics<NC>` (p.out == nullptr), every nc of OBTG_NC_DYN
    dynamics_dev, both + the second bound   launch_dyn_t `k_dynamics2<NC>`; R > 0: launch_dyn_elev_t `k_dynamics_elev<NC>`; second_speed_rows
  angular rate (launch_ang_rate; obtg_ctx_ang_rate_order_in_effect asserted per case)
    nc in OBTG_NC_DYN, N = 65  dyn_fast -> k_dynamics2                                          order 0
    R = 1, 12, 100, 4 R = 1000 (deg 15)   dyn_fast_elev -> k_dynamics_elev                      order 0
    order 2                    k_dynamics_elev, then ang_exact_finish -> k_angrate_dd           order 2
    order 1; deg 16, R = 3     k_generic_angrate (`c->ang_elevate_first`; nc_in_dyn and deg <= 15 only) order 1
    m = 6, 7, 127 | 2 (deg 2), 128, 250   k_generic_angrate balanced | plain schedule: angrate_balanced(m) and angrate_balanced2(m)
                               are the same predicate for every m (both count floor(m / 2) + 1 tiles), so two of the four
                               combinations exist; m = 250 is launch_ang_rate's `m > 250` limit
    a vehicle at rest; nearstop.npz in all three orders

Measured on MI355X, largest share of the bound (every figure <= 1 is a pass): see DESIGN.md 4.5a.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_rows_ref as C  # noqa: E402

pytestmark = pytest.mark.gpu

MS = C.SEP_MAX_SEP


@pytest.fixture(scope="module")
def capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    assert _capi.device_count() > 0, "these tests need the GPU"
    return _capi


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Shares(object):
    """Every comparison of one test: all are made, the largest share of the bound is printed per form, then the failures raise."""

    def __init__(self, title):
        self.title, self.worst, self.n, self.failed = title, {}, 0, []

    def hold(self, form, cand, ref, what):
        self.n += 1
        fn = C.ang_assert_within if isinstance(ref, C.AngRef) else C.assert_within
        try:
            self.worst[form] = max(self.worst.get(form, 0.0), fn(cand, ref, "%s %s" % (form, what)))
        except AssertionError as e:
            self.worst[form] = math.inf
            self.failed.append(str(e))

    def same(self, got, want, what):
        self.n += 1
        if not np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True):
            self.failed.append("%s: not bit for bit" % what)

    def true(self, cond, what):
        self.n += 1
        if not cond:
            self.failed.append(what)

    def done(self):
        print("\n%s: largest share of the bound used by the device (%d comparisons)" % (self.title, self.n))
        for form in sorted(self.worst):
            print("  %-64s %.3f" % (form, self.worst[form]))
        assert not self.failed, "%d of %d comparisons failed:\n%s" % (len(self.failed), self.n, "\n".join(self.failed[:20]))


def _form_name(f):
    if "generic" in f["kernel"]:
        return f["kernel"]
    return "%s, %d waves, %s%s" % (f["kernel"], f["waves"], f["staging"], ", %d-row tile" % f["tile_rows"] if f["kernel"] == "k_normsq_elev" else "")


def _dev_rows(torch, ctx, Yb, rng):
    """obtg_temporal_sep_dev on pairs [begin, begin + count)"""
    B = Yb.shape[0]
    L = ctx.len_temporal_sep // ctx.num_pairs
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dY = torch.from_numpy(np.ascontiguousarray(Yb)).cuda()
    out = torch.full((B, rng[1] * L), float("nan"), dtype=torch.float64, device="cuda")
    ctx.temporal_sep_dev(dY.data_ptr(), B, MS, out.data_ptr(), rng[0], rng[1])
    torch.cuda.synchronize()
    ctx.use_own_stream()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
#  separation, full rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.SEP_CASES, ids=[c[0] for c in C.SEP_CASES])
def test_separation_rows(capi, torch, case):
    name, N, d, n, R, M, kind, B, rng, want = case
    f = C.sep_form(N + M, d, n, R, B, *(rng or (0, None)))
    assert all(f[k] == v for k, v in want.items()), (f, want)
    sh = Shares("separation, %s" % name)
    Yb = C.rows_batch(100 + n + R, B, N, d, n, kind)
    obs = C.point_obstacles(7, M, d) if M else None
    ctx = capi.Context(N, d, n, R, point_obs=obs)
    try:
        pairs = C.all_pairs(N + M)
        L = 2 * n + R + 1
        if rng is None:
            got = ctx.temporal_sep(Yb, MS).reshape(B, len(pairs), L)
        else:
            got = _dev_rows(torch, ctx, Yb, rng).reshape(B, rng[1], L)
            pairs = pairs[rng[0]:rng[0] + rng[1]]
    finally:
        ctx.close()
    for b in range(B):
        ref = C.temporal_sep(Yb[b], N, d, R, MS, obs, pairs)
        sh.hold(_form_name(f), got[b], ref, "row %d" % b)
        if kind == "edges" and rng is None:
            # vehicles 0, 1 exactly max_sep apart (2-D: a row of zeros), vehicles 2, 3 coincident (-max_sep^2 in every column)
            i01, i23 = pairs.index((0, 1)), pairs.index((2, 3))
            sh.same(got[b, i23], np.full(L, -C.square(MS)), "row %d: coincident vehicles" % b)
            if d == 2:
                zero = np.abs(got[b, i01]).max()
                print("\n%s row %d: the pair exactly max_sep apart, largest |value| %.3g (exact: 0)" % (name, b, zero))
    sh.done()


def test_separation_longest_generic_row_just_inside_the_finiteness_condition(capi):
    """2 n + R + 1 = 1024 (n = 2, R = 1019) with the differences scaled so that the largest unnormalised sum of
    generic_normsq_elev_tail lies in [DBL_MAX / 8, DBL_MAX / 2): finite and within the bound -- the condition include/obtg.h states"""
    Y, peak = C.longest_row_case()
    sh = Shares("separation, 1024 coefficients")
    ctx = capi.Context(2, 2, 2, 1019)
    try:
        got = ctx.temporal_sep(Y, MS).reshape(1, 1024)
        mn = ctx.temporal_sep_min(Y, MS)
    finally:
        ctx.close()
    assert np.isfinite(got).all()
    ref = C.temporal_sep(Y, 2, 2, 1019, MS)
    sh.hold("k_generic_normsq_elev, 1024 coefficients", got, ref, "rows")
    sh.true(C.min_within(mn, ref), "temporal_sep_min of the longest row")
    sh.done()


# ---------------------------------------------------------------------------------------------------------------------
#  separation, reduced and fused forms
# ---------------------------------------------------------------------------------------------------------------------
REDUCED = [("nc 11, R = 0", 12, 2, 10, 0, 1), ("nc 6, R = 6", 9, 2, 5, 6, 0), ("nc 21, R = 30, 3-D", 6, 3, 20, 30, 1),
           ("any degree: deg 12, R = 7", 5, 3, 12, 7, 1), ("any degree: deg 2", 6, 2, 2, 0, 0)]


@pytest.mark.parametrize("case", REDUCED, ids=[c[0] for c in REDUCED])
def test_separation_min_and_active(capi, case):
    """temporal_sep_min to the bound (and, as its kernels do, equal to the minimum of the full rows' values), temporal_sep_active
    (k = 1..4, with indices) bit for bit the entries of obtg_temporal_sep, as include/obtg.h promises"""
    name, N, d, n, R, M = case
    B = 2
    sh = Shares("separation minima, %s" % name)
    Yb = C.rows_batch(200 + n + R, B, N, d, n, "edges")
    obs = C.point_obstacles(8, M, d) if M else None
    ctx = capi.Context(N, d, n, R, point_obs=obs)
    try:
        P = ctx.num_pairs
        L = 2 * n + R + 1
        full = ctx.temporal_sep(Yb, MS).reshape(B, P, L)
        mn = ctx.temporal_sep_min(Yb, MS)
        begin, count = P // 3 + 1, P // 2
        mr = ctx.temporal_sep_min(Yb, MS, begin, count)
        act = {k: ctx.temporal_sep_active(Yb, MS, k, True) for k in (1, 2, 3, 4)}
    finally:
        ctx.close()
    for b in range(B):
        ref = C.temporal_sep(Yb[b], N, d, R, MS, obs)
        sh.hold("full rows", full[b], ref, "row %d" % b)
        sh.true(C.min_within(mn[b], ref), "row %d: temporal_sep_min outside the bound" % b)
        sh.same(mn[b], full[b].min(axis=1), "row %d: temporal_sep_min against the minimum of the full rows" % b)
        sh.same(mr[b], mn[b, begin:begin + count], "row %d: temporal_sep_min_range from pair %d" % (b, begin))
        order = np.argsort(full[b], axis=1, kind="stable")
        for k, (val, idx) in act.items():
            want_idx = np.sort(order[:, :k], axis=1)
            sh.same(idx[b].reshape(P, k), want_idx, "row %d: active k = %d, indices" % (b, k))
            sh.same(val[b].reshape(P, k), np.take_along_axis(full[b], want_idx, axis=1), "row %d: active k = %d, values" % (b, k))
    sh.done()


def test_separation_min_range_from_the_middle_of_a_group(capi):
    """pairs [70, 70 + 131) of 276: the range starts inside a 64-pair group of the whole launch and ends inside another"""
    N, d, n = 24, 2, 5
    sh = Shares("temporal_sep_min_range")
    Yb = C.rows_batch(300, 3, N, d, n)
    for R in (0, 3):
        ctx = capi.Context(N, d, n, R)
        try:
            mr = ctx.temporal_sep_min(Yb, MS, 70, 131)
        finally:
            ctx.close()
        pairs = C.all_pairs(N)[70:201]
        for b in range(3):
            sh.true(C.min_within(mr[b], C.temporal_sep(Yb[b], N, d, R, MS, None, pairs)), "R = %d row %d outside the bound" % (R, b))
    sh.done()


@pytest.mark.parametrize("R", [0, 6])
def test_separation_fd_blocks(capi, R):
    """obtg_temporal_sep_fd: block t = the pairs of the perturbed vehicle under perturbation t, bit for bit the entries of
    obtg_temporal_sep on the fully perturbed row (include/obtg.h), and within the bound of that row's exact values"""
    N, d, n, M = 7, 2, 5, 2
    sh = Shares("temporal_sep_fd, R = %d" % R)
    Y0 = C.swarm(400, N, d, n, "edges")
    obs = C.point_obstacles(9, M, d)
    perts = [(0, 1, 0.125), (3, n, -2.5), (2 * (N - 1) + 1, 0, 1e-7), (5, 2, 3.0)]        # (row of Y0, column, new value)
    ctx = capi.Context(N, d, n, R, point_obs=obs)
    try:
        blk = ctx.temporal_sep_fd(Y0, [p[0] for p in perts], [p[1] for p in perts], [p[2] for p in perts], MS)
        rows = []
        for r, c, v in perts:
            Yp = Y0.copy()
            Yp[r, c] = v
            rows.append(Yp)
        full = ctx.temporal_sep(np.stack(rows), MS).reshape(len(perts), -1, 2 * n + R + 1)
    finally:
        ctx.close()
    pairs = C.all_pairs(N + M)
    for t, (r, c, v) in enumerate(perts):
        veh = r // d
        mine = [(min(veh, u), max(veh, u)) for u in range(N + M) if u != veh]
        sh.same(blk[t], full[t][[pairs.index(p) for p in mine]], "perturbation %d against the full row" % t)
        sh.hold("k_tsep_fd", blk[t], C.temporal_sep(rows[t], N, d, R, MS, obs, mine), "perturbation %d" % t)
    sh.done()


@pytest.mark.parametrize("d,n,R", [(2, 5, 0), (3, 3, 10), (2, 10, 10)])
def test_one_vs_many(capi, d, n, R):
    """one_vs_many_min within the bound of the pairs (one_b, many_k); one_vs_many_min_spans on equal spans bit for bit the same"""
    B, K = 3, 70
    sh = Shares("one_vs_many_min, %d-D deg %d R = %d" % (d, n, R))
    many = C.swarm(500, K, d, n).reshape(K, d, n + 1)
    one = C.swarm(501, B, d, n, "offset" if d == 3 else "full").reshape(B, d, n + 1)
    if d == 3:
        many = many + 1e6
    ctx = capi.Context(1, d, n, R)
    try:
        got = ctx.one_vs_many_min(one, many, MS)
        sp = ctx.one_vs_many_min_spans(one, np.tile([0.5, 4.0], (B, 1)), many, np.tile([0.5, 4.0], (K, 1)), MS)
    finally:
        ctx.close()
    sh.same(sp, got, "equal spans")
    for b in range(B):
        Y = np.concatenate([one[b].reshape(d, -1), many.reshape(K * d, -1)])
        ref = C.temporal_sep(Y, K + 1, d, R, MS, None, [(0, k + 1) for k in range(K)])
        sh.true(C.min_within(got[b], ref), "candidate %d outside the bound" % b)
    sh.done()


# ---------------------------------------------------------------------------------------------------------------------
#  speed
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.SPEED_CASES, ids=[c[0] for c in C.SPEED_CASES])
def test_speed_rows(capi, case):
    name, N, d, n, R, kind, form = case
    B = len(C.SPEED_TF)
    tf = np.array(C.SPEED_TF)
    sh = Shares("speed, %s" % name)
    Yb = C.rows_batch(600 + n + R, B, N, d, n, kind)
    ctx = capi.Context(N, d, n, R)
    try:
        got = {im: ctx.speed(Yb, tf, bound, im).reshape(B, N, -1) for im, bound in ((1, C.SPEED_BOUNDS[0]), (0, C.SPEED_BOUNDS[1]))}
    finally:
        ctx.close()
    for im, bound in ((1, C.SPEED_BOUNDS[0]), (0, C.SPEED_BOUNDS[1])):
        for b in range(B):
            sh.hold("%s, is_max %d" % (form, im), got[im][b], C.speed(Yb[b], N, d, R, tf[b], bound, im), "row %d tf %r" % (b, tf[b]))
    sh.done()


DYN = [(nc - 1, 0) for nc in C.NC_DYN] + [(10, 12), (5, 1)]


@pytest.mark.parametrize("n,R", DYN, ids=["deg %d R = %d" % c for c in DYN])
def test_dynamics_dev_speed_with_and_without_the_angular_rows(capi, torch, n, R):
    """obtg_dynamics_dev: the speed rows alone (k_dynamics at R = 0, the speed entry's kernels at R > 0), then with the angular
    rows and the second speed bound from the same pass (k_dynamics2 | k_dynamics_elev): all to the bound"""
    N, B = 5, 3
    tf = np.array(C.SPEED_TF)
    vmax, vmin = C.SPEED_BOUNDS
    sh = Shares("dynamics_dev, deg %d R = %d" % (n, R))
    Yb = C.rows_batch(700 + n + R, B, N, 2, n)
    ctx = capi.Context(N, 2, n, R)
    try:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dY, dtf = torch.from_numpy(Yb).cuda(), torch.from_numpy(tf).cuda()
        nan = float("nan")
        sp0 = torch.full((B, ctx.len_speed), nan, dtype=torch.float64, device="cuda")
        sp1, sp2 = torch.full_like(sp0, nan), torch.full_like(sp0, nan)
        an = torch.full((B, ctx.len_ang_rate), nan, dtype=torch.float64, device="cuda")
        ctx.dynamics_dev(dY.data_ptr(), dtf.data_ptr(), B, vmax, True, 1.0, sp0.data_ptr(), None)
        ctx.set_second_speed_bound(vmin, False, sp2.data_ptr())
        ctx.dynamics_dev(dY.data_ptr(), dtf.data_ptr(), B, vmax, True, 1.0, sp1.data_ptr(), an.data_ptr())
        torch.cuda.synchronize()
        ctx.set_second_speed_bound(0.0, False, None)
        order = ctx.ang_rate_order_in_effect()
        ctx.use_own_stream()
    finally:
        ctx.close()
    sp0, sp1, sp2, an = (t.cpu().numpy() for t in (sp0, sp1, sp2, an))
    for b in range(B):
        rmax, rmin = C.speed(Yb[b], N, 2, R, tf[b], vmax, 1), C.speed(Yb[b], N, 2, R, tf[b], vmin, 0)
        sh.hold("speed alone", sp0[b].reshape(N, -1), rmax, "row %d" % b)
        sh.hold("speed beside the angular rows", sp1[b].reshape(N, -1), rmax, "row %d" % b)
        sh.hold("second speed bound", sp2[b].reshape(N, -1), rmin, "row %d" % b)
        sh.hold("angular rows", an[b].reshape(N, -1), C.ang_rate(Yb[b], N, R, tf[b], 1.0, order), "row %d" % b)
    sh.done()


# ---------------------------------------------------------------------------------------------------------------------
#  angular rate
# ---------------------------------------------------------------------------------------------------------------------
ANG = list(C.ANG_CASES) + [("any degree m = %d" % m, 2, 6, m - 6, 0, "full", ("k_generic_angrate", 1 if m > 6 else 0)) for m in (6, 7, 127, 128)] + \
      [("any degree m = 2", 3, 2, 0, 0, "full", ("k_generic_angrate", 0))]


@pytest.mark.parametrize("case", ANG, ids=[c[0] for c in ANG])
def test_angular_rate_rows(capi, case):
    name, N, n, R, order, kind, form = case
    assert C.ang_form(n, R, order) == form
    tfs = np.array(C.ANG_TF[:2] if 4 * (n + R) > 600 else C.ANG_TF)
    B = len(tfs)
    sh = Shares("angular rate, %s" % name)
    Yb = C.rows_batch(800 + n + R, B, N, 2, n, kind)
    ctx = capi.Context(N, 2, n, R)
    try:
        ctx.set_ang_rate_order(order)
        in_effect = ctx.ang_rate_order_in_effect()
        got = ctx.ang_rate(Yb, tfs, 1.0).reshape(B, N, -1)
    finally:
        ctx.close()
    assert in_effect == form[1], (in_effect, form)
    sched = ""
    if form[0] == "k_generic_angrate":
        sched = ", balanced" if C.angrate_balanced(n + R) else ", plain schedule"
    inside = 0
    for b in range(B):
        ref = C.ang_rate(Yb[b], N, R, tfs[b], 1.0, in_effect)
        if form[0] == "k_generic_angrate" and ref.peak >= C.DBL_MAX / 2:
            # outside the any-degree kernel's finiteness condition (include/obtg.h): nothing is promised of this row
            print("\n%s tf %r: the unnormalised sums reach %.3g x DBL_MAX, outside the kernel's domain" % (name, tfs[b], float(ref.peak / C.DBL_MAX)))
            continue
        inside += 1
        sh.hold("%s%s, order %d" % (form[0], sched, in_effect), got[b], ref, "row %d tf %r" % (b, tfs[b]))
    sh.true(inside >= 1, "no row of the case inside the kernel's domain")
    sh.done()


def test_angular_rate_any_degree_just_inside_the_finiteness_condition(capi):
    """k_generic_angrate at its limit m = 250 with tf chosen (a power of two times 7.3) so that the largest unnormalised sum
    C(4m, k) num_k lies in [DBL_MAX / 128, DBL_MAX / 2): finite and within the quotient test -- the condition include/obtg.h states"""
    N, n, R = 2, 6, 244
    Y = C.swarm(950, N, 2, n)
    tf = C.ang_tf_inside(Y, N, R, 7.3)
    sh = Shares("angular rate, m = 250 just inside the finiteness condition (tf = %r)" % tf)
    ctx = capi.Context(N, 2, n, R)
    try:
        assert ctx.ang_rate_order_in_effect() == 1
        got = ctx.ang_rate(Y, tf, 1.0).reshape(N, -1)
    finally:
        ctx.close()
    sh.true(bool(np.isfinite(got).all()), "a non-finite element inside the condition")
    sh.hold("k_generic_angrate, plain schedule, order 1", got, C.ang_rate(Y, N, R, tf, 1.0, 1), "rows")
    sh.done()


@pytest.mark.parametrize("n,R,order", [(5, 0, 0), (10, 12, 0), (10, 12, 1), (10, 12, 2), (12, 0, 0)])
def test_vehicle_at_rest(capi, n, R, order):
    """Every control point of vehicle 1 the same point: numerator and denominator are exact zeros, the row must be NaN
    (optimization.py:608 keeps 0 / 0); the other vehicles' rows pass the quotient test.

    tf = 2.0: n / tf times the coordinates 3.25, -1.5 is exact.  tf = 7.3: it is not, and this case found a defect -- the
    derivative `p[c] * (-val) + p[c + 1] * val` is contracted into fma(-val, p[c], fl(val * p[c + 1])), which for equal control
    points returned the rounding error of val * p: the vehicle had a velocity of ~1e-16 |val p|, the cross product
    y'' x' - x'' y' still cancelled exactly, and every element of the row was max_rate^2 - 0 / tiny = 1.0 in orders 0 and 1
    (k_dynamics2, k_dynamics_elev, k_generic_angrate; order 2's double-double pass returned NaN).  diff_elev1 (bern_device.h)
    and k_generic_angrate now give two equal control points the derivative coefficient 0, as the unfused reference arithmetic
    does; every other coefficient keeps its bits."""
    N = 3
    sh = Shares("angular rate, a vehicle at rest, deg %d R = %d order %d" % (n, R, order))
    Y = C.swarm(900 + n, N, 2, n)
    Y[2:4] = [[3.25], [-1.5]]
    tfs = np.array([2.0, 7.3])
    ctx = capi.Context(N, 2, n, R)
    try:
        ctx.set_ang_rate_order(order)
        in_effect = ctx.ang_rate_order_in_effect()
        got = ctx.ang_rate(np.stack([Y, Y]), tfs, 1.0).reshape(2, N, -1)
    finally:
        ctx.close()
    for b in range(2):
        print("\nvehicle at rest, tf %r: %d of %d elements NaN, first values %r" % (tfs[b], int(np.isnan(got[b, 1]).sum()), got.shape[2], got[b, 1, :3].tolist()))
        sh.hold("order %d" % in_effect, got[b], C.ang_rate(Y, N, R, tfs[b], 1.0, in_effect), "tf %r" % tfs[b])
    sh.done()


def test_near_stop_vehicles_in_all_three_orders(capi, golden_dir):
    """tests/golden/nearstop.npz: every order's rows meet the quotient test of its counts (order 2: order 0's).  The rows the
    double-double pass rewrote (those that differ from order 0's) are recorded element by element against the exact value, in
    units of 2^-53 |exact|, and held to the quotient test of an evaluation whose tables carry 64 bits (constraint_rows_ref
    ang_shares dd=True).  Measured on MI355X: 2070 (tf = 10) and 1150 (tf = 14.3) units, i.e. 2.3e-13 relative, where order 0
    is 3.6e6 and 5.0e6 units off: the condition number times 2^-64, which is what include/obtg.h now says ("a few 1e-16"
    was the sentence's error, not the kernel's: the ratio of the two orders is the 2^11 between 64 and 53 bits)."""
    g = np.load(os.path.join(golden_dir, "nearstop.npz"))
    Y = g["Y"]
    N, n, R = int(g["par"][0]), int(g["par"][2]), int(g["par"][3])
    sh = Shares("angular rate, near-stop vehicles")
    units = []
    for tf in g["tfs"]:
        got = {}
        for order in (0, 1, 2):
            ctx = capi.Context(N, 2, n, R)
            try:
                ctx.set_ang_rate_order(order)
                assert ctx.ang_rate_order_in_effect() == order
                got[order] = ctx.ang_rate(Y, float(tf), 1.0).reshape(N, -1)
            finally:
                ctx.close()
            sh.hold("order %d" % order, got[order], C.ang_rate(Y, N, R, float(tf), 1.0, order), "tf %g" % tf)
        rewritten = [v for v in range(N) if not np.array_equal(got[2][v], got[0][v])]
        ref = C.ang_rate(Y, N, R, float(tf), 1.0, 0)
        u2, u0 = C.ang_rel_units(got[2], ref, rewritten), C.ang_rel_units(got[0], ref, rewritten)
        s, ok = C.ang_shares(got[2], ref, dd=True)
        dd_share = max([float(s[v].max()) for v in rewritten] + [0.0])
        units.append((u2, dd_share))
        print("\nnear-stop, tf %g: the double-double pass rewrote vehicles %r; largest |c - exact| / |exact| on them %.3g units of 2^-53 "
              "(order 0 on the same rows: %.3g); share of the double-double bound %.3g" % (tf, rewritten, u2, u0, dd_share))
        sh.true(len(rewritten) >= 1, "tf %g: the double-double pass rewrote no row" % tf)
        # 64-bit tables against float64's 53: 2^11 closer; granted 2^8
        sh.true(u2 * 256 <= u0, "tf %g: the double-double rows are %.3g units off, float64's %.3g" % (tf, u2, u0))
        sh.true(all(ok[v].all() for v in rewritten), "tf %g: a rewritten row outside the double-double bound (share %.3g)" % (tf, dd_share))
    sh.done()
