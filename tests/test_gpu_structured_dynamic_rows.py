"""The structured FD step with rows handed out at run time (k_step_fd_structured, StructuredParams::tickets): behind the
fixed row ranges of an S group or a G chunk come its sweepers, workgroups that draw tickets of a few rows from the
group's counter.  Which sweeper writes which row then depends on the order the hardware runs them in; what is written
must not.  Most cases here sweep EVERY row (OBTG_STRUCT_DYNAMIC_SHARE=100: no fixed ranges in front), the hardest form.  The independent side of every comparison is the brute-force sweep of the MATERIALISED batch, which never
routes (tests/test_gpu_fd_view_routing.py), compared bit for bit; every output starts as NaN / -7, so an element that no
worker wrote shows up, and the separation block's rows are checked for the same reason the other arrays are.

The knobs are read per call: OBTG_STRUCT_DYNAMIC_ROWS (1: sweepers whatever the shape, 0: fixed ranges alone),
OBTG_STRUCT_DYNAMIC_SHARE ("S,G" per cent of a group's rows that are swept), OBTG_STRUCT_TICKET_ROWS (rows per S ticket; a
G ticket is twice as many), OBTG_STRUCT_SEP_WGS / OBTG_STRUCT_GJK_WGS (sweepers of all groups together)."""
import numpy as np
import pytest

from test_gpu_fd_view_routing import Case, same_bits

TICKET = 4                       # S rows per ticket in these tests (G: 8)
B_MAX = 37
# (N, n, M, point obstacles)
SMALL = {"six_vehicles": (6, 10, 2, None), "twelve_vehicles": (12, 10, 2, None),
         "point_obstacles": (12, 10, 2, [[20.0, 30.0], [55.5, 41.0], [70.0, 12.5]])}
LARGE = {"rows_of_70KB": (256, 15, 0, None), "rows_of_96KB": (558, 10, 2, None)}      # two and one workgroup per CU
TF_ROWS = ("one_tf", "a_few_rows_with_their_own_tf", "every_row_its_own_tf")


def tf_rows_of(kind, B):
    """tf of rows 0 .. B-1; a view of fewer rows takes the first ones, so one reference serves every batch size."""
    tf = np.full(B, 6.5)
    if kind == "a_few_rows_with_their_own_tf":
        for k in (1, 2, 4, 9, 11, B - 1):
            if 0 < k < B:
                tf[k] = 6.5 + 1e-3 * k
        if B > 6:
            tf[6] = np.nextafter(6.5, 7.0)
    if kind == "every_row_its_own_tf":
        tf = np.linspace(3.0, 9.0, B)
    return tf


@pytest.fixture(scope="module")
def capi():
    from optimalbeziertrajectorygeneration_amd import _capi
    assert _capi.device_count() > 0, "these tests need the GPU"
    return _capi


@pytest.fixture(scope="module")
def synth():
    from optimalbeziertrajectorygeneration_amd import synth
    return synth


class Ref:
    """A case with the brute-force results of its first `rows` batch rows, per tf pattern: computed once, never written again."""

    def __init__(self, capi, synth, shape, rows):
        import torch
        N, n, M, pobs = dict(SMALL, **LARGE)[shape]
        self.c = Case(capi, synth, N, 2, n, 0, M, 1, B=rows, pobs=pobs, seed=41)
        self.rows, self.tf, self.ref = rows, {}, {}
        dY = self.c.materialised(rows)
        for kind in TF_ROWS:
            self.tf[kind] = torch.from_numpy(tf_rows_of(kind, rows)).cuda()
            self.ref[kind] = self.c.bufs(rows)
            self.c.sweep(dY.data_ptr(), self.tf[kind], rows, self.ref[kind])

    def check(self, kind, r0, cnt, what):
        """The in-view call on rows [r0, r0 + cnt) into fresh NaN / -7 buffers: one launch, the reference's bits."""
        import torch
        c = self.c
        got = c.bufs(cnt)
        ks = c.in_view(self.tf[kind][r0:r0 + cnt].contiguous(), cnt, got, row_begin=r0)
        assert ks == {"pair_sweep": 1}, (what, ks)
        same_bits(torch, {k: v[r0:r0 + cnt] for k, v in self.ref[kind].items()}, got, what)
        return got


@pytest.fixture(scope="module")
def refs(capi, synth):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Ref(capi, synth, shape, 3 if shape in LARGE else B_MAX)
        return made[shape]
    yield get
    for r in made.values():
        r.c.close()


@pytest.fixture
def dynamic(monkeypatch):
    """Tickets on, every row of both kinds handed out by ticket (no fixed ranges in front), 4 / 8 rows per ticket."""
    monkeypatch.setenv("OBTG_STRUCT_DYNAMIC_ROWS", "1")
    monkeypatch.setenv("OBTG_STRUCT_DYNAMIC_SHARE", "100")
    monkeypatch.setenv("OBTG_STRUCT_TICKET_ROWS", str(TICKET))
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize("share", ["default", "50", "30,70", "0,100", "100,0", "3,97"])
def test_fixed_ranges_in_front_of_the_swept_rows(refs, dynamic, share):
    """The first rows of a group in fixed ranges, the rest by ticket ("S,G" per cent swept; the library's default; a kind
    with nothing swept has no sweepers): full batches, short ones, row ranges."""
    if share == "default":
        dynamic.delenv("OBTG_STRUCT_DYNAMIC_SHARE")
        dynamic.delenv("OBTG_STRUCT_TICKET_ROWS")
    else:
        dynamic.setenv("OBTG_STRUCT_DYNAMIC_SHARE", share)
    for shape in ("six_vehicles", "point_obstacles"):
        r = refs(shape)
        for r0, cnt in ((0, B_MAX), (0, 2), (0, TICKET + 1), (5, 9), (B_MAX - 7, 7)):
            for tf_rows in TF_ROWS:
                r.check(tf_rows, r0, cnt, (share, shape, r0, cnt, tf_rows))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SMALL))
@pytest.mark.parametrize("tf_rows", TF_ROWS)
def test_batch_sizes_around_the_ticket_size(refs, dynamic, shape, tf_rows):
    """B = 1 and 2, one below / at / one above the S ticket (4 rows) and the G ticket (8 rows), and 37 rows."""
    r = refs(shape)
    for B in (1, 2, TICKET - 1, TICKET, TICKET + 1, 2 * TICKET - 1, 2 * TICKET, 2 * TICKET + 1, B_MAX):
        r.check(tf_rows, 0, B, (shape, tf_rows, B))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["six_vehicles", "point_obstacles"])
@pytest.mark.parametrize("workers", [1, 256])
def test_worker_counts(refs, dynamic, shape, workers):
    """One worker per group (it draws every ticket), and 256 workers for the one or two groups of these shapes: far more
    than rows, most of them find the counter exhausted and leave."""
    dynamic.setenv("OBTG_STRUCT_SEP_WGS", str(workers))
    dynamic.setenv("OBTG_STRUCT_GJK_WGS", str(workers))
    r = refs(shape)
    for B in (2, TICKET + 1, B_MAX):
        for tf_rows in TF_ROWS:
            r.check(tf_rows, 0, B, (shape, workers, B, tf_rows))


@pytest.mark.gpu
@pytest.mark.parametrize("ticket", [1, 100])
def test_ticket_of_one_row_and_of_more_rows_than_the_batch(refs, dynamic, ticket):
    dynamic.setenv("OBTG_STRUCT_TICKET_ROWS", str(ticket))
    r = refs("twelve_vehicles")
    for B in (1, 5, B_MAX):
        for tf_rows in TF_ROWS:
            r.check(tf_rows, 0, B, (ticket, B, tf_rows))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SMALL))
def test_row_range_views_without_row_0(refs, dynamic, shape):
    """obtg_fd_view_begin_rows: the counters hand out LOCAL rows; rows [5, 14) of the 37, the last rows, one row."""
    r = refs(shape)
    for r0, cnt in ((5, 9), (B_MAX - 7, 7), (1, 1), (3, TICKET), (0, B_MAX)):
        for tf_rows in TF_ROWS:
            r.check(tf_rows, r0, cnt, (shape, r0, cnt, tf_rows))


@pytest.mark.gpu
def test_counters_are_ready_for_every_next_call_of_a_context(refs, dynamic):
    """Twenty calls in a row, then another B, then a row range, then the fixed ranges and tickets again: each call finds
    the bank the call before it left zero, with nothing queued between them."""
    r = refs("twelve_vehicles")
    for k in range(20):
        r.check("a_few_rows_with_their_own_tf", 0, B_MAX, ("call", k))
    r.check("a_few_rows_with_their_own_tf", 0, 9, "another B")
    r.check("every_row_its_own_tf", 5, 9, "a row range")
    dynamic.setenv("OBTG_STRUCT_DYNAMIC_ROWS", "0")
    r.check("one_tf", 0, B_MAX, "fixed ranges in between")
    dynamic.setenv("OBTG_STRUCT_DYNAMIC_ROWS", "1")
    for k in range(3):
        r.check("one_tf", 0, B_MAX, ("tickets again", k))


@pytest.mark.gpu
def test_two_contexts_on_two_streams_used_alternately(capi, synth, refs, dynamic):
    """Each context has its own counters: launches of two contexts on two streams, queued alternately with nothing
    between them, all give the reference's bits."""
    import torch
    r = refs("twelve_vehicles")
    N, n, M, pobs = SMALL["twelve_vehicles"]
    cases = [Case(capi, synth, N, 2, n, 0, M, 1, B=B_MAX, seed=41) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    kind = "a_few_rows_with_their_own_tf"
    dtf = r.tf[kind]
    outs = [[c.bufs(B_MAX) for _ in range(6)] for c in cases]
    torch.cuda.synchronize()
    for c, s in zip(cases, streams):
        c.ctx.set_stream(s.cuda_stream)
    for k in range(6):
        for c, mine in zip(cases, outs):
            o = mine[k]
            c.ctx.set_second_speed_bound(0.4, False, o["sp2"].data_ptr())
            c.ctx.fd_view_begin(c.d0.data_ptr(), c.fixed, c.h, B_MAX, row_begin=0)
            try:
                c.ctx.constraint_sweep_dev(None, dtf.data_ptr(), B_MAX, 0.9, o["sep"].data_ptr(), 4.0, True, 1.5, o["sp"].data_ptr(),
                                           o["an"].data_ptr(), o["flag"].data_ptr(), o["p1"].data_ptr(), o["p2"].data_ptr(),
                                           o["dist"].data_ptr(), o["ns"].data_ptr(), o["st"].data_ptr(), 128, 500)
            finally:
                c.ctx.fd_view_end()
    torch.cuda.synchronize()
    for i, mine in enumerate(outs):
        for k, o in enumerate(mine):
            same_bits(torch, r.ref[kind], o, ("context", i, "call", k))
    for c in cases:
        c.ctx.set_second_speed_bound(0.0, False, None)
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["twelve_vehicles"] + sorted(LARGE))
def test_fixed_ranges_and_tickets_give_the_same_bits_in_one_process(refs, dynamic, shape):
    """OBTG_STRUCT_DYNAMIC_ROWS = 0 and = 1 on one context; the large-row kernel forms (two and one workgroup per CU: 256
    vehicles of degree 15, 558 of degree 10; B = 3) take the tickets only when asked to."""
    import torch
    r = refs(shape)
    B = r.rows
    for tf_rows in TF_ROWS:
        dynamic.setenv("OBTG_STRUCT_DYNAMIC_ROWS", "0")
        fixed = r.check(tf_rows, 0, B, (shape, tf_rows, "fixed ranges"))
        dynamic.setenv("OBTG_STRUCT_DYNAMIC_ROWS", "1")
        tickets = r.check(tf_rows, 0, B, (shape, tf_rows, "tickets"))
        same_bits(torch, fixed, tickets, (shape, tf_rows, "fixed ranges against tickets"))
        if B > 2:
            r.check(tf_rows, 1, B - 1, (shape, tf_rows, "tickets, rows from 1"))
