// The launch layout of the structured finite-difference step (gjk_kernels.hip k_step_fd_structured), as pure integer
// arithmetic: how many workgroups of each kind (S, F, G, D), which rows the fixed ranges own and which go out by ticket,
// how the kinds interleave over every 16 block ids -- and the decode the kernel performs on a block id.  Every output
// element is written exactly once only if these agree, so they live in one place that needs no GPU to check:
// plain C++17, no HIP header, no allocation, no global state (tests/test_struct_layout.py compiles it for the host and
// walks every block id of the bench shapes).  launch_step_fd_structured copies a StructLayout into StructuredParams.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <limits.h>
#include <algorithm>

#if defined(__HIPCC__)
#define OBTG_SL_HD __host__ __device__ __forceinline__
#else
#define OBTG_SL_HD inline
#endif

namespace obtg {

constexpr int kStructWave = 64;        // pairs of an S group, vehicles of a D group, rows of a D fix-up group (kWave)

// rows at run time: the default share of a group's rows, in per cent, that its sweepers write.
// C3, short runs on one box, parent 0.1009 ms: S 10 / 20 / 30 / 40 / 50 / 60 / 70 % swept 0.0988 / 0.1030 / 0.1041 / 0.1077 /
// 0.1105 / 0.1149 / 0.1259 ms -- a chip full of sweepers alone stores at 5.7 TB/s, under the 6.3 of the mixed launch, so they
// get what fills the tail and no more; G sweepers on top cost more (20,20: 0.1144; 30,30: 0.1161 against 0.1041)
constexpr int kStructSweptShareSep = 10, kStructSweptShareGjk = 0;

// what the layout depends on, and nothing else
struct StructShape {
    int deg, R;                        // degree n of the trajectories, DEG_ELEV
    int n_veh;
    int n_pairs, n_hull_pairs;         // separation pairs (S), hull pairs (G)
    int n_cus;                         // compute units of the device (0: unknown, 256 assumed)
    int row0;                          // the FD view's first row in the batch (obtg_fd_view_begin_rows)
    int wpc, gjk_chunk_pairs, dyn_split;      // from step_fd_structured_plan: workgroups per CU of the kernel form, pairs of a G chunk, D streams of 16 vehicles
};

// The switches the tests flip in-process (tests/test_gpu_structured_dynamic_rows.py); kStructUnset: the variable is not set.
constexpr int kStructUnset = INT_MIN;
struct StructKnobs {
    int dynamic_rows = kStructUnset;   // OBTG_STRUCT_DYNAMIC_ROWS: 0 fixed ranges alone, 1 sweepers whatever the shape
    int share[2] = { kStructUnset, kStructUnset };   // OBTG_STRUCT_DYNAMIC_SHARE "S,G": per cent of a group's rows that are swept (100: no fixed ranges at all)
    int ticket_rows = kStructUnset;    // OBTG_STRUCT_TICKET_ROWS: S rows per ticket; G tickets are twice as many rows (half as wide)
    int sep_wgs = kStructUnset;        // OBTG_STRUCT_SEP_WGS / OBTG_STRUCT_GJK_WGS: S / G workgroups; with the sweepers on, the
    int gjk_wgs = kStructUnset;        // sweepers of all groups together
};

// The one place that reads them.  Per launch, not once: A/B runs and the tests change them between calls.
inline StructKnobs struct_knobs_from_env()
{
    StructKnobs k;
    if (const char* e = getenv("OBTG_STRUCT_DYNAMIC_ROWS")) if (e[0]) k.dynamic_rows = e[0] != '0';
    if (const char* e = getenv("OBTG_STRUCT_DYNAMIC_SHARE")) {
        k.share[0] = kStructSweptShareSep; k.share[1] = kStructSweptShareGjk;
        if (sscanf(e, "%d,%d", &k.share[0], &k.share[1]) < 2) k.share[1] = k.share[0];
    }
    if (const char* e = getenv("OBTG_STRUCT_TICKET_ROWS")) k.ticket_rows = atoi(e);
    if (const char* e = getenv("OBTG_STRUCT_SEP_WGS")) k.sep_wgs = atoi(e);
    if (const char* e = getenv("OBTG_STRUCT_GJK_WGS")) k.gjk_wgs = atoi(e);
    return k;
}

// Every integer of the split.  The fields up to gjk_static_rows are StructuredParams' of the same name.
struct StructLayout {
    int n_sep_groups, sep_rows_per;    // S: groups of the separation block, rows per fixed range
    int gjk_chunks, gjk_chunk_pairs, gjk_rows_per;   // G
    int fix_chunk;                     // F: candidates per segment of the fix-up pass
    int n_kind[4];                     // workgroups of each kind (S, F, G, D)
    int per16[4];                      // of every 16 block ids, per16[k] belong to kind k,
    unsigned char pat[16], rank[16];   // in the order pat[]; rank[i]: how many slots of pat[i]'s kind come before slot i
    int dyn_groups_per_row, dyn_rows_per, dyn_streams, dyn_fix_groups, dyn_split;   // D
    int first_pert;                    // the view's first perturbed local row: 1, or 0 in a row range that starts later
    int sep_ticket_rows, gjk_ticket_rows;            // 0 with the tickets off
    int sep_static_ranges, sep_static_rows, gjk_static_ranges, gjk_static_rows;
    int grid;                          // block ids of the launch: a multiple of 16
    int sep_sweepers, gjk_sweepers;    // sweepers per group / per chunk, behind its fixed ranges
    int tickets;                       // rows handed out at run time (flat S and G kinds); 0: fixed ranges only
    int B, n_veh, n_hull_pairs;        // the launch's rows and the shape's counts that the decode below needs
};

// Today's split.  Rows at run time (flat steps): with fixed ranges alone the launch has a tail -- whichever workgroup is
// dispatched last still has its whole range to write, and for the last tenth of the span most slots are empty
// (profiles/struct_dynamic_rows/timeline_parent_c3.txt).  So only the first rows of every group go to fixed ranges, of the
// usual length; the rest are handed out by ticket (StructuredParams::tickets) to SWEEPERS, whose block ids come behind
// every other id of the grid: they start in the slots the draining launch leaves empty, share what is left down to a
// ticket and end together.  A sweeper stays until its group's rows are gone, which is why they are not mixed in
// earlier: S and G workers that draw ALL rows by ticket crowd the F and D workgroups out of the slots.
// With more groups than half the slots (C4: 510 groups on 256 or 512 slots) the fixed ranges stay alone.
inline StructLayout struct_layout(const StructShape& s, int B, const StructKnobs& knobs)
{
    StructLayout l{};
    l.B = B; l.n_veh = s.n_veh; l.n_hull_pairs = s.n_hull_pairs;
    const bool elev = s.R > 0;
    const int L = 2 * s.deg + 1, LR = L + s.R;
    // S: one workgroup per (64-pair group, row range); about two thousand workgroups of streams
    l.n_sep_groups = (s.n_pairs + kStructWave - 1) / kStructWave;
    // (a large step -- C4: 58 GB of separation rows -- gets more, so that a stream stays near 4 MB)
    const double sep_stream_bytes = 8.0 * kStructWave * LR * (double)B * l.n_sep_groups;
    // (small batches -- a rank's share of a row-sharded iteration -- get fewer, longer streams: every S workgroup repeats row
    // 0's products for its group and every G workgroup its gjkNew chunk, and 2048 + 1024 of them are three rounds of resident
    // workgroups for a few rows each.  C3, tools/r04_struct_small_batch_scan.sh: B = 145 0.044 -> 0.027 ms with 512 / 384
    // workgroups, B = 289 0.055 -> 0.040 with 1024 / 512; from B = 577 on the old numbers are the best)
    const double s_floor = std::min(2048.0, std::max(256.0, 3.5 * B));
    int s_target = (int)std::min(32768.0, std::max(s_floor, sep_stream_bytes / (4 << 20)));
    // G: chunks of ~80 hull pairs (one short gjkNew phase per workgroup), row ranges for ~512 workgroups
    l.gjk_chunk_pairs = s.gjk_chunk_pairs;
    l.gjk_chunks = (s.n_hull_pairs + l.gjk_chunk_pairs - 1) / l.gjk_chunk_pairs;
    // (with the sweepers on, the two worker-count knobs count sweepers, not fixed ranges)
    const int n_slots = (s.n_cus > 0 ? s.n_cus : 256) * s.wpc;
    const bool dyn_rows = !elev && (knobs.dynamic_rows != kStructUnset ? knobs.dynamic_rows != 0 : 2 * (l.n_sep_groups + l.gjk_chunks) <= n_slots);
    const bool has_sep_wgs = knobs.sep_wgs != kStructUnset, has_gjk_wgs = knobs.gjk_wgs != kStructUnset;
    if (has_sep_wgs && !dyn_rows) s_target = std::max(1, knobs.sep_wgs);
    const int g_target = has_gjk_wgs && !dyn_rows ? std::max(1, knobs.gjk_wgs) : (int)std::min(1024.0, std::max(192.0, 2.6 * B));
    int g_target_b = (int)std::min(32768.0, std::max((double)g_target, 68.0 * s.n_hull_pairs * (double)B / (4 << 20)));
    int s_ranges = std::max(1, std::min(B, s_target / std::max(1, l.n_sep_groups)));
    l.sep_rows_per = (B + s_ranges - 1) / s_ranges;
    s_ranges = (B + l.sep_rows_per - 1) / l.sep_rows_per;
    int g_ranges = std::max(1, std::min(B, g_target_b / std::max(1, l.gjk_chunks)));
    l.gjk_rows_per = (B + g_ranges - 1) / g_ranges;
    g_ranges = (B + l.gjk_rows_per - 1) / l.gjk_rows_per;
    l.sep_static_ranges = s_ranges; l.gjk_static_ranges = g_ranges;
    l.sep_static_rows = l.gjk_static_rows = B;
    l.tickets = dyn_rows;
    if (dyn_rows) {
        // a ticket of 40 - 48 KB (C3: 4 rows of a separation group, 9 of a chunk): about 3 us of a sweeper's stores
        l.sep_ticket_rows = std::max(2, (48 << 10) / (8 * kStructWave * L));
        l.gjk_ticket_rows = std::max(2, (48 << 10) / (68 * l.gjk_chunk_pairs));
        if (knobs.ticket_rows != kStructUnset) {
            l.sep_ticket_rows = std::max(1, knobs.ticket_rows);
            l.gjk_ticket_rows = 2 * l.sep_ticket_rows;
        }
        int share[2] = { kStructSweptShareSep, kStructSweptShareGjk };
        if (knobs.share[0] != kStructUnset)
            for (int k = 0; k < 2; ++k) share[k] = std::max(0, std::min(100, knobs.share[k]));
        // (whole ranges: a fixed range is as long as without sweepers)
        l.sep_static_rows = B - (int)((long long)B * share[0] / 100);
        l.sep_static_rows -= l.sep_static_rows % l.sep_rows_per;
        l.gjk_static_rows = B - (int)((long long)B * share[1] / 100);
        l.gjk_static_rows -= l.gjk_static_rows % l.gjk_rows_per;
        l.sep_static_ranges = l.sep_static_rows / l.sep_rows_per;
        l.gjk_static_ranges = l.gjk_static_rows / l.gjk_rows_per;
        // sweepers: a chip's worth of S, half of one of G; no more than tickets, unless the count was asked for
        const int s_swept = B - l.sep_static_rows, g_swept = B - l.gjk_static_rows;
        if (s_swept > 0)
            l.sep_sweepers = has_sep_wgs ? std::max(1, knobs.sep_wgs / std::max(1, l.n_sep_groups))
                                         : std::max(1, std::min(n_slots / std::max(1, l.n_sep_groups), (s_swept + l.sep_ticket_rows - 1) / l.sep_ticket_rows));
        if (g_swept > 0)
            l.gjk_sweepers = has_gjk_wgs ? std::max(1, knobs.gjk_wgs / std::max(1, l.gjk_chunks))
                                         : std::max(1, std::min(n_slots / 2 / std::max(1, l.gjk_chunks), (g_swept + l.gjk_ticket_rows - 1) / l.gjk_ticket_rows));
    }
    l.fix_chunk = 256;
    l.n_kind[0] = l.n_sep_groups * (l.sep_static_ranges + l.sep_sweepers);
    l.first_pert = s.row0 > 0 ? 0 : 1;            // (a range that starts later: its local row 0 is a perturbed row too)
    l.n_kind[1] = B - l.first_pert;
    l.n_kind[2] = l.gjk_chunks * (l.gjk_static_ranges + l.gjk_sweepers);
    // D: ~256 streams of row 0's groups (at most 64 rows each, at least 4 when there are that many: at C5 a stream of 19
    // rows keeps its workgroup for 430 us of a 650 us launch, one of 5 rows for 190), the advanced vehicles 64 to a
    // group, and one workgroup per 8 rows that looks for rows with their own tf
    l.dyn_groups_per_row = (s.n_veh + kStructWave - 1) / kStructWave;
    l.dyn_rows_per = std::min(64, std::max((B + 255) / 256, std::min(4, B)));
    l.dyn_split = s.dyn_split;      // (DEG_ELEV > 0: stream workgroups of 16 vehicles that collect their rows in LDS)
    if (l.dyn_split) l.dyn_rows_per = std::min(64, 4 * l.dyn_rows_per);      // (16 vehicles per stream workgroup instead of 64: the same bytes)
    l.dyn_streams = (l.dyn_split ? 4 : 1) * l.dyn_groups_per_row * ((B + l.dyn_rows_per - 1) / l.dyn_rows_per);
    l.dyn_fix_groups = (B - l.first_pert + kStructWave - 1) / kStructWave;
    const int dyn_x = l.dyn_groups_per_row * ((B - 1 + 7) / 8);
    l.n_kind[3] = l.dyn_streams + l.dyn_fix_groups + dyn_x;
    // shares of every 16 block ids by expected work (workgroups x duration on the C3 timeline: S 12.5, F 15.2, G 20.2, D 10.7 us)
    // (what decides is where each kind's ids run out: the kinds should end at about the same block id, so the D
    // weights are those of its neighbours, not its 190 us streams: 7:3:3:3 instead of 7:4:4:1 costs C5 10 %)
    const double cost_flat[4] = { 12.5, 15.2, 20.2, 16.0 }, cost_elev[4] = { 40.0, 36.0, 38.0, 40.0 };
    const double* cost = elev ? cost_elev : cost_flat;     // (DEG_ELEV > 0: the streams are 2n+R+1 columns wide, the dynamics groups k_dynamics_elev's)
    double w[4], tot = 0.0;
    // (the sweepers are left out: the shares make the fixed ranges, F, G and D run out of ids together, and the sweepers'
    // ids follow)
    const int n_fixed[4] = { l.n_sep_groups * l.sep_static_ranges, l.n_kind[1], l.gjk_chunks * l.gjk_static_ranges, l.n_kind[3] };
    for (int k = 0; k < 4; ++k) { w[k] = n_fixed[k] * cost[k]; tot += w[k]; }
    tot -= w[3];
    w[3] = (l.dyn_streams + l.dyn_fix_groups) * cost[3];      // (the workgroups that look for rows with their own tf come last and cost nothing)
    tot += w[3];
    int sum = 0;
    for (int k = 0; k < 4; ++k) { l.per16[k] = l.n_kind[k] > 0 ? std::max(1, (int)(16.0 * w[k] / tot + 0.5)) : 0; sum += l.per16[k]; }
    while (sum != 16) {             // give to / take from the kind with the largest share
        int kmax = 0;
        for (int k = 1; k < 4; ++k) if (l.per16[k] > l.per16[kmax]) kmax = k;
        l.per16[kmax] += sum < 16 ? 1 : -1;
        sum += sum < 16 ? 1 : -1;
    }
    // spread each kind's slots evenly over the 16
    struct Slot { double pos; int kind; };
    Slot order[16];
    int n = 0;
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < l.per16[k]; ++j) order[n++] = Slot{ (j + 0.5) / l.per16[k] + 1e-3 * k, k };
    std::sort(order, order + 16, [](const Slot& a, const Slot& b) { return a.pos < b.pos; });
    int seen[4] = { 0, 0, 0, 0 };
    int groups = 0;
    for (int i = 0; i < 16; ++i) { l.pat[i] = (unsigned char)order[i].kind; l.rank[i] = (unsigned char)seen[order[i].kind]++; }
    for (int k = 0; k < 4; ++k)
        if (l.per16[k] > 0) groups = std::max(groups, (l.n_kind[k] + l.per16[k] - 1) / l.per16[k]);
    l.grid = groups * 16;
    return l;
}

// the first line of a workgroup timeline (OBTG_TIMELINE; tools/timeline_report.py, profiles/struct_dynamic_rows)
inline void struct_layout_header(const StructLayout& l, char* out, size_t size)
{
    snprintf(out, size, "# grid %u structured n_S %d n_F %d n_G %d n_D %d per16 %d %d %d %d pat %d%d%d%d%d%d%d%d%d%d%d%d%d%d%d%d B %d ticket_rows %d %d",
             (unsigned)l.grid, l.n_kind[0], l.n_kind[1], l.n_kind[2], l.n_kind[3], l.per16[0], l.per16[1], l.per16[2], l.per16[3],
             l.pat[0], l.pat[1], l.pat[2], l.pat[3], l.pat[4], l.pat[5], l.pat[6], l.pat[7], l.pat[8], l.pat[9], l.pat[10],
             l.pat[11], l.pat[12], l.pat[13], l.pat[14], l.pat[15], l.B, l.sep_ticket_rows, l.gjk_ticket_rows);
}

// ---- The decode of a block id, as k_step_fd_structured performs it.  These are the HOST MIRROR of the kernel's text:
// calling them from the kernel, even the first one alone, moves its instructions (the scheduler orders the loads of the
// kernel arguments differently), and the kernel's code is held fixed.  So the kernel keeps its text, with a comment at
// every piece that names its mirror here; a change to either side is a change to both.  The host test walks every
// block id of a layout through them and counts who writes what.

struct StructBlock { int kind, id; bool live; };      // kind: 0 S, 1 F, 2 G, 3 D; live: id < n_kind[kind] (the others return at once)
// (block id mod 8 is the XCD: the pattern is rotated by one slot per group of 16, or every XCD would see one or two kinds only)
OBTG_SL_HD StructBlock struct_block(const StructLayout& l, int block)
{
    const int grp = block >> 4, slot = (block + grp) & 15;
    const int kind = l.pat[slot];
    const int id = grp * l.per16[kind] + l.rank[slot];
    return StructBlock{ kind, id, id < l.n_kind[kind] };
}

// What the S kind (units: separation groups) and the G kind (units: hull-pair chunks) have in common: a unit's first
// static_ranges workgroups own fixed ranges of rows [0, static_rows), those behind them are its sweepers and draw
// tickets of ticket_rows of the rows [static_rows, B) from the unit's counter.
struct StructStreamKind { int units, rows_per, static_ranges, static_rows, ticket_rows; };
OBTG_SL_HD StructStreamKind struct_sep_kind(const StructLayout& l)
{
    return StructStreamKind{ l.n_sep_groups, l.sep_rows_per, l.sep_static_ranges, l.sep_static_rows, l.sep_ticket_rows };
}
OBTG_SL_HD StructStreamKind struct_gjk_kind(const StructLayout& l)
{
    return StructStreamKind{ l.gjk_chunks, l.gjk_rows_per, l.gjk_static_ranges, l.gjk_static_rows, l.gjk_ticket_rows };
}

struct StructWorker { int unit, range; bool sweeper; };
OBTG_SL_HD StructWorker struct_worker(const StructStreamKind& k, bool tickets, int id)
{
    const int unit = id % k.units, range = id / k.units;
    return StructWorker{ unit, range, tickets && range >= k.static_ranges };
}

struct StructRows { int b0, b1; };     // rows [b0, b1)
// (with DEG_ELEV > 0 the S kind bounds its ranges by B: the tickets are off there and static_rows is B)
OBTG_SL_HD StructRows struct_range_rows(const StructStreamKind& k, int range)
{
    const int b0 = range * k.rows_per, e = b0 + k.rows_per;
    return StructRows{ b0, k.static_rows < e ? k.static_rows : e };
}
// the rows of the ticket whose counter value (before the draw) was `cur`; cur >= B - static_rows: none are left
OBTG_SL_HD StructRows struct_ticket_rows(const StructStreamKind& k, int B, int cur)
{
    const int n_swept = B - k.static_rows, e = cur + k.ticket_rows;
    return StructRows{ k.static_rows + cur, k.static_rows + (n_swept < e ? n_swept : e) };
}

// G: the hull pairs [k0, k0 + n_valid) of a chunk
struct StructPairs { int k0, n_valid; };
OBTG_SL_HD StructPairs struct_chunk_pairs(const StructLayout& l, int chunk)
{
    const int k0 = chunk * l.gjk_chunk_pairs, left = l.n_hull_pairs - k0;
    const int n = l.gjk_chunk_pairs < left ? l.gjk_chunk_pairs : left;
    return StructPairs{ k0, n > 0 ? n : 0 };
}

// F: the row whose own pairs workgroup `id` evaluates
OBTG_SL_HD int struct_fix_row(const StructLayout& l, int id) { return id + l.first_pert; }

// D.  part 0: a stream -- vehicle group `group` of the view's unperturbed row (dyn_split: its vehicles 16 sub .. 16 sub + 15;
// live = false where the last group has none there) copied into rows [b0, b1); part 1: a fix-up group -- the advanced vehicles
// of the perturbed rows [b0, b1), 64 to a group; part 2: vehicle group `group` of those rows of [b0, b1) that have a tf of
// their own, in full.
struct StructDyn { int part, group, sub, b0, b1; bool live; };
OBTG_SL_HD StructDyn struct_dyn_worker(const StructLayout& l, int id)
{
    const int gd = l.dyn_groups_per_row;
    if (id < l.dyn_streams) {
        const int gs = l.dyn_split ? 4 * gd : gd;
        const int r = id / gs, u = id - r * gs;
        const int b0 = r * l.dyn_rows_per, e = b0 + l.dyn_rows_per, b1 = l.B < e ? l.B : e;
        if (!l.dyn_split) return StructDyn{ 0, u, -1, b0, b1, true };
        const int sub = u & 3;
        return StructDyn{ 0, u >> 2, sub, b0, b1, 64 * (u >> 2) + 16 * sub < l.n_veh };
    }
    if (id < l.dyn_streams + l.dyn_fix_groups) {
        const int g = id - l.dyn_streams, n = l.B - l.first_pert;
        const int e = kStructWave * g + kStructWave;
        return StructDyn{ 1, g, -1, l.first_pert + kStructWave * g, l.first_pert + (n < e ? n : e), true };
    }
    const int x = id - l.dyn_streams - l.dyn_fix_groups, xr = x / gd, gv = x - xr * gd;
    const int e = 9 + 8 * xr;
    return StructDyn{ 2, gv, -1, 1 + 8 * xr, l.B < e ? l.B : e, true };
}

}  // namespace obtg
