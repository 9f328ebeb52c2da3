// Host build of csrc/struct_layout.h (the launch layout of the structured FD step and the decode of its block ids) for
// tests/test_struct_layout.py:
//   g++ -O2 -std=c++17 -shared -fPIC tests/native/struct_layout_host.cpp -o <tmp>/libstruct_layout_host.so
#include "../../optimalbeziertrajectorygeneration_amd/csrc/struct_layout.h"

using namespace obtg;

extern "C" {

int sl_sizeof_layout() { return (int)sizeof(StructLayout); }

// knobs: dynamic_rows, share S, share G, ticket_rows, sep_wgs, gjk_wgs (kStructUnset = INT_MIN: not set)
void sl_knobs_from_env(int* knobs)
{
    const StructKnobs k = struct_knobs_from_env();
    knobs[0] = k.dynamic_rows; knobs[1] = k.share[0]; knobs[2] = k.share[1]; knobs[3] = k.ticket_rows; knobs[4] = k.sep_wgs; knobs[5] = k.gjk_wgs;
}

// shape: deg, R, n_veh, n_pairs, n_hull_pairs, n_cus, row0, wpc, gjk_chunk_pairs, dyn_split
void sl_layout(const int* shape, int B, const int* knobs, StructLayout* out)
{
    const StructShape s{ shape[0], shape[1], shape[2], shape[3], shape[4], shape[5], shape[6], shape[7], shape[8], shape[9] };
    StructKnobs k;
    k.dynamic_rows = knobs[0]; k.share[0] = knobs[1]; k.share[1] = knobs[2]; k.ticket_rows = knobs[3]; k.sep_wgs = knobs[4]; k.gjk_wgs = knobs[5];
    *out = struct_layout(s, B, k);
}

void sl_header(const StructLayout* l, char* out, int size) { struct_layout_header(*l, out, (size_t)size); }

// every block id of the grid: out[block] = kind, id, live
void sl_blocks(const StructLayout* l, int* out)
{
    for (int b = 0; b < l->grid; ++b) {
        const StructBlock k = struct_block(*l, b);
        out[3 * b] = k.kind; out[3 * b + 1] = k.id; out[3 * b + 2] = k.live;
    }
}

static StructStreamKind stream_kind(const StructLayout* l, int kind) { return kind == 0 ? struct_sep_kind(*l) : struct_gjk_kind(*l); }

// S (kind 0) or G (kind 2) workgroup `id`: out = unit, range, sweeper, and a fixed range's rows b0, b1
void sl_worker(const StructLayout* l, int kind, int id, int* out)
{
    const StructStreamKind k = stream_kind(l, kind);
    const StructWorker w = struct_worker(k, l->tickets != 0, id);
    const StructRows r = struct_range_rows(k, w.range);
    out[0] = w.unit; out[1] = w.range; out[2] = w.sweeper; out[3] = r.b0; out[4] = r.b1;
}

// the rows of the ticket drawn at counter value `cur`
void sl_ticket(const StructLayout* l, int kind, int cur, int* out)
{
    const StructRows r = struct_ticket_rows(stream_kind(l, kind), l->B, cur);
    out[0] = r.b0; out[1] = r.b1;
}

void sl_chunk_pairs(const StructLayout* l, int chunk, int* out)
{
    const StructPairs p = struct_chunk_pairs(*l, chunk);
    out[0] = p.k0; out[1] = p.n_valid;
}

int sl_fix_row(const StructLayout* l, int id) { return struct_fix_row(*l, id); }

// D workgroup `id`: out = part, group, sub, b0, b1, live
void sl_dyn(const StructLayout* l, int id, int* out)
{
    const StructDyn d = struct_dyn_worker(*l, id);
    out[0] = d.part; out[1] = d.group; out[2] = d.sub; out[3] = d.b0; out[4] = d.b1; out[5] = d.live;
}

}  // extern "C"
