// Curve <-> curve and curve <-> polygon collision checks: Bezier.collCheck -> _collCheckBez2Bez (bezier.py:859-862,
// 1561-1614) and Bezier.collCheck2Poly -> _collCheckBez2Poly (bezier.py:864-867, 1617-1651).
//
// Both are depth-first subdivisions that ask gjkNew for its FLAG alone: no closest points enter the result, every split
// is at 0.5, no parameter interval is tracked, and a node whose hulls are apart ends its branch with `1`.
//   _collCheckBez2Bez(c1, c2, cnt, alpha): cnt += 1; cnt > 100 -> -1.  flag > 0 -> 1.  alpha = min(alpha, smallest
//     end-point distance); 0 >= alpha (1 - eps) -> alpha.  Else split both and, for (c3,c5) (c3,c6) (c4,c5) (c4,c6) in that
//     order, alpha = min(alpha, child(alpha)); -> alpha.
//   _collCheckBez2Poly(c, poly, cnt): cnt += 1; cnt > 100 -> -1.  flag > 0 -> 1.  Else split; 1 when the left half gives 1
//     and then the right half gives 1 (the right half is not visited otherwise), else 0.
// The arrangement is k_min_dist_quad's (gjk_kernels.hip): a wavefront is a worker on a ticket queue; the children of a
// node are evaluated when the node is split, a 16-lane row of the wavefront each, by the lockstep gjkNew machines of
// gjk_device.h (planar when every z of the call is +0); the walk, which IS order dependent (once alpha <= 0 every later
// sibling ends after its one gjkNew call; the polygon form's `and` short-circuits), reads the children's records in the
// reference's order and counts a gjkNew call only where the reference makes one.  A frame's blob -- the half curves of an
// expanded node and its children's records -- is kept per depth in a global stack per worker; its scalars (curve form:
// alpha and the next child; polygon form: the next child) in LDS, the walk's own frame in registers.  The reference's
// cnt bounds the depth at 100, so the stack has a fixed size.
//
// This unit is compiled with -ffp-contract=off, as gjk_kernels.hip: the sub-curves and every branch decision are the
// reference's bit for bit.
#include <cstdlib>

#include "gjk_device.h"
#include "obtg_internal.h"
#include "md_device.h"
#pragma clang fp contract(fast)
#include "bern_device.h"      // wave_sync
#pragma clang fp contract(off)

namespace obtg {

using gjk::Ctx;
using gjk::MemLds;
using gjk::Poly;
using gjk::Result;

enum { C_CAP = 0, C_POS, C_UB, C_NREC = 4 };      // a child's record: gjkNew never returns / flag > 0 / _upperbound (curve form)
// frames of a worker's stack: a node the reference visits with cnt = c <= 99 and splits becomes frame c - 1; one visited
// with cnt = 100 is not split (its children would all return -1 before any gjkNew call)
constexpr int kCcFrames = 99;
constexpr int kCcMaxCnt = 100;
__host__ __device__ constexpr int cc_blob(int K) { return 12 * K + 4 * C_NREC; }      // c3 c4 c5 c6, four records
__host__ __device__ constexpr int cp_blob(int K) { return 6 * K + 2 * C_NREC; }       // left, right, two records
static size_t cc_lds_bytes(int K) { return sizeof(double) * ((size_t)2 * cc_blob(K) + 64 + 2 * kCcFrames); }
static size_t cp_lds_bytes(int K) { return sizeof(double) * ((size_t)2 * cp_blob(K) + 48 + 64 + kCcFrames); }

struct CcParams {
    const double* __restrict__ curves;   // [n_curves][3][K]
    const int* __restrict__ pa;
    const int* __restrict__ pb;
    int n_pairs, K, max_iter, md_cap, max_nodes;
    double eps;
    double* stack;                        // [workers][kCcFrames][cc_blob(K)]
    double* __restrict__ res;             // [n_pairs]
    int* __restrict__ info;               // [n_pairs][4]
    int* queue;                           // the next pair (zeroed before the launch)
};

struct CpParams {
    const double* __restrict__ curves;   // [n_curves][3][K]
    const double* __restrict__ soa;      // polygons, [3][K_a] per polygon at 3 * off[a]
    const int* __restrict__ off;
    const int* __restrict__ pc;
    const int* __restrict__ pp;
    int n_pairs, K, max_iter, md_cap, max_nodes;
    double* stack;                        // [workers][kCcFrames][cp_blob(K)]
    double* __restrict__ res;
    int* __restrict__ info;
    int* queue;
};

// The record of the pair of point sets a row of the wavefront names: whether gjkNew returns, its flag and, for two curves,
// _upperbound (bezier.py:1499-1541: the smallest of the four end-point distances, numpy's argmin: the first NaN wins).
// gjkNew's closest points are formed by the machine and dropped: nothing here reads them.
template <bool PLANAR, bool CURVES>
__device__ __forceinline__ void cc_eval_row(const double* lds, int o1, int K, int o2, int cs2, int K2, int max_iter, int md_cap,
                                            double* rec)
{
    Ctx<MemLds> g;
    g.mem = MemLds{ lds };
    g.P1 = Poly{ o1, K, K, 1 };
    g.P2 = Poly{ o2, cs2, K2, 1 };
    g.trace = nullptr; g.trace_cap = 0; g.n_support = 0;
    Result gr;
    if constexpr (PLANAR) gjk::run_quarter2<MemLds>(g, max_iter, md_cap, gr);
    else gjk::run_quarter<MemLds>(g, max_iter, md_cap, gr);
    const bool cap = gr.status == OBTG_ST_MD_CAP || gr.status == OBTG_ST_CYCLE;
    double ub = 0.0;
    if constexpr (CURVES) {
        int am;
        ub = md_upper_bound<PLANAR>(lds + o1, K, lds + o2, K, am);
    }
    rec[C_CAP] = cap ? 1.0 : 0.0; rec[C_POS] = (gr.flag > 0 && !cap) ? 1.0 : 0.0; rec[C_UB] = ub;
}

// Worker waves per SIMD the register allocation is held to.  The planar builds take 104 .. 118 registers, so four fit with
// nothing spilled; the 3-D machine held to four (128 registers) spills 240 .. 310 B of scratch per lane, so it runs two.
#ifndef OBTG_CC_MIN_WAVES_PLANAR
#define OBTG_CC_MIN_WAVES_PLANAR 4
#endif
#ifndef OBTG_CC_MIN_WAVES_3D
#define OBTG_CC_MIN_WAVES_3D 2
#endif
__host__ __device__ constexpr int cc_min_waves(bool planar) { return planar ? OBTG_CC_MIN_WAVES_PLANAR : OBTG_CC_MIN_WAVES_3D; }

// PLANAR: every curve of the call has z == +0 in every control point (the host has looked).
// KC: the control-point count the kernel is built for (0: any count up to 16).
template <bool PLANAR, int KC>
__global__ __launch_bounds__(64, cc_min_waves(PLANAR)) void k_coll_check(const CcParams p)
{
    extern __shared__ double cc_lds[];
    const int lane = threadIdx.x, q = lane >> 4;
    const int K = KC > 0 ? KC : p.K, BL = cc_blob(K);
    double* st = p.stack + (size_t)blockIdx.x * kCcFrames * BL;
    double* dump = cc_lds + 2 * BL;             // [64] the split's idle stores
    double* scs = dump + 64;                    // [kCcFrames][2] (alpha, next child) of the frames below the walk's
  for (;;) {
    // every lane issues the atomic and every lane stores the results: no lane-0-only region at either end of the loop body
    // (hipcc merged two such regions across the back edge)
    const int ticket = atomicAdd(p.queue, lane == 0 ? 1 : 0);
    const int k = __builtin_amdgcn_readfirstlane(ticket);
    if (k >= p.n_pairs) break;
    wave_sync();
    double* cur = cc_lds;                       // [BL] blob of the frame `cur_depth`
    double* nxt = cur + BL;                     // [BL] blob being built
    // the pair's own curves as the blob of a frame "-1", pieces c1 c1 c2 c2, whose child 0 is the root
    const double* ca = p.curves + (size_t)p.pa[k] * 3 * K;
    const double* cb = p.curves + (size_t)p.pb[k] * 3 * K;
    for (int i = lane; i < 3 * K; i += kWave) {
        const double a = ca[i], bq = cb[i];
        nxt[i] = a; nxt[3 * K + i] = a; nxt[6 * K + i] = bq; nxt[9 * K + i] = bq;
    }
    double f_alpha = INFINITY;        // the frame whose children the walk is going through (wave-uniform values)
    int f_next = 0;
    int depth = -1, cur_depth = -1;   // depth: the frame in registers; cur_depth: which frame's blob `cur` holds
    int eval_depth = -1;              // which frame's blob `nxt` is about to become
    int nodes = 0, calls = 0, dmax = 0, status = OBTG_MD_OK;
    double r = 0.0;
    bool done = false;
    while (!done) {
        // ---- the four children of the blob in `nxt`, a row of the wavefront each
        wave_sync();
        cc_eval_row<PLANAR, true>(cc_lds, (int)(nxt - cc_lds) + (q >> 1) * 3 * K, K, (int)(nxt - cc_lds) + (2 + (q & 1)) * 3 * K, K, K,
                                  p.max_iter, p.md_cap, nxt + 12 * K + q * C_NREC);
        wave_sync();
        if (eval_depth >= 0) {
            double* f = st + (size_t)eval_depth * BL;
            for (int i = lane; i < BL; i += kWave) f[i] = nxt[i];
        }
        { double* tsw = cur; cur = nxt; nxt = tsw; }
        cur_depth = eval_depth;
        // ---- the walk, until a node has to be split (its pieces go to `nxt`) or the search ends.  A value returned to a
        //      frame: `alpha = min(alpha, child)`, Python's min: the child's value when it is smaller; to frame -1: the answer.
#define OBTG_CC_RETURN() \
    { if (depth < 0) { done = true; break; } \
      if (r < f_alpha) f_alpha = r; \
      continue; }
        for (;;) {
            if (f_next >= 4) {                   // the four children are done: `return alpha`
                r = f_alpha;
                depth--;
                if (depth < 0) { done = true; break; }
                f_alpha = scs[2 * depth]; f_next = (int)scs[2 * depth + 1];
                OBTG_CC_RETURN()
            }
            // ---- child f_next of the frame: (c3,c5) (c3,c6) (c4,c5) (c4,c6), visited with cnt = depth + 2 <= 100
            const int ch = f_next++, h1 = ch >> 1, h2 = ch & 1;
            const int cnt = depth + 2;
            if (nodes >= p.max_nodes) { status = OBTG_MD_NODE_CAP; done = true; break; }
            nodes++;
            if (cnt > dmax) dmax = cnt;
            if (cur_depth != depth) {            // the walk came back up: fetch this frame's blob again
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                const double* f = st + (size_t)depth * BL;
                for (int i = lane; i < BL; i += kWave) cur[i] = f[i];
                cur_depth = depth;
                wave_sync();
            }
            const double* rec = cur + 12 * K + ch * C_NREC;
            calls++;
            if (rec[C_CAP] != 0.0) { status = OBTG_MD_GJK_CAP; done = true; break; }
            if (rec[C_POS] != 0.0) { r = 1.0; OBTG_CC_RETURN() }
            double alpha = f_alpha;
            const double ub = rec[C_UB];
            if (ub <= alpha) alpha = ub;
            if (0.0 >= alpha * (1 - p.eps)) { r = alpha; OBTG_CC_RETURN() }
            if (cnt >= kCcMaxCnt) {              // its four children return -1 at once: min(alpha, -1), four times
                r = -1.0 < alpha ? -1.0 : alpha;
                OBTG_CC_RETURN()
            }
            // ---- split the child: both pieces of both its curves to `nxt`; this frame goes to `scs`, the child's into the registers
            if constexpr (KC > 0 && 6 * KC <= kWave) split_both_t<KC>(cur + h1 * 3 * K, cur + (2 + h2) * 3 * K, K, 0.5, 0.5, nxt, 0, 6, dump);
            else if (KC == 0 && 6 * K <= kWave) split_both_t<0>(cur + h1 * 3 * K, cur + (2 + h2) * 3 * K, K, 0.5, 0.5, nxt, 0, 6, dump);
            else {
                split_both_t<KC>(cur + h1 * 3 * K, cur + (2 + h2) * 3 * K, K, 0.5, 0.5, nxt, 0, 3, dump);
                split_both_t<KC>(cur + h1 * 3 * K, cur + (2 + h2) * 3 * K, K, 0.5, 0.5, nxt, 3, 3, dump);
            }
            if (depth >= 0) { scs[2 * depth] = f_alpha; scs[2 * depth + 1] = (double)f_next; }
            f_alpha = alpha; f_next = 0;
            depth++;
            eval_depth = depth;
            break;
        }
#undef OBTG_CC_RETURN
    }
    // (every lane, the same values to the same addresses)
    p.res[k] = status == OBTG_MD_OK ? r : 0.0;
    if (p.info) { p.info[4 * k] = nodes; p.info[4 * k + 1] = calls; p.info[4 * k + 2] = dmax; p.info[4 * k + 3] = status; }
  }
}

// The curve <-> polygon form: a node has two children, the curve's halves against the same polygon (at most 16 vertices,
// copied to LDS once per pair); rows 0 and 1 of the wavefront take them, rows 2 and 3 repeat them.  The right half is
// evaluated beside the left one whether or not the walk will ask for it; it is COUNTED only when the walk does.
// PLANAR: the curves and the polygons of the call all have z == +0.
template <bool PLANAR, int KC>
__global__ __launch_bounds__(64, cc_min_waves(PLANAR)) void k_coll_check2poly(const CpParams p)
{
    extern __shared__ double cp_lds[];
    const int lane = threadIdx.x, q = (lane >> 4) & 1;
    const int K = KC > 0 ? KC : p.K, BL = cp_blob(K);
    double* st = p.stack + (size_t)blockIdx.x * kCcFrames * BL;
    double* pol = cp_lds + 2 * BL;              // [3][16] polygon, SoA
    double* dump = pol + 48;                    // [64]
    double* scs = dump + 64;                    // [kCcFrames] the next child of the frames below the walk's
  for (;;) {
    const int ticket = atomicAdd(p.queue, lane == 0 ? 1 : 0);      // (see k_coll_check)
    const int k = __builtin_amdgcn_readfirstlane(ticket);
    if (k >= p.n_pairs) break;
    wave_sync();
    double* cur = cp_lds;
    double* nxt = cur + BL;
    const int po = p.off[p.pp[k]], PK = p.off[p.pp[k] + 1] - po;
    const double* ca = p.curves + (size_t)p.pc[k] * 3 * K;
    for (int i = lane; i < 3 * K; i += kWave) { const double a = ca[i]; nxt[i] = a; nxt[3 * K + i] = a; }      // frame "-1": pieces c, c
    for (int i = lane; i < 3 * PK; i += kWave) pol[(i / PK) * 16 + (i % PK)] = p.soa[3 * po + i];
    int f_next = 0;
    int depth = -1, cur_depth = -1, eval_depth = -1;
    int nodes = 0, calls = 0, dmax = 0, status = OBTG_MD_OK;
    double r = 0.0;
    bool done = false;
    while (!done) {
        wave_sync();
        cc_eval_row<PLANAR, false>(cp_lds, (int)(nxt - cp_lds) + q * 3 * K, K, (int)(pol - cp_lds), 16, PK, p.max_iter, p.md_cap,
                                   nxt + 6 * K + q * C_NREC);
        wave_sync();
        if (eval_depth >= 0) {
            double* f = st + (size_t)eval_depth * BL;
            for (int i = lane; i < BL; i += kWave) f[i] = nxt[i];
        }
        { double* tsw = cur; cur = nxt; nxt = tsw; }
        cur_depth = eval_depth;
        bool ret = false;             // r is a child's value on its way to the frame `depth`
        for (;;) {
            if (ret) {
                if (depth < 0) { done = true; break; }
                if (r == 1.0 && f_next < 2) ret = false;        // `left == 1 and ...`: now the right half
                else {                                          // this frame's value: 1 when both halves gave 1, else 0
                    r = r == 1.0 ? 1.0 : 0.0;
                    depth--;
                    if (depth < 0) { done = true; break; }
                    f_next = (int)scs[depth];
                    continue;
                }
            }
            const int h1 = f_next++;             // the left (0) / right (1) half, visited with cnt = depth + 2 <= 100
            const int cnt = depth + 2;
            if (nodes >= p.max_nodes) { status = OBTG_MD_NODE_CAP; done = true; break; }
            nodes++;
            if (cnt > dmax) dmax = cnt;
            if (cur_depth != depth) {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                const double* f = st + (size_t)depth * BL;
                for (int i = lane; i < BL; i += kWave) cur[i] = f[i];
                cur_depth = depth;
                wave_sync();
            }
            const double* rec = cur + 6 * K + h1 * C_NREC;
            calls++;
            if (rec[C_CAP] != 0.0) { status = OBTG_MD_GJK_CAP; done = true; break; }
            if (rec[C_POS] != 0.0) { r = 1.0; ret = true; continue; }
            if (cnt >= kCcMaxCnt) { r = 0.0; ret = true; continue; }      // its left half returns -1 at once: not 1
            split_both_t<KC>(cur + h1 * 3 * K, cur + h1 * 3 * K, K, 0.5, 0.5, nxt, 0, 3, dump);
            if (depth >= 0) scs[depth] = (double)f_next;
            f_next = 0;
            depth++;
            eval_depth = depth;
            break;
        }
    }
    p.res[k] = status == OBTG_MD_OK ? r : 0.0;
    if (p.info) { p.info[4 * k] = nodes; p.info[4 * k + 1] = calls; p.info[4 * k + 2] = dmax; p.info[4 * k + 3] = status; }
  }
}

// ------------------------------------------------------------------------------------- launchers
bool coll_check_supported(int K, int max_poly_K) { return K >= 2 && K <= kMdQuadMaxK && max_poly_K <= 16; }

static unsigned cc_workers(const obtg_ctx* c, int n_pairs, size_t lds, bool planar)
{
    return (unsigned)min_dist_workers(c, n_pairs, lds, cc_min_waves(planar));
}

// doubles of frame stack the launch writes: a stack per worker wave (the planar form's grid is the larger one)
size_t coll_check_stack_doubles(const obtg_ctx* c, int K, int n_pairs, bool poly, bool planar)
{
    if (n_pairs <= 0 || !coll_check_supported(K, 0)) return 0;
    return (size_t)cc_workers(c, n_pairs, poly ? cp_lds_bytes(K) : cc_lds_bytes(K), planar) * kCcFrames * (poly ? cp_blob(K) : cc_blob(K));
}

int launch_coll_check(obtg_ctx* c, const double* d_curves, int K, const int* d_pa, const int* d_pb, int n_pairs, double eps,
                      int max_iter, int md_cap, int max_nodes, double* d_stack, double* d_res, int* d_info, int* d_queue,
                      bool planar)
{
    if (n_pairs <= 0) return OBTG_OK;
    if (!coll_check_supported(K, 0)) return OBTG_ERR_UNSUPPORTED;
    if (!d_queue || !d_stack) return OBTG_ERR_ARG;
    CcParams p{ d_curves, d_pa, d_pb, n_pairs, K, max_iter, md_cap, max_nodes, eps, d_stack, d_res, d_info, d_queue };
    ScopedKernelTimer t(c, OBTG_K_MIN_DIST);
    OBTG_HIP(c, hipMemsetAsync(d_queue, 0, sizeof(int), c->stream));
    void (*kern)(const CcParams) = planar ? k_coll_check<true, 0> : k_coll_check<false, 0>;
    switch (K) {        // the counts with a build of their own
#define OBTG_CASE(NC_) case NC_: kern = planar ? k_coll_check<true, NC_> : k_coll_check<false, NC_>; break;
        OBTG_NC_DYN(OBTG_CASE)
#undef OBTG_CASE
        default: break;
    }
    const size_t lds = cc_lds_bytes(K);
    hipLaunchKernelGGL(kern, dim3(cc_workers(c, n_pairs, lds, planar)), dim3(kWave), lds, c->stream, p);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_coll_check2poly(obtg_ctx* c, const double* d_curves, int K, const double* d_soa, const int* d_off, const int* d_pc,
                           const int* d_pp, int n_pairs, int max_iter, int md_cap, int max_nodes, double* d_stack, double* d_res,
                           int* d_info, int* d_queue, int max_poly_K, bool planar)
{
    if (n_pairs <= 0) return OBTG_OK;
    if (!coll_check_supported(K, max_poly_K)) return OBTG_ERR_UNSUPPORTED;
    if (!d_queue || !d_stack) return OBTG_ERR_ARG;
    CpParams p{ d_curves, d_soa, d_off, d_pc, d_pp, n_pairs, K, max_iter, md_cap, max_nodes, d_stack, d_res, d_info, d_queue };
    ScopedKernelTimer t(c, OBTG_K_MIN_DIST);
    OBTG_HIP(c, hipMemsetAsync(d_queue, 0, sizeof(int), c->stream));
    void (*kern)(const CpParams) = planar ? k_coll_check2poly<true, 0> : k_coll_check2poly<false, 0>;
    switch (K) {
#define OBTG_CASE(NC_) case NC_: kern = planar ? k_coll_check2poly<true, NC_> : k_coll_check2poly<false, NC_>; break;
        OBTG_NC_DYN(OBTG_CASE)
#undef OBTG_CASE
        default: break;
    }
    const size_t lds = cp_lds_bytes(K);
    hipLaunchKernelGGL(kern, dim3(cc_workers(c, n_pairs, lds, planar)), dim3(kWave), lds, c->stream, p);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

}  // namespace obtg
