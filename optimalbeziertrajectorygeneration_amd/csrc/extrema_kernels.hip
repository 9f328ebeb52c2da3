// True extrema of Bernstein polynomials over [0, 1] for gfx950 (MI355X): obtg_bern_extrema and the fused consumer
// obtg_temporal_sep_true_min (include/obtg.h states the contract).
//
// What the reference has here is Bezier.min / Bezier.max (bezier.py:631-667, 727-763), a subdivision sketch that
// extrapolates outside a child's span (bezier.py:659-661 with 560-561) and so returns values below the minimum or does
// not return.  This unit is NOT that recursion: it is a certified search, val - bound <= tol, held to exact rationals.
//
// Search (wave_search): depth-first bisection at 1/2.  A sub-curve's smallest coefficient bounds it from below, the
// end-point values met so far bound the minimum from above (U); a sub-curve with U - lower <= tol is a leaf.  Of two live
// children the one with the smaller lower bound is followed, the other waits on a stack of kExStack frames in LDS.
// Every split is a pair of averages per level -- 0.5 * a + 0.5 * b with contraction off -- so a row's result
// depends on its coefficients alone.
//
// Kernel form: the first step (smallest coefficient at an end, or the end values within tol of it) is one LANE per row:
// most rows of a constraint batch end there.  A row that needs the search gets the whole WAVE: lane k holds coefficient
// k, a de Casteljau level is one DPP move of the lane above's value and one average (md_device.h wave_next_lane), the left
// piece is lane 0's value level by level, the right piece what each lane holds when it stops.  No per-lane coefficient
// arrays in the search (K is a run-time count up to 64), the stack is kExStack x (K + 3) doubles per wave.
//
// True-minimum row families (obtg_temporal_sep_true_min[_jac], obtg_speed_true_min[_jac], obtg_ang_rate_true_min[_jac],
// obtg_accel_true_min[_jac], obtg_jerk_true_min[_jac]): the polynomial of a pair's separation, of a vehicle's own speed, of one
// side of its angular-rate bound, of its acceleration, of its jerk, formed in the lane and searched as above -- one kernel body
// (true_min_body) over a family struct (TsepRows, SpeedRows, AngRows, AccelRows, JerkRows), under the kernel names
// k_tsep_true_min / k_speed_true_min / k_ang_true_min / k_accel_true_min / k_jerk_true_min.  The acceleration and the jerk
// families' fused value-and-blocks kernels are the counts of OBTG_NC_ACCEL_LIST / OBTG_NC_JERK_LIST (obtg_internal.h): every
// count of OBTG_NC_SEP, in 2-D and 3-D.  The keep-in family (obtg_keep_in_true_min[_jac]: KeepInRows, k_keep_in_true_min,
// k_keep_in_envelope, bern_device.h keep_in_coeff / keep_in_envelope_block) is the one whose polynomial is linear in the curve:
// L = NC coefficients per item, not 2 NC - 1 -- the row length is the family's (obtg_internal.h RowFamily::row_len).
// Envelope Jacobian: the derivative of the item's polynomial at the t_star the search returned, bern_device.h
// envelope_block / speed_envelope_block / ang_envelope_block / accel_envelope_block / jerk_envelope_block -- written with explicit fma, so it is the same arithmetic here
// (contraction off) as anywhere else.  Fused form: the <NC, DIM, true> kernels re-read the item's control points from Y after the search (no
// register is held across wave_search for it) and every lane writes its own block.  Two-launch form: the value path, then
// k_tsep_envelope / k_speed_envelope / k_ang_envelope / k_accel_envelope / k_jerk_envelope on Y and t_star, any degree up to 31.
#include <algorithm>
#include <cfloat>
#include <utility>

#include "obtg_internal.h"
#include "md_device.h"
#pragma clang fp contract(fast)
#include "bern_device.h"
#pragma clang fp contract(off)

namespace obtg {

constexpr int kExStack = 32;          // live sub-curves waiting per row; one more: OBTG_MD_DEPTH_CAP
constexpr int kExMaxK = kWave;        // a row is a row of lanes
constexpr int kExWaves = 2;           // waves per workgroup (K = 64: 34 KB of stacks)

struct ExOut {
    double val, t, bound;
    int nodes, status;
};

__device__ __forceinline__ double ex_lane(double v, int src)      // src wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ex_lane0(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ex_wave_min(double v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// One row's scan, a coefficient at a time in index order: smallest value, largest magnitude, the two ends.
struct ExScan {
    double m = INFINITY, s = 0.0, c0 = 0.0, cl = 0.0;
    bool bad = false;
    __device__ __forceinline__ void put(double v, int k)
    {
        if (k == 0) c0 = v;
        cl = v;
        bad = bad || !(fabs(v) <= DBL_MAX);
        m = fmin(m, v);
        s = fmax(s, fabs(v));
    }
};

// The first step of a row (node 1).  true: `o` is the row's answer; false: the search has to run (tol is set either way).
__device__ __forceinline__ bool ex_first(const ExScan& sc, double eps_rel, double eps_abs, ExOut& o, double& tol)
{
    tol = fmax(eps_abs, eps_rel * sc.s);
    o.status = OBTG_MD_OK;
    if (sc.bad) { o.val = o.t = o.bound = __builtin_nan(""); o.nodes = 0; return true; }
    o.nodes = 1;
    o.bound = sc.m;
    if (sc.c0 == sc.m) { o.val = sc.c0; o.t = 0.0; return true; }
    if (sc.cl == sc.m) { o.val = sc.cl; o.t = 1.0; return true; }
    if (sc.c0 <= sc.cl) { o.val = sc.c0; o.t = 0.0; } else { o.val = sc.cl; o.t = 1.0; }
    return o.val - sc.m <= tol;
}

// The whole wave on ONE row (every lane must be here).  b: lane k < K holds coefficient k, the other lanes +inf.
// stk: this wave's kExStack x (K + 3) doubles.  Every scalar below is the same in all lanes by construction.
__device__ __forceinline__ ExOut wave_search(double b, const int K, const double tol, const double c0, const double cl,
                                             const double m, const int max_nodes, double* stk)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int pitch = K + 3;
    double U, tU;
    if (c0 <= cl) { U = c0; tU = 0.0; } else { U = cl; tU = 1.0; }
    double bound = INFINITY, t0 = 0.0, w = 1.0, cur_lb = m;
    int nodes = 1, sp = 0, status = OBTG_MD_OK;
    for (;;) {
        if (nodes + 2 > max_nodes) { status = OBTG_MD_NODE_CAP; bound = fmin(bound, cur_lb); break; }
        // deCasteljau at 1/2, both pieces: left[r] is lane 0's value after level r, right[i] lane i's after level K - 1 - i
        double left = b, lbL = ex_lane0(b), mid = lbL;
        for (int r = 1; r < K; ++r) {
            const double up = wave_next_lane(b);
            if (lane <= K - 1 - r) b = 0.5 * b + 0.5 * up;      // (two exact scalings, one rounding: no overflow below DBL_MAX)
            mid = ex_lane0(b);
            if (lane == r) left = mid;
            lbL = fmin(lbL, mid);
        }
        const double lbR = ex_wave_min(b);
        const double hw = 0.5 * w, tm = t0 + hw;
        nodes += 2;
        if (mid < U) { U = mid; tU = tm; }
        const bool aliveL = U - lbL > tol, aliveR = U - lbR > tol;
        if (!aliveL) bound = fmin(bound, lbL);
        if (!aliveR) bound = fmin(bound, lbR);
        if (aliveL && aliveR) {
            if (sp == kExStack) { status = OBTG_MD_DEPTH_CAP; bound = fmin(bound, fmin(lbL, lbR)); break; }
            const bool go_left = lbL <= lbR;
            double* f = stk + sp * pitch;
            if (lane < K) f[lane] = go_left ? b : left;
            if (lane == 0) { f[K] = go_left ? lbR : lbL; f[K + 1] = go_left ? tm : t0; f[K + 2] = hw; }
            ++sp;
            if (go_left) { b = left; cur_lb = lbL; } else { t0 = tm; cur_lb = lbR; }
            w = hw;
        } else if (aliveL) { b = left; cur_lb = lbL; w = hw; }
        else if (aliveR) { t0 = tm; cur_lb = lbR; w = hw; }
        else {
            bool found = false;
            wave_sync();
            while (sp > 0) {
                --sp;
                const double* f = stk + sp * pitch;
                const double plb = f[K];
                if (U - plb > tol) {
                    b = lane < K ? f[lane] : INFINITY;
                    t0 = f[K + 1]; w = f[K + 2]; cur_lb = plb;
                    found = true;
                    break;
                }
                bound = fmin(bound, plb);
            }
            wave_sync();
            if (!found) break;
        }
    }
    if (status != OBTG_MD_OK) {            // what still waits is part of the bracket
        wave_sync();
        for (int i = 0; i < sp; ++i) bound = fmin(bound, stk[i * pitch + K]);
        wave_sync();
    }
    ExOut o;
    o.val = U; o.t = tU; o.bound = fmin(bound, U); o.nodes = nodes; o.status = status;
    return o;
}

struct ExParams {
    const double* __restrict__ c;      // [M][K]
    double* __restrict__ val;          // [M]
    double* __restrict__ t;            // [M] nullable
    double* __restrict__ bound;        // [M] nullable
    int* __restrict__ nodes;           // [M] nullable
    int* __restrict__ status;          // [M] nullable
    long M;
    int K, want_max, max_nodes;
    double eps_rel, eps_abs;
};

__device__ __forceinline__ void ex_store(const ExParams& p, long row, const ExOut& o, bool neg)
{
    p.val[row] = neg ? -o.val : o.val;
    if (p.t) p.t[row] = o.t;
    if (p.bound) p.bound[row] = neg ? -o.bound : o.bound;
    if (p.nodes) p.nodes[row] = o.nodes;
    if (p.status) p.status[row] = o.status;
}

__global__ __launch_bounds__(kExWaves * kWave) void k_bern_extrema(const ExParams p)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    double* stk = lds + (size_t)wave * kExStack * (p.K + 3);
    const long row = ((long)blockIdx.x * kExWaves + wave) * kWave + lane;
    const bool valid = row < p.M;
    const long rr = valid ? row : p.M - 1;
    const bool neg = p.want_max != 0;
    const double* cr = p.c + rr * p.K;
    ExScan sc;
    for (int k = 0; k < p.K; ++k) { const double v = cr[k]; sc.put(neg ? -v : v, k); }
    ExOut mine;
    double tol;
    const bool need = !ex_first(sc, p.eps_rel, p.eps_abs, mine, tol) && valid;
    unsigned long long mask = __ballot(need);
    while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const long row0 = ((long)blockIdx.x * kExWaves + wave) * kWave;
        const double* cs = p.c + (row0 + src) * p.K;
        double b = INFINITY;
        if (lane < p.K) { const double v = cs[lane]; b = neg ? -v : v; }
        const ExOut o = wave_search(b, p.K, ex_lane(tol, src), ex_lane(sc.c0, src), ex_lane(sc.cl, src), ex_lane(sc.m, src),
                                    p.max_nodes, stk);
        if (lane == src) mine = o;
    }
    if (valid) ex_store(p, row, mine, neg);
}

// ---- the true-minimum row families: the polynomial of every item (a (row, pair), a (row, vehicle)) formed in the lane,
// then the same first step and the same search: the coefficients never reach memory.  A family is a struct that names
//   Params                  its parameter block (with ex, sign, offset: the outputs [M], the output transform of its rows),
//   NC, L                   control points per curve, coefficients per item,
//   coeffs(q, item, cf)     the item's coefficients BEFORE the output transform, as its rows have them at R = 0,
//   envelope(q, item, nc, t) the item's envelope block(s) at t, nc <= NC control points at run time,
// and two __global__ wrappers under names of their own (true_min_body, envelope_body; RowKernels finds them for the host).
// A further family starts as a copy of SpeedRows, as AngRows, AccelRows and JerkRows did.
struct TsepExParams {
    const double* __restrict__ Y;      // [B][n_veh*DIM][NC]
    const double* __restrict__ obs;    // [n_obj - n_veh][DIM]
    const int2* __restrict__ pairs;    // [P]
    const double* __restrict__ W2;
    ExParams ex;                       // outputs [B][P]; c unused
    double* __restrict__ jac;          // [B][P][DIM][NC] (the envelope forms)
    int n_veh, P;
    double sign, offset;
};

// obtg_temporal_sep's rows: normsq_coeffs of the pair's differences.  The envelope block is the a side of
// obtg_temporal_sep_jac's conventions -- b's block is the negation, an obstacle has no variable, a pair of two obstacles is
// all zeros; the fused form re-reads the pair's control points from Y (the differences are dead by then).
template <int NC_, int DIM>
struct TsepRows {
    using Params = TsepExParams;
    static constexpr int NC = NC_, L = 2 * NC_ - 1;
    static __device__ __forceinline__ void coeffs(const Params& q, long item, double (&cf)[L])
    {
        const int b = (int)(item / q.P), pr = (int)(item - (long)b * q.P);
        const int2 ij = q.pairs[pr];
        const double* Yrow = q.Y + (size_t)b * q.n_veh * (DIM * NC);
        double a[DIM][NC];
#pragma unroll
        for (int d = 0; d < DIM; ++d)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double xi = ij.x < q.n_veh ? Yrow[(size_t)(ij.x * DIM + d) * NC + c] : q.obs[(ij.x - q.n_veh) * DIM + d];
                const double xj = ij.y < q.n_veh ? Yrow[(size_t)(ij.y * DIM + d) * NC + c] : q.obs[(ij.y - q.n_veh) * DIM + d];
                a[d][c] = xi - xj;
            }
        normsq_coeffs<NC, DIM>(a, as_ctab(q.W2), cf);
    }
    static __device__ __forceinline__ void envelope(const Params& q, long item, int nc, double t)
    {
        const int b = (int)(item / q.P), pr = (int)(item - (long)b * q.P);
        const int2 ij = q.pairs[pr];
        double* o = q.jac + (size_t)item * (DIM * nc);
        if (ij.x >= q.n_veh) {
            for (int e = 0; e < DIM * nc; ++e) o[e] = 0.0;
            return;
        }
        const double* Yrow = q.Y + (size_t)b * q.n_veh * (DIM * nc);
        const double* ya = Yrow + (size_t)ij.x * (DIM * nc);
        const bool veh = ij.y < q.n_veh;
        const double* yb = veh ? Yrow + (size_t)ij.y * (DIM * nc) : q.obs + (size_t)(ij.y - q.n_veh) * DIM;
        envelope_block<NC, DIM>(ya, yb, veh ? nc : 1, veh ? 1 : 0, nc, t, o);
    }
};

struct SpeedExParams {
    const double* __restrict__ Y;      // [B][n_veh*DIM][NC]
    const double* __restrict__ tf;     // [B]
    const double* __restrict__ W2;
    ExParams ex;                       // outputs [B][n_veh]; c unused
    double* __restrict__ jac;          // [B][n_veh][DIM][NC] (the envelope forms)
    double* __restrict__ jac_tf;       // [B][n_veh], nullable
    int n_veh;
    double sign, offset;
};

// obtg_speed's rows, q(t) = sign (DIM/2) |c'(t)|^2 + offset of a vehicle: diff_elev1_speed_rows per coordinate
// (k_normsq_elev's speed path leaves the contraction of that step to the compiler: bern_device.h states what it comes to,
// with explicit fma), then normsq_coeffs.  The envelope is the vehicle's block and its d/dtf.
template <int NC_, int DIM>
struct SpeedRows {
    using Params = SpeedExParams;
    static constexpr int NC = NC_, L = 2 * NC_ - 1;
    static __device__ __forceinline__ void coeffs(const Params& q, long item, double (&cf)[L])
    {
        const int b = (int)(item / q.n_veh);
        const double* v = q.Y + (size_t)item * (DIM * NC);
        const double val = (double)(NC - 1) / q.tf[b];       // Bezier.diff(): (n/T)(P_{i+1} - P_i), then elev(1)
        double a[DIM][NC];
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            double x[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c] = v[d * NC + c];
            diff_elev1_speed_rows<NC>(x, val, a[d]);
        }
        normsq_coeffs<NC, DIM>(a, as_ctab(q.W2), cf);
    }
    static __device__ __forceinline__ void envelope(const Params& q, long item, int nc, double t)
    {
        const int b = (int)(item / q.n_veh);
        const double dtf = speed_envelope_block<NC, DIM>(q.Y + (size_t)item * (DIM * nc), nc, q.tf[b], q.sign, t,
                                                         q.jac + (size_t)item * (DIM * nc));
        if (q.jac_tf) q.jac_tf[item] = dtf;
    }
};

// obtg_accel's rows, q(t) = sign (DIM/2) |c''(t)|^2 + offset of a vehicle: SpeedRows with the source curve one derivative
// further (bern_device.h diff2_elev1_rows, the rows kernels' own function: explicit fma throughout) and the block of the
// second derivative.  The parameter block is the speed family's.
template <int NC_, int DIM>
struct AccelRows {
    using Params = SpeedExParams;
    static constexpr int NC = NC_, L = 2 * NC_ - 1;
    static __device__ __forceinline__ void coeffs(const Params& q, long item, double (&cf)[L])
    {
        const int b = (int)(item / q.n_veh);
        const double* v = q.Y + (size_t)item * (DIM * NC);
        const double val = (double)(NC - 1) / q.tf[b];
        double a[DIM][NC];
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            double x[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c] = v[d * NC + c];
            diff2_elev1_rows<NC>(x, val, a[d]);
        }
        normsq_coeffs<NC, DIM>(a, as_ctab(q.W2), cf);
    }
    static __device__ __forceinline__ void envelope(const Params& q, long item, int nc, double t)
    {
        const int b = (int)(item / q.n_veh);
        const double dtf = accel_envelope_block<NC, DIM>(q.Y + (size_t)item * (DIM * nc), nc, q.tf[b], q.sign, t,
                                                         q.jac + (size_t)item * (DIM * nc));
        if (q.jac_tf) q.jac_tf[item] = dtf;
    }
};

// obtg_jerk's rows, q(t) = sign (DIM/2) |c'''(t)|^2 + offset of a vehicle: AccelRows with the source curve one derivative
// further still (bern_device.h diff3_elev1_rows) and the block of the third derivative -- a copy beside AccelRows, not an
// order template over both: that form moved instructions in seven of the parent's k_accel_true_min kernels.
template <int NC_, int DIM>
struct JerkRows {
    using Params = SpeedExParams;
    static constexpr int NC = NC_, L = 2 * NC_ - 1;
    static __device__ __forceinline__ void coeffs(const Params& q, long item, double (&cf)[L])
    {
        const int b = (int)(item / q.n_veh);
        const double* v = q.Y + (size_t)item * (DIM * NC);
        const double val = (double)(NC - 1) / q.tf[b];
        double a[DIM][NC];
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            double x[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c] = v[d * NC + c];
            diff3_elev1_rows<NC>(x, val, a[d]);
        }
        normsq_coeffs<NC, DIM>(a, as_ctab(q.W2), cf);
    }
    static __device__ __forceinline__ void envelope(const Params& q, long item, int nc, double t)
    {
        const int b = (int)(item / q.n_veh);
        const double dtf = jerk_envelope_block<NC, DIM>(q.Y + (size_t)item * (DIM * nc), nc, q.tf[b], q.sign, t,
                                                         q.jac + (size_t)item * (DIM * nc));
        if (q.jac_tf) q.jac_tf[item] = dtf;
    }
};

struct KeepInExParams {
    const double* __restrict__ Y;      // [B][n_veh*DIM][NC]
    const double* __restrict__ H;      // [F][DIM + 1]: (a, b) of every half-space a . p <= b
    const int2* __restrict__ VF;       // [P]: (vehicle, face)
    ExParams ex;                       // outputs [B][P]; c unused
    double* __restrict__ jac;          // [B][P][DIM][NC] (the envelope forms)
    int n_veh, P;
    double sign, offset;               // the identity (1, 0)
};

// obtg_keep_in's rows at R = 0, g(t) = b_f - a_f . c_v(t) of a (vehicle, face) item: a polynomial of the curve's own degree, so
// L = NC (bern_device.h keep_in_coeff).  No span.  The envelope block does not read Y: g is linear in the control points.
template <int NC_, int DIM>
struct KeepInRows {
    using Params = KeepInExParams;
    static constexpr int NC = NC_, L = NC_;
    static __device__ __forceinline__ void coeffs(const Params& q, long item, double (&cf)[L])
    {
        const int b = (int)(item / q.P), it = (int)(item - (long)b * q.P);
        const int2 vf = q.VF[it];
        const double* v = q.Y + ((size_t)b * q.n_veh + vf.x) * (DIM * NC);
        const double* h = q.H + (size_t)vf.y * (DIM + 1);
#pragma unroll
        for (int i = 0; i < NC; ++i) cf[i] = keep_in_coeff<DIM>(h, v, NC, i);
    }
    static __device__ __forceinline__ void envelope(const Params& q, long item, int nc, double t)
    {
        const int it = (int)(item % q.P);
        keep_in_envelope_block<NC, DIM>(q.H + (size_t)q.VF[it].y * (DIM + 1), nc, t, q.jac + (size_t)item * (DIM * nc));
    }
};

struct AngExParams {
    const double* __restrict__ Y;      // [B][n_veh*2][NC]
    const double* __restrict__ tf;     // [B]
    const double* __restrict__ tab;    // C(n, .)[n+1], then 1 / C(2n, .)[2n+1] (capi.cpp ang_rows_table)
    ExParams ex;                       // outputs [B][n_veh][2]; c unused
    double* __restrict__ jac;          // [B][n_veh][2][2][NC] (the envelope forms)
    double* __restrict__ jac_tf;       // [B][n_veh][2], nullable
    int n_veh;
    double sign, offset;               // the identity (1, 0): W and the side enter in coeffs
    double W;                          // the bound on |angular rate|
};

// The true angular-rate rows: item = (row, vehicle, side), side 0: p_+ = W den - num (sigma = +1), side 1: p_- = W den + num.
// bern_device.h diff_elev1_at / ang_row_coeff define the coefficients (k_ang_rows below writes the same ones to memory);
// the envelope is the side's block over the vehicle's control points and its d/dtf.  DIM is 2: the family has no other.
template <int NC_, int DIM>
struct AngRows {
    using Params = AngExParams;
    static constexpr int NC = NC_, L = 2 * NC_ - 1;
    static __device__ __forceinline__ void coeffs(const Params& q, long item, double (&cf)[L])
    {
        constexpr int N = NC - 1;
        const long veh = item >> 1;
        const int b = (int)(veh / q.n_veh);
        const double sigma = (item & 1) ? -1.0 : 1.0;
        const double* v = q.Y + (size_t)veh * (2 * NC);
        const double val = (double)N / q.tf[b];
        const ctab_t Cn = as_ctab(q.tab), Sk = Cn + NC;
        double u1[2][NC], u2[2][NC];           // C(n, j) x'_j, C(n, j) y'_j;  C(n, j) x''_j, C(n, j) y''_j
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            double x[NC], x1[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c] = v[d * NC + c];
#pragma unroll
            for (int c = 0; c < NC; ++c) x1[c] = diff_elev1_at(x, c, N, val);
#pragma unroll
            for (int c = 0; c < NC; ++c) u2[d][c] = Cn[c] * diff_elev1_at(x1, c, N, val);
#pragma unroll
            for (int c = 0; c < NC; ++c) u1[d][c] = Cn[c] * x1[c];
        }
#pragma unroll
        for (int k = 0; k < L; ++k) cf[k] = ang_row_coeff(u1[0], u1[1], u2[0], u2[1], N, k, Sk[k], q.W, sigma);
    }
    static __device__ __forceinline__ void envelope(const Params& q, long item, int nc, double t)
    {
        const long veh = item >> 1;
        const int b = (int)(veh / q.n_veh);
        const double dtf = ang_envelope_block<NC>(q.Y + (size_t)veh * (2 * nc), nc, q.tf[b], q.W, (item & 1) ? -1.0 : 1.0, t,
                                                  q.jac + (size_t)item * (2 * nc));
        if (q.jac_tf) q.jac_tf[item] = dtf;
    }
};

// The fused kernel of a family F: one item per lane -- its coefficients, the output transform as one fma (sign is +-1: the
// product is exact, fused or not; this is the R = 0 row's value), the first step -- then the whole wave on each item that
// needs the search, in lane order; JAC: every lane writes its own envelope block at the t_star it holds.
template <class F, bool JAC>
__device__ __forceinline__ void true_min_body(const typename F::Params& q)
{
    constexpr int L = F::L;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    double* stk = lds + (size_t)wave * kExStack * (L + 3);
    const ExParams& p = q.ex;
    const long item = ((long)blockIdx.x * kExWaves + wave) * kWave + lane;
    const bool valid = item < p.M;
    double cf[L];
    F::coeffs(q, valid ? item : p.M - 1, cf);
    ExScan sc;
#pragma unroll
    for (int k = 0; k < L; ++k) { cf[k] = fma(q.sign, cf[k], q.offset); sc.put(cf[k], k); }
    ExOut mine;
    double tol;
    const bool need = !ex_first(sc, p.eps_rel, p.eps_abs, mine, tol) && valid;
    unsigned long long mask = __ballot(need);
    while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        double bb = INFINITY;
#pragma unroll
        for (int k = 0; k < L; ++k) { const double v = ex_lane(cf[k], src); if (lane == k) bb = v; }
        const ExOut o = wave_search(bb, L, ex_lane(tol, src), ex_lane(sc.c0, src), ex_lane(sc.cl, src), ex_lane(sc.m, src),
                                    p.max_nodes, stk);
        if (lane == src) mine = o;
    }
    if (valid) ex_store(p, item, mine, false);
    if (JAC && valid) F::envelope(q, item, F::NC, mine.t);
}

// The blocks alone, from the family's operands and the t_star of an earlier launch: one item per lane, nc <= kEnvMaxNC at
// run time (F is the family at NC = kEnvMaxNC)
constexpr int kEnvMaxNC = 32;
constexpr int kEnvThreads = 128;
template <class F>
__device__ __forceinline__ void envelope_body(const typename F::Params& q, const int nc)
{
    const long item = (long)blockIdx.x * kEnvThreads + threadIdx.x;
    if (item < q.ex.M) F::envelope(q, item, nc, q.ex.t[item]);
}

template <int NC, int DIM, bool JAC>
__global__ __launch_bounds__(kExWaves * kWave) void k_tsep_true_min(const TsepExParams q) { true_min_body<TsepRows<NC, DIM>, JAC>(q); }
template <int DIM>
__global__ __launch_bounds__(kEnvThreads) void k_tsep_envelope(const TsepExParams q, const int nc) { envelope_body<TsepRows<kEnvMaxNC, DIM>>(q, nc); }
template <int NC, int DIM, bool JAC>
__global__ __launch_bounds__(kExWaves * kWave) void k_speed_true_min(const SpeedExParams q) { true_min_body<SpeedRows<NC, DIM>, JAC>(q); }
template <int DIM>
__global__ __launch_bounds__(kEnvThreads) void k_speed_envelope(const SpeedExParams q, const int nc) { envelope_body<SpeedRows<kEnvMaxNC, DIM>>(q, nc); }
template <int NC, int DIM, bool JAC>
__global__ __launch_bounds__(kExWaves * kWave) void k_accel_true_min(const SpeedExParams q) { true_min_body<AccelRows<NC, DIM>, JAC>(q); }
template <int DIM>
__global__ __launch_bounds__(kEnvThreads) void k_accel_envelope(const SpeedExParams q, const int nc) { envelope_body<AccelRows<kEnvMaxNC, DIM>>(q, nc); }
template <int NC, int DIM, bool JAC>
__global__ __launch_bounds__(kExWaves * kWave) void k_jerk_true_min(const SpeedExParams q) { true_min_body<JerkRows<NC, DIM>, JAC>(q); }
template <int DIM>
__global__ __launch_bounds__(kEnvThreads) void k_jerk_envelope(const SpeedExParams q, const int nc) { envelope_body<JerkRows<kEnvMaxNC, DIM>>(q, nc); }
template <int NC, int DIM, bool JAC>
__global__ __launch_bounds__(kExWaves * kWave) void k_keep_in_true_min(const KeepInExParams q) { true_min_body<KeepInRows<NC, DIM>, JAC>(q); }
template <int DIM>
__global__ __launch_bounds__(kEnvThreads) void k_keep_in_envelope(const KeepInExParams q, const int nc) { envelope_body<KeepInRows<kEnvMaxNC, DIM>>(q, nc); }
template <int NC, bool JAC>
__global__ __launch_bounds__(kExWaves * kWave) void k_ang_true_min(const AngExParams q) { true_min_body<AngRows<NC, 2>, JAC>(q); }
__global__ __launch_bounds__(kEnvThreads) void k_ang_envelope(const AngExParams q, const int nc) { envelope_body<AngRows<kEnvMaxNC, 2>>(q, nc); }

// The angular-rate rows' polynomials to memory, any degree 1 .. 31: one wave per (row, vehicle), the derivative curves
// through LDS, lane k forms coefficient k of both sides with the functions the fused kernels use -- out[B][n_veh][2][2n+1].
// q.sign, q.offset: the fused body's output transform (the identity; fma(1, p, 0) takes a -0 to +0 there and so here).
__global__ __launch_bounds__(kWave) void k_ang_rows(const AngExParams q, const int nc, double* __restrict__ out)
{
    __shared__ double sh[6][kEnvMaxNC];       // x, y -> u1x, u1y after the last read; x', y'; u2x, u2y
    const long veh = blockIdx.x;
    const int b = (int)(veh / q.n_veh), lane = threadIdx.x, n = nc - 1, L = 2 * n + 1;
    const double val = (double)n / q.tf[b];
    const double* v = q.Y + (size_t)veh * (2 * nc);
    const double* Cn = q.tab;
    const double* Sk = Cn + nc;
    if (lane < nc) { sh[0][lane] = v[lane]; sh[1][lane] = v[nc + lane]; }
    __syncthreads();
    if (lane < nc)
        for (int d = 0; d < 2; ++d) sh[2 + d][lane] = diff_elev1_at(sh[d], lane, n, val);
    __syncthreads();
    if (lane < nc)
        for (int d = 0; d < 2; ++d) {
            sh[4 + d][lane] = Cn[lane] * diff_elev1_at(sh[2 + d], lane, n, val);
            sh[d][lane] = Cn[lane] * sh[2 + d][lane];
        }
    __syncthreads();
    if (lane < L)
        for (int side = 0; side < 2; ++side)
            out[((size_t)veh * 2 + side) * L + lane] =
                fma(q.sign, ang_row_coeff(sh[0], sh[1], sh[4], sh[5], n, lane, Sk[lane], q.W, side ? -1.0 : 1.0), q.offset);
}

// ---- the proximity family (obtg_proximity_poly, obtg_proximity_true[_jac]; include/obtg.h states the contract, DESIGN.md 4.28
// the reasoning): an item (a, b, kind, rho, tau0, tau1) of the context's table is vehicle a against vehicle b or point
// b - n_veh of the family's own point table, g = (DIM/2)(rho^2 - |c_a - c_b|^2) on the window (bern_device.h proximity_coeffs).
// kind OBTG_PROX_WITHIN takes the minimum of g, OBTG_PROX_REACH the maximum -- k_bern_extrema's want_max, per ITEM: the
// coefficients are negated going in, val and bound coming out, and the search's parameter t_w becomes the curve's,
// fma(t_w, tau1 - tau0, tau0).  That transform cannot ride on true_min_body's one (sign, offset) pair, so the family has a body
// of its own over ex_first / wave_search / ex_store (prox_body), and true_min_body stays as it is.  The envelope kernel is
// envelope_body's.
struct ProxExParams {
    const double* __restrict__ Y;      // [B][n_veh*DIM][NC]
    const double* __restrict__ pts;    // [Q][DIM]
    const int* __restrict__ items;     // [P][3]: a, b, kind
    const double* __restrict__ par;    // [P][3]: rho, tau0, tau1
    const double* __restrict__ W2;
    ExParams ex;                       // outputs [B][P]; c: the workspace rows of k_prox_search
    double* __restrict__ jac;          // [B][P][DIM][NC] (the envelope forms)
    double* __restrict__ rows;         // [B][P][2 NC - 1] (the rows kernels)
    int n_veh, P;
};

// the item's two curves as proximity_coeffs and envelope_block take them: b's element (c, i) is yb[c * b_cs + i * b_is]
struct ProxPair {
    const double* ya;
    const double* yb;
    int b_cs, b_is;
};
template <int DIM>
__device__ __forceinline__ ProxPair prox_pair(const ProxExParams& q, const int b, const int it, const int nc)
{
    const int ia = q.items[3 * it], ib = q.items[3 * it + 1];
    const double* Yrow = q.Y + (size_t)b * q.n_veh * (DIM * nc);
    const bool veh = ib < q.n_veh;
    return ProxPair{ Yrow + (size_t)ia * (DIM * nc), veh ? Yrow + (size_t)ib * (DIM * nc) : q.pts + (size_t)(ib - q.n_veh) * DIM,
                     veh ? nc : 1, veh ? 1 : 0 };
}

template <int NC_, int DIM>
struct ProxRows {
    using Params = ProxExParams;
    static constexpr int NC = NC_, L = 2 * NC_ - 1;
    static __device__ __forceinline__ void coeffs(const Params& q, long item, double (&cf)[L])
    {
        const int b = (int)(item / q.P), it = (int)(item - (long)b * q.P);
        const ProxPair pr = prox_pair<DIM>(q, b, it, NC);
        const double* w = q.par + 3 * it;
        proximity_coeffs<NC, DIM>(pr.ya, pr.yb, pr.b_cs, pr.b_is, w[0], w[1], w[2], as_ctab(q.W2), cf);
    }
    // the first object's block of g at the CURVE's parameter t, on the unrestricted control points: envelope_block negated (a
    // second vehicle's block is the exact negation and is not stored; a point has no variable)
    static __device__ __forceinline__ void envelope(const Params& q, long item, int nc, double t)
    {
        const int b = (int)(item / q.P), it = (int)(item - (long)b * q.P);
        const ProxPair pr = prox_pair<DIM>(q, b, it, nc);
        envelope_block<NC, DIM, true>(pr.ya, pr.yb, pr.b_cs, pr.b_is, nc, t, q.jac + (size_t)item * (DIM * nc));
    }
};

// the item's answer to memory; returns t_star, the CURVE's parameter of the search's t_w
__device__ __forceinline__ double prox_store(const ProxExParams& q, long item, ExOut o, bool neg)
{
    const double* w = q.par + 3 * (item % q.P);
    o.t = fma(o.t, w[2] - w[1], w[1]);
    ex_store(q.ex, item, o, neg);
    return o.t;
}

// MODE 0: the values; 1: the values and the blocks; 2: the coefficients to memory, no search (obtg_proximity_poly)
template <class F, int MODE>
__device__ __forceinline__ void prox_body(const ProxExParams& q)
{
    constexpr int L = F::L;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    double* stk = lds + (size_t)wave * kExStack * (L + 3);
    const ExParams& p = q.ex;
    const long item = ((long)blockIdx.x * kExWaves + wave) * kWave + lane;
    const bool valid = item < p.M;
    const long it = valid ? item : p.M - 1;
    double cf[L];
    F::coeffs(q, it, cf);
    if (MODE == 2) {
        if (valid) {
#pragma unroll
            for (int k = 0; k < L; ++k) q.rows[(size_t)item * L + k] = cf[k];
        }
        return;
    }
    const bool neg = q.items[3 * (it % q.P) + 2] != 0;
    ExScan sc;
#pragma unroll
    for (int k = 0; k < L; ++k) { cf[k] = neg ? -cf[k] : cf[k]; sc.put(cf[k], k); }
    ExOut mine;
    double tol;
    const bool need = !ex_first(sc, p.eps_rel, p.eps_abs, mine, tol) && valid;
    unsigned long long mask = __ballot(need);
    while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        double bb = INFINITY;
#pragma unroll
        for (int k = 0; k < L; ++k) { const double v = ex_lane(cf[k], src); if (lane == k) bb = v; }
        const ExOut o = wave_search(bb, L, ex_lane(tol, src), ex_lane(sc.c0, src), ex_lane(sc.cl, src), ex_lane(sc.m, src),
                                    p.max_nodes, stk);
        if (lane == src) mine = o;
    }
    if (valid) {
        const double t_star = prox_store(q, item, mine, neg);
        if (MODE == 1) F::envelope(q, item, F::NC, t_star);
    }
}

template <int NC, int DIM, int MODE>
__global__ __launch_bounds__(kExWaves * kWave) void k_prox_true(const ProxExParams q) { prox_body<ProxRows<NC, DIM>, MODE>(q); }
template <int DIM>
__global__ __launch_bounds__(kEnvThreads) void k_prox_envelope(const ProxExParams q, const int nc) { envelope_body<ProxRows<kEnvMaxNC, DIM>>(q, nc); }

// The family's rows for the counts without a kernel of their own, any degree 1 .. 31: one wave per item, lane i holds control
// point i.  The window's cuts are window_row's levels lane-parallel (a level reads only values of the level before), then the
// difference and the product in the any-degree separation kernel's arithmetic (bern_kernels.hip k_generic_normsq_elev, R = 0):
// ah = (x - y) C(n, i), c_k = (DIM/2) sum_q conv_at(ah_q, ah_q, k) / C(2n, k) -- so a full-window item is fma(-1, ., off) of
// obtg_temporal_sep's R = 0 row on those degrees too.  bn, b2n: the binomial rows C(n, .) and C(2n, .).
__device__ __forceinline__ double prox_window_lane(double v, const SpanCut& s, const int nc, const int lane)
{
    if (s.head) {
        const double z = s.zh, w = 1.0 - z;
        for (int lev = 1; lev < nc; ++lev) {
            const double up = __shfl_down(v, 1);
            if (lane < nc - lev) v = w * v + z * up;
        }
    }
    if (s.tail) {
        const double z = s.zt, w = 1.0 - z;
        for (int lev = 1; lev < nc; ++lev) {
            const double dn = __shfl_up(v, 1);
            if (lane >= lev && lane < nc) v = w * dn + z * v;
        }
    }
    return v;
}

template <int DIM>
__global__ __launch_bounds__(kWave) void k_prox_rows(const ProxExParams q, const int nc, const double* __restrict__ bn,
                                                     const double* __restrict__ b2n)
{
    __shared__ double ah[DIM][kEnvMaxNC];
    const long item = blockIdx.x;
    const int lane = threadIdx.x, n = nc - 1, L = 2 * n + 1;
    const int b = (int)(item / q.P), it = (int)(item - (long)b * q.P);
    const ProxPair pr = prox_pair<DIM>(q, b, it, nc);
    const double* w = q.par + 3 * it;
    const SpanCut cut(0.0, 1.0, w[1], w[2]);            // (the whole wave: the window belongs to the item)
    const int i = lane < nc ? lane : 0;
    for (int d = 0; d < DIM; ++d) {
        double x = pr.ya[d * nc + i], y = pr.yb[d * pr.b_cs + i * pr.b_is];
        x = prox_window_lane(x, cut, nc, lane);
        if (pr.b_is) y = prox_window_lane(y, cut, nc, lane);
        if (lane < nc) ah[d][lane] = (x - y) * bn[lane];
    }
    __syncthreads();
    if (lane < L) {
        double s = 0.0;
        for (int d = 0; d < DIM; ++d) s += conv_at(ah[d], nc, ah[d], nc, lane);
        const double c = (0.5 * DIM) * s / b2n[lane];
        q.rows[(size_t)item * L + lane] = fma(-1.0, c, proximity_offset<DIM>(w[0]));
    }
}

// k_bern_extrema on the family's workspace rows q.ex.c[M][K], want_max and the window per item
__global__ __launch_bounds__(kExWaves * kWave) void k_prox_search(const ProxExParams q)
{
    extern __shared__ double lds[];
    const ExParams& p = q.ex;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    double* stk = lds + (size_t)wave * kExStack * (p.K + 3);
    const long row0 = ((long)blockIdx.x * kExWaves + wave) * kWave;
    const long row = row0 + lane;
    const bool valid = row < p.M;
    const long rr = valid ? row : p.M - 1;
    const bool neg = q.items[3 * (rr % q.P) + 2] != 0;
    const double* cr = p.c + rr * p.K;
    ExScan sc;
    for (int k = 0; k < p.K; ++k) { const double v = cr[k]; sc.put(neg ? -v : v, k); }
    ExOut mine;
    double tol;
    const bool need = !ex_first(sc, p.eps_rel, p.eps_abs, mine, tol) && valid;
    unsigned long long mask = __ballot(need);
    while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const double* cs = p.c + (row0 + src) * p.K;
        const bool sneg = __shfl((int)neg, src) != 0;
        double b = INFINITY;
        if (lane < p.K) { const double v = cs[lane]; b = sneg ? -v : v; }
        const ExOut o = wave_search(b, p.K, ex_lane(tol, src), ex_lane(sc.c0, src), ex_lane(sc.cl, src), ex_lane(sc.m, src),
                                    p.max_nodes, stk);
        if (lane == src) mine = o;
    }
    if (valid) prox_store(q, row, mine, neg);
}

// =====================================================================================
//  the curvature rows, planar (dim 2) and in space (dim 3): kappa = mag / den^(3/2) is not a polynomial -- the planar one's
//  polynomial form has 6n + 1 coefficients, more than a row of lanes from degree 11 on; the norm of the space one's numerator
//  has none -- so the two families have a search of their own over an item's NP polynomials at once, den last
//  (include/obtg.h obtg_curvature_true_min and obtg_space_curvature_true_min state the contracts; DESIGN.md 4.21, 4.22 the
//  reasoning).  One body, written over a policy that says what a family's own is (PlanarCurv, SpaceCurv3 below):
//
//    planar   NP = 2: (sigma num, den), num = x' y'' - y' x''.  An item is (row, vehicle, side); sigma = +1 / -1 for side 0 / 1
//             multiplies num once, when the coefficients are formed, and the search MAXIMISES sigma kappa.  mag = sigma num.
//    space    NP = 4: (wx, wy, wz, den), w = c' x c''.  An item is (row, vehicle); mag = |(wx, wy, wz)|, the norm of a vector
//             of polynomials: without a sign, so no sides and no clamp logic, and the incumbent starts at 0.
//
//  The shape is wave_search's: the first step one lane per item, an item that needs the search gets the wave, lane k holds
//  coefficient k of the NP polynomials, a de Casteljau level is the same pair of averages on each of them, the pieces are taken
//  as wave_search takes them, waiting sub-curves are frames of NP K + 3 doubles (the polynomials | bound, t0, width) in LDS.
//  Incumbent U: the largest value met at an end of [0, 1] or at a bisection midpoint (curv_kappa).  Upper bound of a node
//  (curv_node_bound): the tangent of the convex den^(3/2) at the node's mid-range under every coefficient's mag, which for the
//  space family bounds |w(t)| by the norm's convexity, |w(t)| <= sum |w_k| B_k(t).  A node with bound - U <= the family's
//  tolerance is closed; of two open children the one with the larger bound is followed.
// =====================================================================================
constexpr int kCvWaves = 1;           // waves per workgroup: K = 63 is 33 KB (planar) or 64 KB (space) of frames per wave, and the
                                      // in-register first step wants the whole register file of a SIMD lane (launch bound 64: 512 VGPRs)
constexpr int kCvMaxNC = 32;

struct CvOut {
    double val, t;                     // the incumbent and where it was met
    int status;
};

struct CurvParams {
    const double* __restrict__ Y;      // [curves][DIM][nc]: the vehicles (curves) in item order, SIDES items per curve
    const double* __restrict__ tab;    // C(n, .)[n+1], then 1 / C(2n, .)[2n+1] (capi.cpp ang_rows_table)
    const double* __restrict__ rows;   // [curves][NP][2n+1], den last (k_curv_rows, k_scurv_rows): the workspace form's operand
    double* __restrict__ val;          // [items]: max_curv - the maximum;  free curves: k_max[curves]
    double* __restrict__ t;            // [items] nullable;                 free curves: t_max[curves]
    double* __restrict__ val1;         // free planar curves: k_min[curves], t_min[curves]; null otherwise
    double* __restrict__ t1;
    int* __restrict__ status;          // [items] nullable
    double* __restrict__ jac;          // [items][DIM][nc] (the envelope forms)
    long M;                            // items
    int nc, max_nodes, free_curve;     // free_curve: the extrema themselves are written (obtg_bern_[space_]curvature, W = 0), no clamp
    double W, eps_rel;                 // W = max_curv
};

__device__ __forceinline__ double cv_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// mag / den^(3/2) at a point, NaN where the point offers no incumbent: den <= 0, or a quotient that is not finite
__device__ __forceinline__ double curv_kappa(double mag, double den)
{
    if (!(den > 0.0)) return __builtin_nan("");
    const double k = mag / (den * __builtin_sqrt(den));
    return fabs(k) <= DBL_MAX ? k : __builtin_nan("");
}

// One coefficient's share of a node's bound, given the node's dmin and dmax: d0 = 0.5 (dmin + dmax),
// g_k = fma(1.5 sqrt(d0), den_k, -0.5 (d0 sqrt(d0))) is the tangent of den^(3/2) at d0 -- below the convex function, so
// sum g_k B_k(t) <= den(t)^(3/2) -- and lambda g_k - mag_k >= 0 for EVERY k gives kappa <= lambda.  A coefficient with
// mag_k <= 0 meets that for every lambda >= 0 only if its g_k >= 0, and a g_k <= 0 beside a positive mag_k breaks it, so the
// rule needs g > 0 at dmin (g is increasing in den: that is every g_k > 0; it fails once dmax >= 5 dmin, where the tangent at
// the mid-range is below 0 at dmin).  Then the bound is the largest mag_k / g_k over mag_k > 0.  +inf where g at dmin is <= 0 or
// dmin <= 0.  What a coefficient with mag_k <= 0 contributes is the family's (ratio).  max is exact, so the order of the
// reduction does not enter.
__device__ __forceinline__ double curv_tangent_ratio(double mag, double den, double dmin, double dmax)
{
    if (!(dmin > 0.0)) return INFINITY;
    const double d0 = 0.5 * (dmin + dmax), s0 = __builtin_sqrt(d0);
    const double a = 1.5 * s0, c = -0.5 * (d0 * s0);
    return fma(a, dmin, c) > 0.0 ? mag / fma(a, den, c) : INFINITY;
}

// A family's policy.  NP polynomials per item, den last; DIM coordinates; SIDES items per curve (2: polynomial 0 is signed).
//   curve, sigma     the item's curve and sign
//   coeff            coefficient k of the curve's polynomials, unsigned, from u1 = C(n, .) c', u2 = C(n, .) c'': THE definition
//                    of the rows (bern_device.h), for the in-register kernel and the rows kernel alike
//   mag              a coefficient's or a point's numerator
//   start, tol       the incumbent before any point is met; when bound - U closes a node
//   bound            a node's bound from max_over(share, idle): the largest share(mag_k, den_k) over its coefficients, idle
//                    where there is none (a lane past K)
//   store            the item's answer to memory; returns the row's value
//   block            the item's envelope block (bern_device.h)
struct PlanarCurv {
    static constexpr int NP = 2, DIM = 2, SIDES = 2;
    static __device__ __forceinline__ long curve(long item) { return item >> 1; }
    static __device__ __forceinline__ double sigma(long item) { return (item & 1) ? -1.0 : 1.0; }
    template <int R>
    static __device__ __forceinline__ void coeff(const double (*u1)[R], const double (*u2)[R], int n, int k, double sk, double (&c)[NP])
    {
        const NumDen r = curvature_row_coeff(u1[0], u1[1], u2[0], u2[1], n, k, sk);
        c[0] = r.num; c[1] = r.den;
    }
    static __device__ __forceinline__ double mag(const double (&c)[NP]) { return c[0]; }
    // a free curve's incumbent is -inf until a point offers a value: it does not enter the tolerance, and the search goes on
    static __device__ __forceinline__ double start(bool clamp) { return clamp ? 0.0 : -INFINITY; }
    static __device__ __forceinline__ double tol(double W, double eps_rel, double U) { return eps_rel * fmax(W, U > -INFINITY ? fabs(U) : 0.0); }
    // -inf stands for "no num_k > 0": the clamp or the chord answers that case
    static __device__ __forceinline__ double ratio(double num, double den, double dmin, double dmax)
    {
        return num > 0.0 ? curv_tangent_ratio(num, den, dmin, dmax) : -INFINITY;
    }
    // No num_k > 0 on the node.  A clamped row: sigma kappa <= 0 there, the bound is 0.  A free curve needs a bound below 0 that
    // converges as fast: the chord of den^(3/2) over [dmin, dmax] lies above it, h_k = fma(slope, den_k - dmin, dmin sqrt(dmin)),
    // slope = (dmax + sqrt(dmax dmin) + dmin) / (sqrt(dmax) + sqrt(dmin)), and num / den^(3/2) <= num / h for num <= 0: the
    // bound is the largest num_k / h_k (dmin <= 0: 0).
    static __device__ __forceinline__ double chord_ratio(double num, double den, double dmin, double dmax)
    {
        if (!(dmin > 0.0)) return 0.0;
        const double a = __builtin_sqrt(dmax), b = __builtin_sqrt(dmin);
        const double slope = ((dmax + a * b) + dmin) / (a + b);
        return num / fma(slope, den - dmin, dmin * b);
    }
    template <class MaxOver>
    static __device__ __forceinline__ double bound(const MaxOver& max_over, double dmin, double dmax, bool clamp)
    {
        double ub = max_over([&](double num, double den) { return ratio(num, den, dmin, dmax); }, -INFINITY);
        if (ub == -INFINITY)
            ub = clamp ? 0.0 : max_over([&](double num, double den) { return chord_ratio(num, den, dmin, dmax); }, -INFINITY);
        return ub;
    }
    // row = max_curv - m_sigma; a free curve's sides are k_max = m_+ and k_min = -m_-.  A free curve on which no point offered
    // an incumbent (den <= 0 at every point met) has no curvature to report: NaN.
    static __device__ __forceinline__ double store(const CurvParams& q, long item, CvOut o)
    {
        double v;
        if (q.free_curve) {
            if (o.val == -INFINITY) o.val = o.t = __builtin_nan("");
            const long m = item >> 1;
            v = (item & 1) ? -o.val : o.val;
            ((item & 1) ? q.val1 : q.val)[m] = v;
            ((item & 1) ? q.t1 : q.t)[m] = o.t;
        } else {
            v = q.W - o.val;
            q.val[item] = v;
            if (q.t) q.t[item] = o.t;
        }
        if (q.status) q.status[item] = o.status;
        return v;
    }
    template <int NCMAX>
    static __device__ __forceinline__ void block(const double* y, int nc, double sigma, double t, double* o)
    {
        curvature_envelope_block<NCMAX>(y, nc, sigma, t, o);
    }
};

struct SpaceCurv3 {
    static constexpr int NP = 4, DIM = 3, SIDES = 1;
    static __device__ __forceinline__ long curve(long item) { return item; }
    static __device__ __forceinline__ double sigma(long) { return 1.0; }
    template <int R>
    static __device__ __forceinline__ void coeff(const double (*u1)[R], const double (*u2)[R], int n, int k, double sk, double (&c)[NP])
    {
        const SpaceCurv r = space_curvature_row_coeff(u1[0], u1[1], u1[2], u2[0], u2[1], u2[2], n, k, sk);
        c[0] = r.wx; c[1] = r.wy; c[2] = r.wz; c[3] = r.den;
    }
    static __device__ __forceinline__ double mag(const double (&c)[NP]) { return space_curvature_norm(c[0], c[1], c[2]); }
    static __device__ __forceinline__ double start(bool) { return 0.0; }
    static __device__ __forceinline__ double tol(double W, double eps_rel, double U) { return eps_rel * fmax(W, U); }
    // 0 where nu is 0: the coefficient meets lambda g_k - nu_k >= 0 for every lambda >= 0 wherever the rule holds, and a node of
    // such coefficients alone has w == 0
    static __device__ __forceinline__ double ratio(double nu, double den, double dmin, double dmax)
    {
        return nu == 0.0 ? 0.0 : curv_tangent_ratio(nu, den, dmin, dmax);
    }
    template <class MaxOver>
    static __device__ __forceinline__ double bound(const MaxOver& max_over, double dmin, double dmax, bool)
    {
        return max_over([&](double nu, double den) { return ratio(nu, den, dmin, dmax); }, 0.0);
    }
    // row = max_curv - max kappa (a free curve: max kappa itself)
    static __device__ __forceinline__ double store(const CurvParams& q, long item, const CvOut& o)
    {
        const double v = q.free_curve ? o.val : q.W - o.val;
        q.val[item] = v;
        if (q.t) q.t[item] = o.t;
        if (q.status) q.status[item] = o.status;
        return v;
    }
    template <int NCMAX>
    static __device__ __forceinline__ void block(const double* y, int nc, double, double t, double* o)
    {
        space_curvature_envelope_block<NCMAX>(y, nc, t, o);
    }
};

// f(p) for p = 0 .. NP - 1 with p a constant of the language: no loop is left for the optimiser to unroll
template <class F, int... P>
__device__ __forceinline__ void curv_each_(const F& f, std::integer_sequence<int, P...>) { (f(std::integral_constant<int, P>()), ...); }
template <int NP, class F>
__device__ __forceinline__ void curv_each(const F& f) { curv_each_(f, std::make_integer_sequence<int, NP>()); }

// the whole wave on one node: lane k < K holds coefficient k; the same value in every lane
template <class Fam>
__device__ __forceinline__ double curv_node_bound(const double (&b)[Fam::NP], bool act, bool clamp)
{
    const double den = b[Fam::NP - 1];
    const double dmin = ex_wave_min(act ? den : INFINITY), dmax = cv_wave_max(act ? den : -INFINITY);
    return Fam::bound([&](auto share, double idle) { return cv_wave_max(act ? share(Fam::mag(b), den) : idle); }, dmin, dmax, clamp);
}

// The first step of an item (node 1), one lane: get(k, c) puts its coefficient k into c (signed).  true: `o` is the item's
// answer; false: the search has to run from (o.val, o.t) as the incumbent.
template <class Fam, int KC, class Get>
__device__ __forceinline__ bool curv_first(const Get& get, int K, double W, double eps_rel, bool clamp, CvOut& o)
{
    constexpr int NP = Fam::NP;
    if (KC > 0) K = KC;
    bool bad = false, any = false;
    double dmin = INFINITY, dmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < (KC > 0 ? KC : K); ++k) {
        double c[NP];
        get(k, c);
#pragma unroll
        for (int p = 0; p < NP; ++p) bad = bad || !(fabs(c[p]) <= DBL_MAX);
#pragma unroll
        for (int p = 0; p < NP - 1; ++p) any = any || c[p] != 0.0;
        dmin = fmin(dmin, c[NP - 1]); dmax = fmax(dmax, c[NP - 1]);
    }
    o.status = OBTG_MD_OK;
    if (bad) { o.val = o.t = __builtin_nan(""); return true; }
    o.val = 0.0; o.t = 0.0;
    if (!any) return true;                  // the numerator == 0 identically: a straight path, degree 1, a vehicle at rest
    o.val = Fam::start(clamp);
    double c0[NP], c1[NP];
    get(0, c0); get(K - 1, c1);
    const double k0 = curv_kappa(Fam::mag(c0), c0[NP - 1]), k1 = curv_kappa(Fam::mag(c1), c1[NP - 1]);
    if (k0 > o.val) { o.val = k0; o.t = 0.0; }
    if (k1 > o.val) { o.val = k1; o.t = 1.0; }
    const double ub = Fam::bound([&](auto share, double idle) {
        double m = idle;
#pragma unroll
        for (int k = 0; k < (KC > 0 ? KC : K); ++k) { double c[NP]; get(k, c); m = fmax(m, share(Fam::mag(c), c[NP - 1])); }
        return m;
    }, dmin, dmax, clamp);
    return !(ub - o.val > Fam::tol(W, eps_rel, o.val));
}

// The whole wave on ONE item (every lane must be here).  Lane k < K holds coefficient k in b0; (U, tU): the first step's
// incumbent.  stk: this wave's kExStack x (NP K + 3) doubles.  Every scalar below is the same in all lanes.
template <class Fam>
__device__ __forceinline__ CvOut curv_wave_search(const double (&b0)[Fam::NP], const int K, const double W, const double eps_rel,
                                                  const bool clamp, double U, double tU, const int max_nodes, double* stk)
{
    constexpr int NP = Fam::NP;
    const int lane = threadIdx.x & (kWave - 1);
    const bool act = lane < K;
    const int pitch = NP * K + 3;
    double b[NP];                      // the search's own copy: written through the caller's array it costs registers
#pragma unroll
    for (int p = 0; p < NP; ++p) b[p] = b0[p];
    double t0 = 0.0, w = 1.0;
    int nodes = 1, sp = 0, status = OBTG_MD_OK;
    for (;;) {
        if (nodes + 2 > max_nodes) { status = OBTG_MD_NODE_CAP; break; }
        // deCasteljau at 1/2 of the NP polynomials, both pieces: l is lane 0's value after level r in lane r, b lane i's
        double l[NP], m[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) { l[p] = b[p]; m[p] = ex_lane0(b[p]); }
        for (int r = 1; r < K; ++r) {
            double up[NP];
            curv_each<NP>([&](auto p) { up[p] = wave_next_lane(b[p]); });
            const bool below = lane <= K - 1 - r;
            curv_each<NP>([&](auto p) { b[p] = below ? 0.5 * b[p] + 0.5 * up[p] : b[p]; });
            curv_each<NP>([&](auto p) { m[p] = ex_lane0(b[p]); });
            if (lane == r) curv_each<NP>([&](auto p) { l[p] = m[p]; });
        }
        const double hw = 0.5 * w, tm = t0 + hw;
        nodes += 2;
        const double km = curv_kappa(Fam::mag(m), m[NP - 1]);
        if (km > U) { U = km; tU = tm; }
        const double tol = Fam::tol(W, eps_rel, U);
        const double ubL = curv_node_bound<Fam>(l, act, clamp), ubR = curv_node_bound<Fam>(b, act, clamp);
        const bool aliveL = ubL - U > tol, aliveR = ubR - U > tol;
        if (aliveL && aliveR) {
            if (sp == kExStack) { status = OBTG_MD_DEPTH_CAP; break; }
            const bool go_left = ubL >= ubR;
            double* f = stk + sp * pitch;
            if (act) {
#pragma unroll
                for (int p = 0; p < NP; ++p) f[p * K + lane] = go_left ? b[p] : l[p];
            }
            if (lane == 0) { f[NP * K] = go_left ? ubR : ubL; f[NP * K + 1] = go_left ? tm : t0; f[NP * K + 2] = hw; }
            ++sp;
            if (go_left) {
#pragma unroll
                for (int p = 0; p < NP; ++p) b[p] = l[p];
            } else t0 = tm;
            w = hw;
        } else if (aliveL) {
#pragma unroll
            for (int p = 0; p < NP; ++p) b[p] = l[p];
            w = hw;
        } else if (aliveR) { t0 = tm; w = hw; }
        else {
            bool found = false;
            wave_sync();
            while (sp > 0) {
                --sp;
                const double* f = stk + sp * pitch;
                if (f[NP * K] - U > tol) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) b[p] = act ? f[p * K + lane] : 0.0;
                    t0 = f[NP * K + 1]; w = f[NP * K + 2];
                    found = true;
                    break;
                }
            }
            wave_sync();
            if (!found) break;
        }
    }
    CvOut o;
    o.val = U; o.t = tU; o.status = status;
    return o;
}

// The item's block from Y at the t_star and the row value an earlier step left: zero where the row IS max_curv (the maximum
// is 0: the clamp, a straight path, degree 1, a vehicle at rest), NaN for a NaN t_star, the family's block otherwise.
template <class Fam, int NCMAX>
__device__ __forceinline__ void curv_envelope(const CurvParams& q, long item, int nc, double row, double t)
{
    double* o = q.jac + (size_t)item * (Fam::DIM * nc);
    if (row == q.W || !(t == t)) {
        const double fill = t == t ? 0.0 : t;
        for (int e = 0; e < Fam::DIM * nc; ++e) o[e] = fill;
        return;
    }
    Fam::template block<NCMAX>(q.Y + (size_t)Fam::curve(item) * (Fam::DIM * nc), nc, Fam::sigma(item), t, o);
}

// What both kernel forms do once an item's first step is known: the wave on every item that needs it, in lane order; `load`
// puts item src's coefficients into the lanes.
template <class Fam, class Load>
__device__ __forceinline__ void curv_search_items(const CurvParams& q, const Load& load, int K, bool need, CvOut& mine, double* stk)
{
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long mask = __ballot(need);
    while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        double b[Fam::NP];
#pragma unroll
        for (int p = 0; p < Fam::NP; ++p) b[p] = 0.0;
        load(src, b);
        const CvOut o = curv_wave_search<Fam>(b, K, q.W, q.eps_rel, !q.free_curve, ex_lane(mine.val, src), ex_lane(mine.t, src), q.max_nodes, stk);
        if (lane == src) mine = o;
    }
}

// Coefficients in registers, one launch (the counts of OBTG_NC_CURV_LIST / OBTG_NC_SCURV_LIST): one lane forms its item's
// NP (2n + 1) coefficients -- AngRows::coeffs on T = 1 with the family's coeff --, then the steps above; JAC: every lane writes
// its own block.
template <class Fam, int NC, bool JAC>
__device__ __forceinline__ void curv_true_min_body(const CurvParams& q)
{
    constexpr int N = NC - 1, L = 2 * NC - 1, NP = Fam::NP, DIM = Fam::DIM;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    double* stk = lds + (size_t)wave * kExStack * (NP * L + 3);
    const long item = ((long)blockIdx.x * kCvWaves + wave) * kWave + lane;
    const bool valid = item < q.M;
    const long it = valid ? item : q.M - 1;
    const double sigma = Fam::sigma(it);
    const double* v = q.Y + (size_t)Fam::curve(it) * (DIM * NC);
    const ctab_t Cn = as_ctab(q.tab), Sk = Cn + NC;
    double co[NP][L];
    {
        double u1[DIM][NC], u2[DIM][NC];       // C(n, j) c'_j;  C(n, j) c''_j
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            double x[NC], x1[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c] = v[d * NC + c];
#pragma unroll
            for (int c = 0; c < NC; ++c) x1[c] = diff_elev1_at(x, c, N, (double)N);
#pragma unroll
            for (int c = 0; c < NC; ++c) u2[d][c] = Cn[c] * diff_elev1_at(x1, c, N, (double)N);
#pragma unroll
            for (int c = 0; c < NC; ++c) u1[d][c] = Cn[c] * x1[c];
        }
#pragma unroll
        for (int k = 0; k < L; ++k) {
            double c[NP];
            Fam::coeff(u1, u2, N, k, Sk[k], c);
            if constexpr (Fam::SIDES == 2) c[0] = sigma * c[0];
#pragma unroll
            for (int p = 0; p < NP; ++p) co[p][k] = c[p];
        }
    }
    CvOut mine;
    const bool need = !curv_first<Fam, L>([&](int k, double (&c)[NP]) {
#pragma unroll
        for (int p = 0; p < NP; ++p) c[p] = co[p][k];
    }, L, q.W, q.eps_rel, !q.free_curve, mine) && valid;
    curv_search_items<Fam>(q, [&](int src, double (&b)[NP]) {
#pragma unroll
        for (int k = 0; k < L; ++k) {
            double a[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) a[p] = ex_lane(co[p][k], src);
            if (lane == k) {
#pragma unroll
                for (int p = 0; p < NP; ++p) b[p] = a[p];
            }
        }
    }, L, need, mine, stk);
    if (valid) {
        const double row = Fam::store(q, item, mine);
        if (JAC) curv_envelope<Fam, NC>(q, item, NC, row, mine.t);
    }
}

// The workspace form, any degree 1 .. 31: the coefficients are the rows kernel's rows in memory, K = 2 nc - 1 at run time
template <class Fam>
__device__ __forceinline__ void curv_search_body(const CurvParams& q)
{
    constexpr int NP = Fam::NP;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, K = 2 * q.nc - 1;
    double* stk = lds + (size_t)wave * kExStack * (NP * K + 3);
    const long item0 = ((long)blockIdx.x * kCvWaves + wave) * kWave, item = item0 + lane;
    const bool valid = item < q.M;
    const long it = valid ? item : q.M - 1;
    // coefficient k of item i, signed
    const auto coef = [&](long i, int k, double (&c)[NP]) {
        const double* r = q.rows + (size_t)Fam::curve(i) * (NP * K);
#pragma unroll
        for (int p = 0; p < NP; ++p) c[p] = r[p * K + k];
        if constexpr (Fam::SIDES == 2) c[0] = Fam::sigma(i) * c[0];
    };
    CvOut mine;
    const bool need = !curv_first<Fam, 0>([&](int k, double (&c)[NP]) { coef(it, k, c); }, K, q.W, q.eps_rel, !q.free_curve, mine) && valid;
    curv_search_items<Fam>(q, [&](int src, double (&b)[NP]) { if (lane < K) coef(item0 + src, lane, b); }, K, need, mine, stk);
    if (valid) Fam::store(q, item, mine);
}

// The rows' polynomials to memory, any degree 1 .. 31: k_ang_rows on T = 1 without a side -- one wave per vehicle (curve),
// lane k forms coefficient k of the NP polynomials with the function the in-register kernels use: out[.][NP][2n+1].
template <class Fam>
__device__ __forceinline__ void curv_rows_body(const CurvParams& q, double* __restrict__ out)
{
    constexpr int NP = Fam::NP, DIM = Fam::DIM;
    __shared__ double sh[3 * DIM][kCvMaxNC];     // c -> u1 after the last read; c'; u2
    const long veh = blockIdx.x;
    const int lane = threadIdx.x, nc = q.nc, n = nc - 1, L = 2 * n + 1;
    const double val = (double)n;
    const double* v = q.Y + (size_t)veh * (DIM * nc);
    const double* Cn = q.tab;
    const double* Sk = Cn + nc;
    if (lane < nc)
        for (int d = 0; d < DIM; ++d) sh[d][lane] = v[d * nc + lane];
    __syncthreads();
    if (lane < nc)
        for (int d = 0; d < DIM; ++d) sh[DIM + d][lane] = diff_elev1_at(sh[d], lane, n, val);
    __syncthreads();
    if (lane < nc)
        for (int d = 0; d < DIM; ++d) {
            sh[2 * DIM + d][lane] = Cn[lane] * diff_elev1_at(sh[DIM + d], lane, n, val);
            sh[d][lane] = Cn[lane] * sh[DIM + d][lane];
        }
    __syncthreads();
    if (lane < L) {
        double c[NP];
        Fam::coeff(sh, sh + 2 * DIM, n, lane, Sk[lane], c);
        double* o = out + (size_t)veh * NP * L + lane;
#pragma unroll
        for (int p = 0; p < NP; ++p) o[p * L] = c[p];
    }
}

// the kernels: the bodies above under the names the host (and a profile) knows them by
template <int NC, bool JAC>
__global__ __launch_bounds__(kCvWaves * kWave) void k_curv_true_min(const CurvParams q) { curv_true_min_body<PlanarCurv, NC, JAC>(q); }
__global__ __launch_bounds__(kCvWaves * kWave) void k_curv_search(const CurvParams q) { curv_search_body<PlanarCurv>(q); }
__global__ __launch_bounds__(kWave) void k_curv_rows(const CurvParams q, double* __restrict__ out) { curv_rows_body<PlanarCurv>(q, out); }
template <int NC, bool JAC>
__global__ __launch_bounds__(kCvWaves * kWave) void k_scurv_true_min(const CurvParams q) { curv_true_min_body<SpaceCurv3, NC, JAC>(q); }
__global__ __launch_bounds__(kCvWaves * kWave) void k_scurv_search(const CurvParams q) { curv_search_body<SpaceCurv3>(q); }
__global__ __launch_bounds__(kWave) void k_scurv_rows(const CurvParams q, double* __restrict__ out) { curv_rows_body<SpaceCurv3>(q, out); }

// The blocks alone, from Y, the rows' values and their t_star: one item per lane, nc <= kCvMaxNC at run time
template <class Fam>
__device__ __forceinline__ void curv_envelope_body(const CurvParams& q)
{
    const long item = (long)blockIdx.x * kEnvThreads + threadIdx.x;
    if (item < q.M) curv_envelope<Fam, kCvMaxNC>(q, item, q.nc, q.val[item], q.t[item]);
}
__global__ __launch_bounds__(kEnvThreads) void k_curv_envelope(const CurvParams q) { curv_envelope_body<PlanarCurv>(q); }
__global__ __launch_bounds__(kEnvThreads) void k_scurv_envelope(const CurvParams q) { curv_envelope_body<SpaceCurv3>(q); }

// =====================================================================================
//  launchers
// =====================================================================================
bool bern_extrema_supported(int K) { return K >= 1 && K <= kExMaxK; }

int launch_bern_extrema(obtg_ctx* c, const double* d_c, long M, int K, int want_max, double eps_rel, double eps_abs,
                        int max_nodes, double* d_val, double* d_t, double* d_bound, int* d_nodes, int* d_status, int kernel_id)
{
    if (M <= 0) return OBTG_OK;
    if (!bern_extrema_supported(K)) return OBTG_ERR_ARG;
    ExParams p{};
    p.c = d_c; p.val = d_val; p.t = d_t; p.bound = d_bound; p.nodes = d_nodes; p.status = d_status;
    p.M = M; p.K = K; p.want_max = want_max; p.max_nodes = max_nodes; p.eps_rel = eps_rel; p.eps_abs = eps_abs;
    const size_t lds = sizeof(double) * kExWaves * kExStack * (size_t)(K + 3);
    const long per_wg = kExWaves * kWave;
    ScopedKernelTimer t(c, kernel_id);
    hipLaunchKernelGGL(k_bern_extrema, dim3((unsigned)((M + per_wg - 1) / per_wg)), dim3(kExWaves * kWave), lds, c->stream, p);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

// The host side of a device family: its kernels by shape, and its parameter block from the context and the descriptor
// (everything but ex and the outputs, which the launchers below set for every family alike)
template <template <int, int> class Rows> struct RowKernels;
template <> struct RowKernels<TsepRows> {
    template <int NC, int DIM, bool JAC> static auto fused() { return k_tsep_true_min<NC, DIM, JAC>; }
    template <int DIM> static auto envelope() { return k_tsep_envelope<DIM>; }
    static TsepExParams params(const obtg_ctx* c, const RowFamily& f, const double* dY, double* d_jac, double*)
    {
        TsepExParams q{};
        q.Y = dY; q.obs = c->d_obs.as<double>(); q.pairs = c->d_pairs.as<int2>(); q.W2 = c->d_w2.as<double>();
        q.n_veh = c->n_veh; q.P = f.items; q.jac = d_jac; q.sign = f.sign; q.offset = f.offset;
        return q;
    }
};
template <> struct RowKernels<SpeedRows> {
    template <int NC, int DIM, bool JAC> static auto fused() { return k_speed_true_min<NC, DIM, JAC>; }
    template <int DIM> static auto envelope() { return k_speed_envelope<DIM>; }
    static SpeedExParams params(const obtg_ctx* c, const RowFamily& f, const double* dY, double* d_jac, double* d_jac_tf)
    {
        SpeedExParams q{};
        q.Y = dY; q.tf = f.d_tf; q.W2 = c->d_w2.as<double>(); q.n_veh = c->n_veh; q.jac = d_jac; q.jac_tf = d_jac_tf;
        q.sign = f.sign; q.offset = f.offset;
        return q;
    }
};

// the counts whose fused value-and-blocks kernel builds without scratch; the others: value kernel, then
// the blocks in a launch of their own
static constexpr bool nc_in_accel(int nc) { return false OBTG_NC_ACCEL_LIST(OBTG_NC_EQ_); }
template <> struct RowKernels<AccelRows> {
    template <int NC, int DIM, bool JAC> static auto fused() -> void (*)(const SpeedExParams)
    {
        if constexpr (!JAC || nc_in_accel(NC)) return k_accel_true_min<NC, DIM, JAC>;
        else return nullptr;
    }
    template <int DIM> static auto envelope() { return k_accel_envelope<DIM>; }
    static SpeedExParams params(const obtg_ctx* c, const RowFamily& f, const double* dY, double* d_jac, double* d_jac_tf)
    {
        return RowKernels<SpeedRows>::params(c, f, dY, d_jac, d_jac_tf);
    }
};

// the jerk family: as the acceleration's, with a list of its own
static constexpr bool nc_in_jerk(int nc) { return false OBTG_NC_JERK_LIST(OBTG_NC_EQ_); }
template <> struct RowKernels<JerkRows> {
    template <int NC, int DIM, bool JAC> static auto fused() -> void (*)(const SpeedExParams)
    {
        if constexpr (!JAC || nc_in_jerk(NC)) return k_jerk_true_min<NC, DIM, JAC>;
        else return nullptr;
    }
    template <int DIM> static auto envelope() { return k_jerk_envelope<DIM>; }
    static SpeedExParams params(const obtg_ctx* c, const RowFamily& f, const double* dY, double* d_jac, double* d_jac_tf)
    {
        return RowKernels<SpeedRows>::params(c, f, dY, d_jac, d_jac_tf);
    }
};

// the keep-in family: every count of OBTG_NC_SEP, values and blocks, builds without scratch: no list
template <> struct RowKernels<KeepInRows> {
    template <int NC, int DIM, bool JAC> static auto fused() { return k_keep_in_true_min<NC, DIM, JAC>; }
    template <int DIM> static auto envelope() { return k_keep_in_envelope<DIM>; }
    static KeepInExParams params(const obtg_ctx* c, const RowFamily& f, const double* dY, double* d_jac, double*)
    {
        KeepInExParams q{};
        q.Y = dY; q.H = c->d_keep_H.as<double>(); q.VF = c->d_keep_VF.as<int2>(); q.n_veh = c->n_veh; q.P = f.items; q.jac = d_jac;
        q.sign = f.sign; q.offset = f.offset;
        return q;
    }
};

// the counts of OBTG_NC_SEP whose angular-rate kernels hold their operands in registers; the others
// take the rows route
static constexpr bool nc_in_ang(int nc) { return false OBTG_NC_ANG_LIST(OBTG_NC_EQ_); }
template <> struct RowKernels<AngRows> {
    template <int NC, int DIM, bool JAC> static auto fused() -> void (*)(const AngExParams)
    {
        if constexpr (DIM == 2 && nc_in_ang(NC)) return k_ang_true_min<NC, JAC>;
        else return nullptr;
    }
    template <int DIM> static auto envelope() { return k_ang_envelope; }
    static AngExParams params(const obtg_ctx* c, const RowFamily& f, const double* dY, double* d_jac, double* d_jac_tf)
    {
        AngExParams q{};
        q.Y = dY; q.tf = f.d_tf; q.tab = c->d_ang_rows.as<double>(); q.n_veh = c->n_veh; q.jac = d_jac; q.jac_tf = d_jac_tf;
        q.sign = f.sign; q.offset = f.offset; q.W = f.w;
        return q;
    }
};

template <template <int, int> class Rows>
static int launch_fused(obtg_ctx* c, const RowFamily& f, const double* dY, const ExParams& ex, double* d_jac, double* d_jac_tf)
{
    auto q = RowKernels<Rows>::params(c, f, dY, d_jac, d_jac_tf);
    q.ex = ex;
    const int nc = c->deg + 1;
    void (*kern)(const decltype(q)) = nullptr;
#define OBTG_CASE(NC_, D_) \
    if (nc == NC_ && c->dim == D_) kern = d_jac ? RowKernels<Rows>::template fused<NC_, D_, true>() : RowKernels<Rows>::template fused<NC_, D_, false>();
#define OBTG_CASE_D(NC_) OBTG_CASE(NC_, 2) OBTG_CASE(NC_, 3)
    OBTG_NC_SEP(OBTG_CASE_D)
#undef OBTG_CASE_D
#undef OBTG_CASE
    if (!kern) return OBTG_ERR_UNSUPPORTED;
    const size_t lds = sizeof(double) * kExWaves * kExStack * (size_t)(ex.K + 3);
    const long per_wg = kExWaves * kWave;
    ScopedKernelTimer t(c, f.kernel_id);
    hipLaunchKernelGGL(kern, dim3((unsigned)((ex.M + per_wg - 1) / per_wg)), dim3(kExWaves * kWave), lds, c->stream, q);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

// ---- the two curvature families' launches.  Frames: kExStack x (NP K + 3) doubles per wave; at K = 63 that is 33 KB for the
// planar family and 65 280 bytes for the space family: under the 64 KB a workgroup's dynamic LDS may be without raising a
// limit, one wave per workgroup.
static_assert(sizeof(double) * kCvWaves * kExStack * (SpaceCurv3::NP * (2 * kCvMaxNC - 1) + 3) <= 65536, "space-curvature frames: lower the frame count");

// The host side of a curvature family, found by `kind`: the policy's shape and the kernels by name
typedef void (*CurvKernel)(const CurvParams);
struct CurvHost {
    int np, sides, dim;                            // the policy's NP, SIDES, DIM
    void (*rows)(const CurvParams, double*);
    CurvKernel search, envelope;
    CurvKernel (*fused)(int nc, bool jac);         // the in-register kernel of a count of the family's list, else null
};
static CurvKernel curv_fused(int nc, bool jac)
{
#define OBTG_CASE(NC_) if (nc == NC_) return jac ? k_curv_true_min<NC_, true> : k_curv_true_min<NC_, false>;
    OBTG_NC_CURV_LIST(OBTG_CASE)
#undef OBTG_CASE
    return nullptr;
}
static CurvKernel scurv_fused(int nc, bool jac)
{
#define OBTG_CASE(NC_) if (nc == NC_) return jac ? k_scurv_true_min<NC_, true> : k_scurv_true_min<NC_, false>;
    OBTG_NC_SCURV_LIST(OBTG_CASE)
#undef OBTG_CASE
    return nullptr;
}
static const CurvHost& curv_host(RowKind kind)
{
    static const CurvHost planar{ PlanarCurv::NP, PlanarCurv::SIDES, PlanarCurv::DIM, k_curv_rows, k_curv_search, k_curv_envelope, curv_fused };
    static const CurvHost space{ SpaceCurv3::NP, SpaceCurv3::SIDES, SpaceCurv3::DIM, k_scurv_rows, k_scurv_search, k_scurv_envelope, scurv_fused };
    return kind == ROWS_SCURV ? space : planar;
}

static CurvParams curv_params(const double* d_curves, const double* d_tab, int nc, long items, double W, double eps_rel, int max_nodes)
{
    CurvParams q{};
    q.Y = d_curves; q.tab = d_tab; q.nc = nc; q.M = items; q.W = W; q.eps_rel = eps_rel; q.max_nodes = max_nodes;
    return q;
}
static size_t curv_lds_bytes(const CurvHost& h, int K) { return sizeof(double) * kCvWaves * kExStack * (size_t)(h.np * K + 3); }
static unsigned curv_grid(long items) { const long per_wg = kCvWaves * kWave; return (unsigned)((items + per_wg - 1) / per_wg); }

bool curvature_supported(int nc) { return nc >= 2 && nc <= kCvMaxNC; }
CurvShape curvature_shape(RowKind kind) { const CurvHost& h = curv_host(kind); return CurvShape{ h.np, h.sides, h.dim }; }

int launch_curv_rows(obtg_ctx* c, RowKind kind, const double* d_curves, const double* d_tab, long n_curves, int nc, double* d_out,
                     int kernel_id)
{
    if (n_curves <= 0) return OBTG_OK;
    if (!curvature_supported(nc)) return OBTG_ERR_UNSUPPORTED;
    const CurvHost& h = curv_host(kind);
    const CurvParams q = curv_params(d_curves, d_tab, nc, h.sides * n_curves, 0.0, 0.0, 1);
    ScopedKernelTimer t(c, kernel_id);
    hipLaunchKernelGGL(h.rows, dim3((unsigned)n_curves), dim3(kWave), 0, c->stream, q, d_out);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_curv_search(obtg_ctx* c, RowKind kind, const double* d_rows, long items, int nc, double max_curv, int free_curve,
                       double eps_rel, int max_nodes, double* d_val, double* d_t, double* d_val1, double* d_t1, int* d_status,
                       int kernel_id)
{
    if (items <= 0) return OBTG_OK;
    if (!curvature_supported(nc)) return OBTG_ERR_UNSUPPORTED;
    const CurvHost& h = curv_host(kind);
    CurvParams q = curv_params(nullptr, nullptr, nc, items, max_curv, eps_rel, max_nodes);
    q.rows = d_rows; q.val = d_val; q.t = d_t; q.val1 = d_val1; q.t1 = d_t1; q.status = d_status; q.free_curve = free_curve;
    ScopedKernelTimer t(c, kernel_id);
    hipLaunchKernelGGL(h.search, dim3(curv_grid(items)), dim3(kCvWaves * kWave), curv_lds_bytes(h, 2 * nc - 1), c->stream, q);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

// the counts of the family's list: coefficients in registers, one launch (with the blocks when d_jac is set)
static int launch_curv_fused(obtg_ctx* c, const RowFamily& f, const double* dY, const ExParams& ex, double* d_jac)
{
    const CurvHost& h = curv_host(f.kind);
    if (c->dim != h.dim) return OBTG_ERR_UNSUPPORTED;
    const int nc = c->deg + 1;
    const CurvKernel kern = h.fused(nc, d_jac != nullptr);
    if (!kern) return OBTG_ERR_UNSUPPORTED;
    CurvParams q = curv_params(dY, c->d_ang_rows.as<double>(), nc, ex.M, f.w, ex.eps_rel, ex.max_nodes);
    q.val = ex.val; q.t = ex.t; q.status = ex.status; q.jac = d_jac;
    ScopedKernelTimer t(c, f.kernel_id);
    hipLaunchKernelGGL(kern, dim3(curv_grid(ex.M)), dim3(kCvWaves * kWave), curv_lds_bytes(h, ex.K), c->stream, q);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

// the blocks alone, from Y, the rows' values and their t_star
static int launch_curv_blocks(obtg_ctx* c, const RowFamily& f, const double* dY, const ExParams& ex, const double* d_val, double* d_jac)
{
    CurvParams q = curv_params(dY, c->d_ang_rows.as<double>(), c->deg + 1, ex.M, f.w, 0.0, 1);
    q.val = const_cast<double*>(d_val); q.t = ex.t; q.jac = d_jac;
    ScopedKernelTimer t(c, f.kernel_id);
    hipLaunchKernelGGL(curv_host(f.kind).envelope, dim3((unsigned)((ex.M + kEnvThreads - 1) / kEnvThreads)), dim3(kEnvThreads), 0, c->stream, q);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_true_min(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double eps_rel, int max_nodes, double* d_out,
                    double* d_t, int* d_status, double* d_jac, double* d_jac_tf)
{
    if (B <= 0 || f.items <= 0) return OBTG_OK;
    if (!nc_in_sep(c->deg + 1) || (c->dim != 2 && c->dim != 3)) return OBTG_ERR_UNSUPPORTED;
    int rc = ensure_tables(c);
    if (rc) return rc;
    ExParams ex{};
    ex.val = d_out; ex.t = d_t; ex.status = d_status;
    ex.M = (long)B * f.items; ex.K = row_len(f, c->deg); ex.max_nodes = max_nodes; ex.eps_rel = eps_rel; ex.eps_abs = 0.0;
    switch (f.kind) {
        case ROWS_ANG: return launch_fused<AngRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_SPEED: return launch_fused<SpeedRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_ACCEL: return launch_fused<AccelRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_JERK: return launch_fused<JerkRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_KEEP_IN: return launch_fused<KeepInRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_CURV: case ROWS_SCURV: return launch_curv_fused(c, f, dY, ex, d_jac);
        default: return launch_fused<TsepRows>(c, f, dY, ex, d_jac, d_jac_tf);
    }
}

template <template <int, int> class Rows>
static int launch_blocks(obtg_ctx* c, const RowFamily& f, const double* dY, const ExParams& ex, double* d_jac, double* d_jac_tf)
{
    auto q = RowKernels<Rows>::params(c, f, dY, d_jac, d_jac_tf);
    q.ex = ex;
    void (*kern)(const decltype(q), int) = c->dim == 1 ? RowKernels<Rows>::template envelope<1>()
                                           : c->dim == 2 ? RowKernels<Rows>::template envelope<2>() : RowKernels<Rows>::template envelope<3>();
    ScopedKernelTimer t(c, f.kernel_id);
    hipLaunchKernelGGL(kern, dim3((unsigned)((ex.M + kEnvThreads - 1) / kEnvThreads)), dim3(kEnvThreads), 0, c->stream, q, c->deg + 1);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_true_min_envelope(obtg_ctx* c, const RowFamily& f, const double* dY, int B, const double* d_t, double* d_jac,
                             double* d_jac_tf, const double* d_val)
{
    if (B <= 0 || f.items <= 0) return OBTG_OK;
    if (c->deg + 1 > kEnvMaxNC) return OBTG_ERR_UNSUPPORTED;
    ExParams ex{};
    ex.t = const_cast<double*>(d_t); ex.M = (long)B * f.items;
    switch (f.kind) {
        case ROWS_CURV: case ROWS_SCURV: return launch_curv_blocks(c, f, dY, ex, d_val, d_jac);
        case ROWS_ANG: return launch_blocks<AngRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_SPEED: return launch_blocks<SpeedRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_ACCEL: return launch_blocks<AccelRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_JERK: return launch_blocks<JerkRows>(c, f, dY, ex, d_jac, d_jac_tf);
        case ROWS_KEEP_IN: return launch_blocks<KeepInRows>(c, f, dY, ex, d_jac, d_jac_tf);
        default: return launch_blocks<TsepRows>(c, f, dY, ex, d_jac, d_jac_tf);
    }
}

// obtg_ang_rate_poly's launch, and the family's rows_r0
int launch_ang_rows(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double* d_out)
{
    if (B <= 0 || f.items <= 0) return OBTG_OK;
    if (c->dim != 2 || c->deg < 1 || c->deg + 1 > kEnvMaxNC) return OBTG_ERR_UNSUPPORTED;
    int rc = ensure_tables(c);
    if (rc) return rc;
    const AngExParams q = RowKernels<AngRows>::params(c, f, dY, nullptr, nullptr);
    ScopedKernelTimer t(c, f.kernel_id);
    hipLaunchKernelGGL(k_ang_rows, dim3((unsigned)((size_t)B * c->n_veh)), dim3(kWave), 0, c->stream, q, c->deg + 1, d_out);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

RowFamily ang_row_family(const obtg_ctx* c, const double* d_tf, double max_rate)
{
    RowFamily f{ ROWS_ANG, 2 * c->n_veh, OBTG_K_ANG_RATE, 1.0, 0.0, d_tf, launch_ang_rows };
    f.w = max_rate;
    return f;
}

// obtg_[space_]curvature_poly's launch, and the families' rows_r0: [B][n_veh][NP][2 deg + 1] -- num then den; wx, wy, wz, den
int launch_curvature_rows(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double* d_out)
{
    if (B <= 0 || f.items <= 0) return OBTG_OK;
    if (c->dim != curv_host(f.kind).dim || !curvature_supported(c->deg + 1)) return OBTG_ERR_UNSUPPORTED;
    int rc = ensure_tables(c);
    if (rc) return rc;
    return launch_curv_rows(c, f.kind, dY, c->d_ang_rows.as<double>(), (long)B * c->n_veh, c->deg + 1, d_out, f.kernel_id);
}

// a family's search of its workspace rows: a curve's NP rows serve its SIDES items
static int curvature_rows_search(obtg_ctx* c, const RowFamily& f, const double* d_rows, long items, double eps_rel, int max_nodes,
                                 double* d_out, double* d_t, int* d_status)
{
    return launch_curv_search(c, f.kind, d_rows, items, c->deg + 1, f.w, 0, eps_rel, max_nodes, d_out, d_t, nullptr, nullptr, d_status,
                              f.kernel_id);
}

// ---- the proximity family's launches (the chain that puts them together: capi.cpp proximity_chain)
static constexpr bool nc_in_prox(int nc) { return false OBTG_NC_PROX_LIST(OBTG_NC_EQ_); }
bool proximity_fused(const obtg_ctx* c) { return (c->dim == 2 || c->dim == 3) && nc_in_prox(c->deg + 1); }

static ProxExParams prox_params(const obtg_ctx* c, const double* dY, int B)
{
    ProxExParams q{};
    q.Y = dY; q.pts = c->d_prox_pts.as<double>(); q.items = c->d_prox_items.as<int>(); q.par = c->d_prox_par.as<double>();
    q.n_veh = c->n_veh; q.P = c->prox_P;             // (W2: the fused launches, once ensure_tables has made it)
    q.ex.M = (long)B * c->prox_P; q.ex.K = 2 * c->deg + 1;
    return q;
}
static void prox_outputs(ProxExParams& q, const ProxOut& o, double eps_rel, int max_nodes)
{
    q.ex.val = o.val; q.ex.t = o.t; q.ex.bound = o.bound; q.ex.nodes = o.nodes; q.ex.status = o.status;
    q.ex.eps_rel = eps_rel; q.ex.eps_abs = 0.0; q.ex.max_nodes = max_nodes;
}
static unsigned prox_grid(long M) { const long per_wg = kExWaves * kWave; return (unsigned)((M + per_wg - 1) / per_wg); }
static size_t prox_lds(int K) { return sizeof(double) * kExWaves * kExStack * (size_t)(K + 3); }

// MODE as prox_body's; null: the count has no kernel of its own
static void (*prox_kernel(const obtg_ctx* c, int mode))(const ProxExParams)
{
    const int nc = c->deg + 1;
#define OBTG_CASE(NC_, D_) \
    if (nc == NC_ && c->dim == D_) return mode == 2 ? k_prox_true<NC_, D_, 2> : mode == 1 ? k_prox_true<NC_, D_, 1> : k_prox_true<NC_, D_, 0>;
#define OBTG_CASE_D(NC_) OBTG_CASE(NC_, 2) OBTG_CASE(NC_, 3)
    OBTG_NC_PROX_LIST(OBTG_CASE_D)
#undef OBTG_CASE_D
#undef OBTG_CASE
    return nullptr;
}

int launch_proximity_rows(obtg_ctx* c, const double* dY, int B, double* d_out)
{
    if (B <= 0 || c->prox_P <= 0) return OBTG_OK;
    if ((c->dim != 2 && c->dim != 3) || c->deg + 1 > kEnvMaxNC) return OBTG_ERR_UNSUPPORTED;
    ProxExParams q = prox_params(c, dY, B);
    q.rows = d_out;
    if (auto kern = prox_kernel(c, 2)) {
        if (int rc = ensure_tables(c)) return rc;
        q.W2 = c->d_w2.as<double>();
        ScopedKernelTimer t(c, OBTG_K_TEMPORAL_SEP);
        hipLaunchKernelGGL(kern, dim3(prox_grid(q.ex.M)), dim3(kExWaves * kWave), 0, c->stream, q);
        OBTG_HIP(c, hipGetLastError());
        return OBTG_OK;
    }
    for (int v : { c->deg, 2 * c->deg }) { const int o = binrow_offset(c, v); if (o < 0) return o; }
    const double* bin = c->d_binrows.as<double>();
    ScopedKernelTimer t(c, OBTG_K_TEMPORAL_SEP);
    hipLaunchKernelGGL(c->dim == 2 ? k_prox_rows<2> : k_prox_rows<3>, dim3((unsigned)q.ex.M), dim3(kWave), 0, c->stream, q, c->deg + 1,
                       bin + binrow_offset(c, c->deg), bin + binrow_offset(c, 2 * c->deg));
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_proximity_true(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, const ProxOut& o, double* d_jac)
{
    if (B <= 0 || c->prox_P <= 0) return OBTG_OK;
    auto kern = proximity_fused(c) ? prox_kernel(c, d_jac ? 1 : 0) : nullptr;
    if (!kern) return OBTG_ERR_UNSUPPORTED;
    ProxExParams q = prox_params(c, dY, B);
    prox_outputs(q, o, eps_rel, max_nodes);
    q.jac = d_jac;
    if (int rc = ensure_tables(c)) return rc;
    q.W2 = c->d_w2.as<double>();
    ScopedKernelTimer t(c, OBTG_K_TEMPORAL_SEP);
    hipLaunchKernelGGL(kern, dim3(prox_grid(q.ex.M)), dim3(kExWaves * kWave), prox_lds(q.ex.K), c->stream, q);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_proximity_search(obtg_ctx* c, const double* d_rows, int B, double eps_rel, int max_nodes, const ProxOut& o)
{
    if (B <= 0 || c->prox_P <= 0) return OBTG_OK;
    if (!bern_extrema_supported(2 * c->deg + 1)) return OBTG_ERR_UNSUPPORTED;
    ProxExParams q = prox_params(c, nullptr, B);
    prox_outputs(q, o, eps_rel, max_nodes);
    q.ex.c = d_rows;
    ScopedKernelTimer t(c, OBTG_K_TEMPORAL_SEP);
    hipLaunchKernelGGL(k_prox_search, dim3(prox_grid(q.ex.M)), dim3(kExWaves * kWave), prox_lds(q.ex.K), c->stream, q);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_proximity_envelope(obtg_ctx* c, const double* dY, int B, const double* d_t, double* d_jac)
{
    if (B <= 0 || c->prox_P <= 0) return OBTG_OK;
    if ((c->dim != 2 && c->dim != 3) || c->deg + 1 > kEnvMaxNC) return OBTG_ERR_UNSUPPORTED;
    ProxExParams q = prox_params(c, dY, B);
    q.ex.t = const_cast<double*>(d_t); q.jac = d_jac;
    ScopedKernelTimer t(c, OBTG_K_TEMPORAL_SEP);
    hipLaunchKernelGGL(c->dim == 2 ? k_prox_envelope<2> : k_prox_envelope<3>, dim3((unsigned)((q.ex.M + kEnvThreads - 1) / kEnvThreads)),
                       dim3(kEnvThreads), 0, c->stream, q, c->deg + 1);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

RowFamily curvature_row_family(const obtg_ctx* c, RowKind kind, double max_curv)
{
    const CurvHost& h = curv_host(kind);
    RowFamily f{ kind, h.sides * c->n_veh, OBTG_K_ANG_RATE, 1.0, 0.0, nullptr, launch_curvature_rows };
    f.w = max_curv;
    f.search = curvature_rows_search;
    f.ws_rows = h.np / h.sides;
    return f;
}

}  // namespace obtg
