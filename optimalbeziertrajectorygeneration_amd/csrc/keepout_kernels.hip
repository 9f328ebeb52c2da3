// The keep-out rows (obtg_keep_out_true_min[_jac][_dev], obtg_bern_keep_out[_dev]): per (batch row, vehicle, obstacle) item
//     min over t in [0, 1] of  G(t) = max over the obstacle's faces f of  g_f(t) = a_f . c(t) - b_f,
// a certified minimum of a maximum of polynomials (keepout_device.h).
//
// Search (k_keep_out): the conventions of obtg_bern_extrema's wave_search (extrema_kernels.hip), the whole wave on one item.
// A node is a sub-curve: its DIM coordinate rows of K control points, lane i holding point i.  It is split at 1/2 by de
// Casteljau (0.5 b + 0.5 up) on the coordinate rows; the left child then sits in lanes 0 .. 31 and the right child in lanes
// 32 .. 63, and both are evaluated at once: every lane forms the F face coefficients of its control point (keep_out_coeff)
// and per face the smallest of a half is the face's hull bound.  A child gives
//     its lower bound  max_f min_i g_f,i    (G >= g_f >= min_i g_f,i on the child, for every f),
//     the exact G at the split point: max_f of the left child's last coefficients (the ends of the root likewise).
// s = max |g_f,i| of the root, tol = eps_rel s; incumbent U from end / mid values, replaced on strict decrease only; a child
// is dropped when U - lb <= tol; depth-first, the smaller bound first; `nodes` counts sub-curves (the root is 1);
// OBTG_MD_NODE_CAP when the next split would pass max_nodes, OBTG_MD_DEPTH_CAP at kKoStack waiting frames, both with a valid
// bracket [bound, val].  Frames (DIM K control points | bound, t0, width) are in LDS, with the obstacle's faces.  A non-finite
// control point or face: NaN outputs, status OK.  A root that closes: val is an end value, t_star 0 or 1, nodes 1.
// Then the faces that carry the envelope block at t_star (keep_out_active: the co-activity rule), from c(t_star) and
// c'(t_star) by de Casteljau on the item's own control points, and -- only when blocks are asked for -- the block
//     jac[c][i] = (lam1 a_f1[c] + lam2 a_f2[c]) B_i(t_star),
// the basis a lane per index in the recurrence of envelope_block.  Whether blocks are written is a null pointer, not another
// kernel: the value call and the _jac call run the same instructions up to there, so they agree bit for bit; an item's
// outputs depend on its control points, its faces, margin, eps_rel and max_nodes alone.
// No finishing step (a monotone root of g_f1 - g_f2) is built: convergence at a kink is linear.
//
// Moving obstacles (obtg_keep_out_moving_*; KeepOutMovingParams): the same body on the RELATIVE curve
// D = P - E, E the obstacle's offset q(s tf) at the vehicle's degree (keep_out_motion_points).  A prologue forms E and D a lane
// per control point and leaves them in LDS beside the faces (2 DIM K doubles per wave); the root reads D from its registers and
// the evaluation at t_star reads it from LDS where the static form reads the item's control points -- everything between is
// the code above, the same instructions.  One more nullable output, jac_tf = -(a^ . E'(t_star)) t_star / tf.  The static
// instantiation has no prologue, no extra LDS and no extra argument.
//
// The Euclidean metric (obtg_keep_out_euclid_*; KeepOutEuclidParams): the same body on the NORMALISED faces with
// the signed Euclidean distance D in G's place.  The obstacle's feature records (keepout_features.h) are staged in LDS beside the
// faces; where the search takes an exact value -- the root's ends, each split point, c(t_star) -- and max_f g_f > 0 there, the
// wave evaluates the features of that point in parallel (keep_out_euclid_point) and the winner's dual pair (u, beta) adds
// min_i (u . P_i - beta) to the bound of both children (of the root: both ends' pairs).  What it changes is folded into the
// per-lane accumulators (gm, gmx, lbh, lb) AHEAD of the statements that read them out, and dir and the active set leave through
// keep_out_euclid_outputs, so the other instantiations keep every statement and their instruction streams.  A root that closes:
// bound = min(lb, val), since a dual bound and the value it meets are rounded apart.
//
// Vehicle pairs (obtg_pair_keep_out_*; KeepOutPairParams, KeepOutEuclidPairParams): the same body on D = Y_i - Y_j
// against ONE region around the origin, under either metric.  The prologue is one subtraction per control point; D stays in LDS
// behind the faces (behind the records under the Euclidean metric: OBTG_KO_LDS_WAVE_DOUBLES), the root reads it from its registers and the
// evaluation at t_star from LDS -- what the moving form does with its D.  No E, no restriction, no jac_tf.
//
// Launch (below the kernel): ONE launcher, launch_keep_out over KeepOutLaunch (obtg_internal.h), for all five
// parameter types.  It refuses what the kernel is not built for, fills the common prefix of the parameters once and the form's
// own members after it, and picks one of the ten instantiations.  A new form is a parameter struct here, its members in
// launch_keep_out_form and a line in launch_keep_out; the host side of it is a line of capi.cpp's column table.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "obtg_internal.h"
#include "md_device.h"
#include "keepout_device.h"
#pragma clang fp contract(off)

namespace obtg {

struct KeepOutParams {
    const double* __restrict__ Y;        // [B][n_veh*DIM][K]; free curves (VO null): [M][DIM][K]
    const double* __restrict__ H;        // [F][DIM + 1]: (a, b) of every face a . p <= b
    const int* __restrict__ obs_off;     // [O + 1]: obstacle o owns faces obs_off[o] .. obs_off[o + 1] - 1
    const int2* __restrict__ VO;         // [P]: (vehicle, obstacle); null: every curve against faces 0 .. F_all - 1
    double* __restrict__ val;            // [M]
    double* __restrict__ t;              // [M] nullable
    int* __restrict__ face;              // [M][2] nullable
    double* __restrict__ lam;            // [M] nullable
    double* __restrict__ bound;          // [M] nullable
    int* __restrict__ nodes;             // [M] nullable
    int* __restrict__ status;            // [M] nullable
    double* __restrict__ jac;            // [M][DIM][K] nullable
    long M;
    int n_veh, P, K, F_all, max_nodes;
    double margin, eps_rel;
    static constexpr bool kMoving = false;
    static constexpr bool kEuclid = false;
    static constexpr bool kPair = false;
};

// The Euclidean metric: H holds the NORMALISED faces; the static form only
struct KeepOutEuclidParams : KeepOutParams {
    const double* __restrict__ feat;     // [NF][kKoFeatRec]: the obstacles' feature records, one obstacle after the other
    const int* __restrict__ feat_off;    // [O + 1]: obstacle o owns records feat_off[o] .. feat_off[o + 1] - 1; free curves: null
    double* __restrict__ dir;            // [M][DIM] nullable: the unit direction the block carries
    int* __restrict__ faces3;            // [M][3] nullable: the active set, -1 padded
    int NF_all;                          // free curves: the records of the one obstacle
    static constexpr bool kEuclid = true;
};

struct KeepOutMovingParams : KeepOutParams {
    const double* __restrict__ Q;        // the obstacles' [DIM][m_o + 1] blocks, one after the other; free curves: [DIM][Km]
    const int* __restrict__ q_off;       // [O + 1], in control points; an empty run: the obstacle stands still
    const double* __restrict__ T;        // [O]: the motions' spans
    const double* __restrict__ tf;       // [B]: the vehicles' spans
    const double* __restrict__ r;        // free curves: [M] the ratios, null: 1
    double* __restrict__ rel;            // [M][DIM][K] nullable: the relative control points
    double* __restrict__ jac_tf;         // [M] nullable
    int Km;                              // free curves: the motion's control points
    static constexpr bool kMoving = true;
};

// Vehicle pairs (obtg_pair_keep_out_*): VO holds the pair's (i, j), i < j, read from the table as the static form
// reads its (vehicle, obstacle) -- no integer square root per item, and the order is the host's, whatever it is; the ONE region
// is faces 0 .. F_all - 1 (and records 0 .. NF_all - 1).  The search runs on D = Y_i - Y_j; obs_off and feat_off are not read.
struct KeepOutPairParams : KeepOutParams {
    double* __restrict__ rel;            // [M][DIM][K] nullable: the relative control points
    static constexpr bool kPair = true;
};

struct KeepOutEuclidPairParams : KeepOutEuclidParams {
    double* __restrict__ rel;            // [M][DIM][K] nullable
    static constexpr bool kPair = true;
};

// The Euclidean outputs of one item: dir[DIM] and the active set (obstacle-local faces fc, -1 padded; f0 the obstacle's first
// face) -- ud null: a NaN item.  dir is left in the wave's first frame slots too, for the envelope block.
template <int DIM>
__device__ __forceinline__ void keep_out_euclid_outputs(const KeepOutEuclidParams& p, const long item, const int lane, double* stk,
                                                        const double* ud, const int* fc, const int f0)
{
    ko_wave_sync();
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const double v = ud ? ud[c] : __builtin_nan("");
            stk[c] = v;
            if (p.dir) p.dir[DIM * item + c] = v;
        }
        if (p.faces3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p.faces3[3 * item + k] = (!fc || fc[k] < 0) ? -1 : f0 + fc[k];
        }
    }
    ko_wave_sync();
}

template <int DIM, class PRM>
__global__ __launch_bounds__(kKoWaves * kWave) void k_keep_out(const PRM p)
{
    constexpr bool MV = PRM::kMoving, EU = PRM::kEuclid, PR = PRM::kPair;
    static_assert(!(MV && EU), "the Euclidean metric is built for obstacles that stand still");
    static_assert(!(MV && PR), "a pair's region does not move in the pair's own frame");
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int K = p.K, pitch = DIM * K + 3;
    double* stk = lds + (size_t)wave * OBTG_KO_LDS_WAVE_DOUBLES(DIM, K, pitch, MV, EU, PR);
    double* hf = stk + kKoStack * pitch;
    double* ed = hf + kKoMaxFaces * (DIM + 1);     // MV: E[DIM][K] | D[DIM][K];  EU: the feature records;  PR: D[DIM][K] behind them
    const long item = (long)blockIdx.x * kKoWaves + wave;
    if (item >= p.M) return;                       // (wave-uniform; the kernel has no workgroup barrier)

    int f0 = 0, F = p.F_all;
    const double* y;
    const double* q = nullptr;                     // MV: the obstacle's motion, Km control points per coordinate (0: none)
    int Km = 0;
    double tf_b = 1.0, ratio = 1.0;
    int nf = 0;                                    // EU: the obstacle's features
    if constexpr (PR) {
        y = nullptr;                               // (the prologue below reads both vehicles; nothing after it reads y)
        if constexpr (EU) {
            nf = min(p.NF_all, kKoMaxFeatures);
            for (int k = lane; k < nf * kKoFeatRec; k += kWave) ed[k] = p.feat[k];
        }
    } else if (p.VO) {
        const long b = item / p.P;
        const int2 vo = p.VO[(int)(item - b * p.P)];
        f0 = p.obs_off[vo.y];
        F = p.obs_off[vo.y + 1] - f0;
        y = p.Y + ((size_t)b * p.n_veh + vo.x) * (DIM * K);
        if constexpr (MV) {
            const int q0 = p.q_off[vo.y];
            Km = p.q_off[vo.y + 1] - q0;
            q = p.Q + (size_t)DIM * q0;
            if (Km > 0) { tf_b = p.tf[b]; ratio = tf_b / p.T[vo.y]; }
        }
        if constexpr (EU) {
            const int r0 = p.feat_off[vo.y];
            nf = min(p.feat_off[vo.y + 1] - r0, kKoMaxFeatures);
            for (int k = lane; k < nf * kKoFeatRec; k += kWave) ed[k] = p.feat[(size_t)r0 * kKoFeatRec + k];
        }
    } else {
        y = p.Y + (size_t)item * (DIM * K);
        if constexpr (MV) {
            Km = p.Km; q = p.Q;
            if (p.r) ratio = p.r[item];
            tf_b = ratio;
        }
        if constexpr (EU) {
            nf = min(p.NF_all, kKoMaxFeatures);
            for (int k = lane; k < nf * kKoFeatRec; k += kWave) ed[k] = p.feat[k];
        }
    }
    for (int k = lane; k < F * (DIM + 1); k += kWave) hf[k] = p.H[(size_t)f0 * (DIM + 1) + k];

    // ---- the root (node 1)
    double x[DIM];
    bool bad_m = false;
    if constexpr (MV) {
        // the relative curve: E from the motion, D = P - E, both kept for the evaluations at t_star
        bad_m = Km > 0 && !(tf_b > 0.0 && tf_b <= DBL_MAX && ratio > 0.0 && ratio <= DBL_MAX);
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const double e = Km > 0 ? keep_out_motion_points(q + c * Km, Km, K, ratio, lane) : 0.0;
            const double d = (lane < K ? y[c * K + lane] : 0.0) - e;
            if (lane < K) {
                ed[c * K + lane] = e;
                ed[(DIM + c) * K + lane] = d;
            }
            x[c] = d;
        }
    }
    if constexpr (PR) {
        // the relative curve D = Y_i - Y_j, one subtraction per control point, kept for the evaluation at t_star
        const long b = item / p.P;
        const int2 ij = p.VO[(int)(item - b * p.P)];
        const double* yi = p.Y + ((size_t)b * p.n_veh + ij.x) * (DIM * K);
        const double* yj = p.Y + ((size_t)b * p.n_veh + ij.y) * (DIM * K);
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const double d = lane < K ? yi[c * K + lane] - yj[c * K + lane] : 0.0;
            if (lane < K) ed[ko_lds_pair_d(EU) + c * K + lane] = d;
            x[c] = d;
        }
    }
    ko_wave_sync();
    if constexpr (!MV && !PR) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) x[c] = lane < K ? y[c * K + lane] : 0.0;
    }
    double gm = -INFINITY, lb = -INFINITY, s = 0.0;
    bool bad = false;
    for (int f = 0; f < F; ++f) {
        const double g = keep_out_coeff<DIM>(hf + f * (DIM + 1), x);
        if (lane < K) { bad = bad || !(fabs(g) <= DBL_MAX); s = fmax(s, fabs(g)); }
        gm = fmax(gm, g);
        const double m = ko_half_min(lane < K ? g : INFINITY);
        lb = fmax(lb, ko_lane(m, kKoLowLast));
    }
    bad = __any(bad) != 0;
    if constexpr (MV) {
        bad = bad || bad_m;
        if (p.rel && lane < K) {                   // (x is still the root: D itself)
#pragma unroll
            for (int c = 0; c < DIM; ++c) p.rel[(size_t)item * (DIM * K) + c * K + lane] = bad ? __builtin_nan("") : x[c];
        }
    }
    if constexpr (PR) {
        if (p.rel && lane < K) {                   // (x is still the root: D itself)
#pragma unroll
            for (int c = 0; c < DIM; ++c) p.rel[(size_t)item * (DIM * K) + c * K + lane] = bad ? __builtin_nan("") : x[c];
        }
    }
    s = ko_wave_max(s);
    const double tol = p.eps_rel * s;
    if constexpr (EU) {
        // the ends' exact distances and the root's dual bounds: the maximisers at both ends
        if (!bad) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int le = e ? K - 1 : 0;
                if (!(ko_lane(gm, le) > 0.0)) continue;
                double pe[DIM];
#pragma unroll
                for (int c = 0; c < DIM; ++c) pe[c] = ko_lane(x[c], le);
                const KoDual<DIM> du = keep_out_euclid_point<DIM>(hf, F, ed, nf, pe, lane);
                const double m = ko_half_min(lane < K ? keep_out_coeff<DIM>(du.ub, x) : INFINITY);
                lb = fmax(lb, ko_lane(m, kKoLowLast));
                if (lane == le) gm = du.v;
            }
        }
    }
    const double G0 = ko_lane(gm, 0), G1 = ko_lane(gm, K - 1);
    double U, tU;
    if (G0 <= G1) { U = G0; tU = 0.0; } else { U = G1; tU = 1.0; }
    double bound = INFINITY;
    int nodes = 1, status = OBTG_MD_OK;

    if (!bad && !(U - lb <= tol)) {
        double t0 = 0.0, w = 1.0, cur_lb = lb;
        int sp = 0;
        for (;;) {
            if (nodes + 2 > p.max_nodes) { status = OBTG_MD_NODE_CAP; bound = fmin(bound, cur_lb); break; }
            // de Casteljau at 1/2 on every coordinate row, both pieces: left[r] is lane 0's value after level r, right[i] lane i's
            // after level K - 1 - i
            double left[DIM];
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                double b = x[c], l = b;
                for (int r = 1; r < K; ++r) {
                    const double up = wave_next_lane(b);
                    if (lane <= K - 1 - r) b = 0.5 * b + 0.5 * up;      // (two exact scalings, one rounding)
                    const double first = ko_lane(b, 0);
                    if (lane == r) l = first;
                }
                x[c] = b; left[c] = l;
            }
            // the left child in lanes 0 .. 31, the right child in lanes 32 .. 63
            double q[DIM];
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const double r = __shfl(x[c], lane & 31);
                q[c] = lane < 32 ? left[c] : r;
            }
            const bool act = (lane & 31) < K;
            double lbh = -INFINITY, gmx = -INFINITY;
            for (int f = 0; f < F; ++f) {
                const double g = keep_out_coeff<DIM>(hf + f * (DIM + 1), q);
                gmx = fmax(gmx, g);
                lbh = fmax(lbh, ko_half_min(act ? g : INFINITY));
            }
            if constexpr (EU) {
                // outside at the split point: its exact distance, and the maximiser there bounds both children
                if (ko_lane(gmx, K - 1) > 0.0) {
                    double pm[DIM];
#pragma unroll
                    for (int c = 0; c < DIM; ++c) pm[c] = ko_lane(q[c], K - 1);
                    const KoDual<DIM> du = keep_out_euclid_point<DIM>(hf, F, ed, nf, pm, lane);
                    lbh = fmax(lbh, ko_half_min(act ? keep_out_coeff<DIM>(du.ub, q) : INFINITY));
                    gmx = du.v;
                }
            }
            const double lbL = ko_lane(lbh, kKoLowLast), lbR = ko_lane(lbh, kKoHighLast), mid = ko_lane(gmx, K - 1);
            const double hw = 0.5 * w, tm = t0 + hw;
            nodes += 2;
            if (mid < U) { U = mid; tU = tm; }
            const bool aliveL = U - lbL > tol, aliveR = U - lbR > tol;
            if (!aliveL) bound = fmin(bound, lbL);
            if (!aliveR) bound = fmin(bound, lbR);
            if (aliveL && aliveR) {
                if (sp == kKoStack) { status = OBTG_MD_DEPTH_CAP; bound = fmin(bound, fmin(lbL, lbR)); break; }
                const bool go_left = lbL <= lbR;
                double* fr = stk + sp * pitch;
                if (lane < K) {
#pragma unroll
                    for (int c = 0; c < DIM; ++c) fr[c * K + lane] = go_left ? x[c] : left[c];
                }
                if (lane == 0) { fr[DIM * K] = go_left ? lbR : lbL; fr[DIM * K + 1] = go_left ? tm : t0; fr[DIM * K + 2] = hw; }
                ++sp;
                if (go_left) {
#pragma unroll
                    for (int c = 0; c < DIM; ++c) x[c] = left[c];
                    cur_lb = lbL;
                } else { t0 = tm; cur_lb = lbR; }
                w = hw;
            } else if (aliveL) {
#pragma unroll
                for (int c = 0; c < DIM; ++c) x[c] = left[c];
                cur_lb = lbL; w = hw;
            } else if (aliveR) { t0 = tm; cur_lb = lbR; w = hw; }
            else {
                bool found = false;
                ko_wave_sync();
                while (sp > 0) {
                    --sp;
                    const double* fr = stk + sp * pitch;
                    const double plb = fr[DIM * K];
                    if (U - plb > tol) {
#pragma unroll
                        for (int c = 0; c < DIM; ++c) x[c] = lane < K ? fr[c * K + lane] : 0.0;
                        t0 = fr[DIM * K + 1]; w = fr[DIM * K + 2]; cur_lb = plb;
                        found = true;
                        break;
                    }
                    bound = fmin(bound, plb);
                }
                ko_wave_sync();
                if (!found) break;
            }
        }
        if (status != OBTG_MD_OK) {            // what still waits is part of the bracket
            ko_wave_sync();
            for (int i = 0; i < sp; ++i) bound = fmin(bound, stk[i * pitch + DIM * K]);
            ko_wave_sync();
        }
        bound = fmin(bound, U);
    } else {
        bound = lb;
        if constexpr (EU) bound = fmin(lb, U);     // (a dual bound and the value it meets are rounded apart: keep bound <= val)
    }

    // ---- the active faces at t_star: c(t_star) and c'(t_star) from the item's own control points (MV: the relative ones)
    const double nan = __builtin_nan("");
    KoActive a;
    a.f1 = -1; a.f2 = -1; a.lam1 = nan;
    if (bad) {
        U = tU = bound = nan; nodes = 0;
        if constexpr (EU) keep_out_euclid_outputs<DIM>(p, item, lane, stk, nullptr, nullptr, 0);
    }
    else {
        const double ts = tU, sc = 1.0 - ts;
        double pt[DIM], dir[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            double b;
            if constexpr (MV) b = lane < K ? ed[(DIM + c) * K + lane] : 0.0;
            else if constexpr (PR) b = lane < K ? ed[ko_lds_pair_d(EU) + c * K + lane] : 0.0;
            else b = lane < K ? y[c * K + lane] : 0.0;
            for (int r = 1; r < K - 1; ++r) {
                const double up = wave_next_lane(b);
                b = __builtin_fma(ts, up, sc * b);
            }
            const double d0 = ko_lane(b, 0), d1 = ko_lane(b, 1);
            dir[c] = (double)(K - 1) * (d1 - d0);
            pt[c] = __builtin_fma(ts, d1, sc * d0);
        }
        a = keep_out_active<DIM>(hf, F, pt, dir, tol, ts > 0.0 && ts < 1.0);
        if constexpr (EU) {
            // outside at c(t_star): the maximiser's unit direction, no co-activity rule (D is C^1 there); otherwise the rule's
            // faces, which are the normalised ones here.  dir goes through LDS (the frames are free now) to the block below
            double gp = -INFINITY;
            for (int f = 0; f < F; ++f) gp = fmax(gp, keep_out_coeff<DIM>(hf + f * (DIM + 1), pt));
            double ud[DIM];
            int fc[3] = {a.f1, a.f2, -1};
            if (gp > 0.0) {
                const KoDual<DIM> du = keep_out_euclid_point<DIM>(hf, F, ed, nf, pt, lane);
#pragma unroll
                for (int c = 0; c < DIM; ++c) ud[c] = du.ub[c];
                fc[0] = du.fc[0]; fc[1] = du.fc[1]; fc[2] = du.fc[2];
            } else {
#pragma unroll
                for (int c = 0; c < DIM; ++c) {
                    ud[c] = hf[a.f1 * (DIM + 1) + c];
                    if (a.f2 >= 0) ud[c] = __builtin_fma(a.lam1, ud[c], (1.0 - a.lam1) * hf[a.f2 * (DIM + 1) + c]);
                }
            }
            keep_out_euclid_outputs<DIM>(p, item, lane, stk, ud, fc, f0);
        }
    }

    if (lane == 0) {
        p.val[item] = U - p.margin;
        if (p.t) p.t[item] = tU;
        if (p.face) { p.face[2 * item] = a.f1 < 0 ? -1 : f0 + a.f1; p.face[2 * item + 1] = a.f2 < 0 ? -1 : f0 + a.f2; }
        if (p.lam) p.lam[item] = a.lam1;
        if (p.bound) p.bound[item] = bound - p.margin;
        if (p.nodes) p.nodes[item] = nodes;
        if (p.status) p.status[item] = status;
    }
    if constexpr (MV) {
        // ---- d row / d tf = -(a^ . E'(t_star)) t_star / tf, E' by de Casteljau on E; an obstacle that stands still: an exact 0
        if (p.jac_tf) {
            double jt = bad ? nan : 0.0;
            if (!bad && Km > 0) {
                const double ts = tU, sc = 1.0 - ts;
                double dE[DIM], ah[DIM];
#pragma unroll
                for (int c = 0; c < DIM; ++c) {
                    double b = lane < K ? ed[c * K + lane] : 0.0;
                    for (int r = 1; r < K - 1; ++r) {
                        const double up = wave_next_lane(b);
                        b = __builtin_fma(ts, up, sc * b);
                    }
                    dE[c] = (double)(K - 1) * (ko_lane(b, 1) - ko_lane(b, 0));
                    ah[c] = hf[a.f1 * (DIM + 1) + c];
                    if (a.f2 >= 0) ah[c] = __builtin_fma(a.lam1, ah[c], (1.0 - a.lam1) * hf[a.f2 * (DIM + 1) + c]);
                }
                jt = -(keep_out_slope<DIM>(ah, dE) * ts / tf_b);
            }
            if (lane == 0) p.jac_tf[item] = jt;
        }
    }
    if (!p.jac) return;
    // ---- the envelope block: the basis a lane per index
    double wv = bad ? nan : (lane == 0 ? 1.0 : 0.0);
    const double ts = tU, sc = 1.0 - ts;
    for (int r = 1; r < K; ++r) {
        const double prev = __shfl_up(wv, 1);
        wv = keep_out_basis_level(lane, wv, prev, ts, sc);
    }
    if (lane < K) {
        double* o = p.jac + (size_t)item * (DIM * K);
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            double ac = nan;
            if (!bad) {
                ac = hf[a.f1 * (DIM + 1) + c];
                if (a.f2 >= 0) ac = __builtin_fma(a.lam1, ac, (1.0 - a.lam1) * hf[a.f2 * (DIM + 1) + c]);
            }
            if constexpr (EU) ac = stk[c];               // (keep_out_euclid_outputs left dir there, NaN for a NaN item)
            o[c * K + lane] = ac * wv;
        }
    }
}

// One form of the launch: the common prefix of the parameters once, then the form's own members, then one of its two kernels
template <class PRM>
static int launch_keep_out_form(obtg_ctx* c, const KeepOutLaunch& a)
{
    const KeepOutOutputs& o = a.out;
    PRM p{};
    p.Y = a.Y; p.H = a.H; p.obs_off = a.off; p.VO = (const int2*)a.VO_or_IJ;
    p.val = o.val; p.t = o.t; p.bound = o.bound; p.nodes = o.nodes; p.status = o.status; p.jac = o.jac;
    p.M = a.M; p.n_veh = a.n_veh; p.P = a.P; p.K = a.K; p.F_all = a.F_all; p.max_nodes = a.max_nodes;
    p.margin = a.margin; p.eps_rel = a.eps_rel;
    if constexpr (PRM::kEuclid) {              // (face and lam stay null: faces3 and dir stand in for them)
        p.feat = a.feat; p.feat_off = a.feat_off; p.NF_all = a.NF_all; p.dir = o.dir; p.faces3 = o.faces3;
    } else {
        p.face = o.face; p.lam = o.lam;
    }
    if constexpr (PRM::kMoving) {
        p.Q = a.Q; p.q_off = a.q_off; p.T = a.T; p.tf = a.tf; p.r = a.r; p.Km = a.Km; p.jac_tf = o.jac_tf;
    }
    if constexpr (PRM::kMoving || PRM::kPair) p.rel = o.rel;
    const size_t lds = ko_lds_bytes(a.dim, a.K, PRM::kMoving, PRM::kEuclid, PRM::kPair);
    const dim3 grid((unsigned)((a.M + kKoWaves - 1) / kKoWaves)), block(kKoWaves * kWave);
    void (*const kernel)(PRM) = a.dim == 2 ? k_keep_out<2, PRM> : k_keep_out<3, PRM>;
    if (PRM::kEuclid && lds > 64 * 1024)
        OBTG_HIP(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ScopedKernelTimer t(c, OBTG_K_SPEED);
    hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, p);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

// The ten instantiations: five parameter types (static, Euclidean, moving, pair, Euclidean pair) times two dimensions
int launch_keep_out(obtg_ctx* c, const KeepOutLaunch& a)
{
    if (a.M <= 0) return OBTG_OK;
    if ((a.dim != 2 && a.dim != 3) || a.K < 2 || a.K > kKoMaxK || (a.euclid && a.NF_all > kKoMaxFeatures) ||
        (a.pair && (a.F_all < 1 || a.F_all > kKoMaxFaces)) || (a.moving && (a.euclid || a.pair)))      // (k_keep_out's static_asserts)
        return OBTG_ERR_UNSUPPORTED;
    if (a.moving) return launch_keep_out_form<KeepOutMovingParams>(c, a);
    if (a.pair) return a.euclid ? launch_keep_out_form<KeepOutEuclidPairParams>(c, a) : launch_keep_out_form<KeepOutPairParams>(c, a);
    return a.euclid ? launch_keep_out_form<KeepOutEuclidParams>(c, a) : launch_keep_out_form<KeepOutParams>(c, a);
}

}  // namespace obtg
