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
};

template <int DIM>
__global__ __launch_bounds__(kKoWaves * kWave) void k_keep_out(const KeepOutParams p)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int K = p.K, pitch = DIM * K + 3;
    double* stk = lds + (size_t)wave * (kKoStack * pitch + kKoMaxFaces * (DIM + 1));
    double* hf = stk + kKoStack * pitch;
    const long item = (long)blockIdx.x * kKoWaves + wave;
    if (item >= p.M) return;                       // (wave-uniform; the kernel has no workgroup barrier)

    int f0 = 0, F = p.F_all;
    const double* y;
    if (p.VO) {
        const long b = item / p.P;
        const int2 vo = p.VO[(int)(item - b * p.P)];
        f0 = p.obs_off[vo.y];
        F = p.obs_off[vo.y + 1] - f0;
        y = p.Y + ((size_t)b * p.n_veh + vo.x) * (DIM * K);
    } else {
        y = p.Y + (size_t)item * (DIM * K);
    }
    for (int k = lane; k < F * (DIM + 1); k += kWave) hf[k] = p.H[(size_t)f0 * (DIM + 1) + k];
    ko_wave_sync();

    // ---- the root (node 1)
    double x[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) x[c] = lane < K ? y[c * K + lane] : 0.0;
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
    s = ko_wave_max(s);
    const double tol = p.eps_rel * s;
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
    }

    // ---- the active faces at t_star: c(t_star) and c'(t_star) from the item's own control points
    const double nan = __builtin_nan("");
    KoActive a;
    a.f1 = -1; a.f2 = -1; a.lam1 = nan;
    if (bad) { U = tU = bound = nan; nodes = 0; }
    else {
        const double ts = tU, sc = 1.0 - ts;
        double pt[DIM], dir[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            double b = lane < K ? y[c * K + lane] : 0.0;
            for (int r = 1; r < K - 1; ++r) {
                const double up = wave_next_lane(b);
                b = __builtin_fma(ts, up, sc * b);
            }
            const double d0 = ko_lane(b, 0), d1 = ko_lane(b, 1);
            dir[c] = (double)(K - 1) * (d1 - d0);
            pt[c] = __builtin_fma(ts, d1, sc * d0);
        }
        a = keep_out_active<DIM>(hf, F, pt, dir, tol, ts > 0.0 && ts < 1.0);
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
            o[c * K + lane] = ac * wv;
        }
    }
}

// d_H | d_off | d_VO: device tables (the context's, or a free-curve call's own); VO null: free curves, one obstacle of F_all faces
int launch_keep_out(obtg_ctx* c, int dim, int K, const double* dY, long M, int n_veh, int P, const double* d_H, const int* d_off,
                    const int* d_VO, int F_all, double margin, double eps_rel, int max_nodes, double* d_val, double* d_t, int* d_face,
                    double* d_lam, double* d_bound, int* d_nodes, int* d_status, double* d_jac, int kernel_id)
{
    if (M <= 0) return OBTG_OK;
    if ((dim != 2 && dim != 3) || K < 2 || K > kKoMaxK) return OBTG_ERR_UNSUPPORTED;
    KeepOutParams p{};
    p.Y = dY; p.H = d_H; p.obs_off = d_off; p.VO = (const int2*)d_VO;
    p.val = d_val; p.t = d_t; p.face = d_face; p.lam = d_lam; p.bound = d_bound; p.nodes = d_nodes; p.status = d_status; p.jac = d_jac;
    p.M = M; p.n_veh = n_veh; p.P = P; p.K = K; p.F_all = F_all; p.max_nodes = max_nodes; p.margin = margin; p.eps_rel = eps_rel;
    const size_t lds = sizeof(double) * kKoWaves * ((size_t)kKoStack * (dim * K + 3) + kKoMaxFaces * (dim + 1));
    ScopedKernelTimer t(c, kernel_id);
    hipLaunchKernelGGL(dim == 2 ? k_keep_out<2> : k_keep_out<3>, dim3((unsigned)((M + kKoWaves - 1) / kKoWaves)), dim3(kKoWaves * kWave),
                       lds, c->stream, p);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

}  // namespace obtg
