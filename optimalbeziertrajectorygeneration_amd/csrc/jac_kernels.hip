// Exact derivatives of the Bernstein constraint / cost families for gfx950 (MI355X): what SLSQP is given as `jac`
// instead of forward differences.
//
// What is differentiated (reference file:line in the reference checkout), n = deg, d = dim, R = DEG_ELEV:
//   temporal separation  optimization.py:311-346   e_m = (d/2) sum_ij G_mij sum_c D_ci D_cj,   D = P_a - P_b
//   max / min speed      optimization.py:349-422   the same rows of D = diff(P) (derivative, then elev(1))
//   angular rate         optimization.py:425-459, 578-611   num_k / den_k, both elevated by 4R
//   objectives           optimization.py:462-539   euclidean; accel / jerk = sum of the speed rows of diff^(k-1)(P)
// with G_mij = C(n,i) C(n,j) C(R, m-i-j) / C(2n+R, m): the folded product (bezier.py:1183-1208) followed by the elevation
// (bezier.py:1127-1147) as ONE table per (deg, R), so that
//   d e_m / d D_ci = d * sum_j G_mij D_cj       (G symmetric in i, j; nonzero for 0 <= m-i-j <= R only).
// diff's linear map (bezier.py:497-519): diff(P)_i = (1/T) [ i (P_i - P_{i-1}) + (n-i) (P_{i+1} - P_i) ], i = 0..n.
//
// Kernel shapes.  Separation writes (n+1) d doubles per row and pair from d (n+1) inputs: store bound.  A workgroup walks
// pairs (grid-stride), stages the pair's difference in LDS and writes the pair's [L][d][n+1] block with consecutive lanes
// on consecutive doubles; G sits in LDS when it fits in 64 KB (R <= 48 at n = 10) and is read through L2 otherwise.
// Angular rate is a dependent chain per vehicle (derivatives -> products -> elevation -> quotient): one workgroup per
// vehicle, every stage in LDS.  float64 throughout; contraction allowed (the bound against exact rationals is 1e-11).
#include <algorithm>
#include <cmath>
#include <vector>

#include "obtg_internal.h"

namespace obtg {

constexpr int kJacThreads = 256;
constexpr size_t kJacLdsG = 64 * 1024;     // largest G staged in LDS

// ------------------------------------------------------------------------------------------------ host tables
static long double binom_l(int n, int k)
{
    if (k < 0 || k > n) return 0.0L;
    if (k > n - k) k = n - k;
    long double r = 1.0L;
    for (int i = 1; i <= k; ++i) r = r * (long double)(n - k + i) / (long double)i;
    return r;
}

// Gd[L][nc][nc] (dim folded in), H[nc][nc] = sum_m Gd[m] (the objectives' row sums); dim == 2, n <= 15, 4R <= 1000 also:
// Wn[2n+1][nc] and W2n[4n+1][2n+1] (equal-degree product weights), E4[4n+1][4(n+R)+1] (elevation by 4R).
static int jac_tables(obtg_ctx* c)
{
    if (c->jac_R == c->R) return OBTG_OK;
    const int n = c->deg, nc = n + 1, R = c->R, L = 2 * n + R + 1;
    std::vector<double> t((size_t)L * nc * nc + (size_t)nc * nc, 0.0);
    const long double den_d = 0.5L * c->dim * 2.0L;    // (d/2) of normSquare, times 2 of the derivative
    for (int m = 0; m < L; ++m) {
        const long double inv = 1.0L / binom_l(2 * n + R, m);
        for (int i = 0; i < nc; ++i)
            for (int j = 0; j < nc; ++j) {
                const int r = m - i - j;
                if (r < 0 || r > R) continue;
                const double g = (double)(den_d * binom_l(n, i) * binom_l(n, j) * binom_l(R, r) * inv);
                t[((size_t)m * nc + i) * nc + j] = g;
                t[(size_t)L * nc * nc + (size_t)i * nc + j] += g;
            }
    }
    c->jac_off_ang = -1;
    if (c->dim == 2 && n <= 15 && 4 * R <= 1000) {
        c->jac_off_ang = (long long)t.size();
        const int L2 = 2 * n + 1, L4 = 4 * n + 1, La = 4 * (n + R) + 1;
        for (int k = 0; k < L2; ++k)
            for (int i = 0; i < nc; ++i)
                t.push_back(k - i >= 0 && k - i <= n ? (double)(binom_l(n, i) * binom_l(n, k - i) / binom_l(2 * n, k)) : 0.0);
        for (int k = 0; k < L4; ++k)
            for (int i = 0; i < L2; ++i)
                t.push_back(k - i >= 0 && k - i <= 2 * n ? (double)(binom_l(2 * n, i) * binom_l(2 * n, k - i) / binom_l(4 * n, k)) : 0.0);
        for (int j = 0; j < L4; ++j)
            for (int k = 0; k < La; ++k)
                t.push_back(k - j >= 0 && k - j <= 4 * R ? (double)(binom_l(4 * n, j) * binom_l(4 * R, k - j) / binom_l(4 * (n + R), k))
                                                          : 0.0);
    }
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));       // a launch in flight may still read the previous R's table
    int rc = c->d_jac.reserve(t.size() * sizeof(double));
    if (rc) return rc;
    OBTG_HIP(c, hipMemcpyAsync(c->d_jac.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->jac_R = R;
    return OBTG_OK;
}

// ------------------------------------------------------------------------------------------------ device helpers
// diff's matrix: A[i][q] = coefficient of P_q in diff(P)_i, times T
__device__ inline double diff_coef(int i, int q, int n)
{
    return q == i - 1 ? -(double)i : q == i ? (double)(2 * i - n) : q == i + 1 ? (double)(n - i) : 0.0;
}

// (A^T g)_q / (1/T): the pull-back of a gradient with respect to diff(P) onto P
__device__ inline double diff_pullback(const double* g, int q, int n)
{
    double s = (double)(2 * q - n) * g[q];
    if (q + 1 <= n) s = fma(-(double)(q + 1), g[q + 1], s);
    if (q >= 1) s = fma((double)(n - q + 1), g[q - 1], s);
    return s;
}

// ------------------------------------------------------------------------------------------------ temporal separation
// out[B][P][L][d][nc]: d row / d P_a (the a side; the b side is its negation).  Pairs whose first object is an obstacle
// (both are) have no variable: zeros.
template <bool G_IN_LDS>
__global__ __launch_bounds__(kJacThreads) void k_tsep_jac(const double* __restrict__ Y, const double* __restrict__ obs,
                                                          const int* __restrict__ pairs, const double* __restrict__ G, int B,
                                                          int P, int n_veh, int dim, int nc, int L, int R, double* __restrict__ out)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, gsize = L * nc * nc, dn = dim * nc, per = L * dn;
    double* sD = lds + (G_IN_LDS ? gsize : 0);
    if (G_IN_LDS)
        for (int e = tid; e < gsize; e += kJacThreads) lds[e] = G[e];
    const double* g = G_IN_LDS ? lds : G;
    const int rows = n_veh * dim;
    for (long long item = blockIdx.x; item < (long long)B * P; item += gridDim.x) {
        const int b = (int)(item / P), p = (int)(item - (long long)b * P);
        const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
        __syncthreads();                         // sD of the previous pair consumed (and G staged)
        if (tid < dn && ia < n_veh) {
            const int cc = tid / nc, j = tid - cc * nc;
            const double* Yb = Y + (size_t)b * rows * nc;
            const double va = Yb[(size_t)(ia * dim + cc) * nc + j];
            const double vb = ib < n_veh ? Yb[(size_t)(ib * dim + cc) * nc + j] : obs[(size_t)(ib - n_veh) * dim + cc];
            sD[tid] = va - vb;
        }
        __syncthreads();
        double* o = out + (size_t)item * per;
        for (int e = tid; e < per; e += kJacThreads) {
            const int m = e / dn, r = e - m * dn, cc = r / nc, i = r - cc * nc;
            double s = 0.0;
            if (ia < n_veh) {
                const int jlo = max(0, m - i - R), jhi = min(nc - 1, m - i);
                const double* gr = g + ((size_t)m * nc + i) * nc;
                const double* dd = sD + cc * nc;
                for (int j = jlo; j <= jhi; ++j) s = fma(gr[j], dd[j], s);
            }
            o[e] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ speed
// One workgroup per (row, vehicle).  out[B][N][L][d][nc] = sign d v_m / d P_cq, out_tf[B][N][L] = sign d v_m / d tf
// (v scales as tf^-2), sign = -1 for the max bound (bound^2 - v), +1 for the min bound.
__global__ __launch_bounds__(kJacThreads) void k_speed_jac(const double* __restrict__ Y, const double* __restrict__ tf,
                                                           const double* __restrict__ G, int N, int dim, int nc, int L, int R,
                                                           double sign, double* __restrict__ out, double* __restrict__ out_tf)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, v = blockIdx.x, b = blockIdx.y, n = nc - 1, dn = dim * nc;
    double* sD = lds;                 // diff(P)        [d][nc]
    double* sg = lds + dn;            // d v_m / d D    [L][d][nc]
    const double T = tf[b], invT = 1.0 / T;
    const double* P = Y + ((size_t)b * N + v) * dn;
    if (tid < dn) {
        const int cc = tid / nc, i = tid - cc * nc;
        double s = 0.0;
        for (int q = max(0, i - 1); q <= min(n, i + 1); ++q) s = fma(diff_coef(i, q, n), P[cc * nc + q], s);
        sD[tid] = s * invT;
    }
    __syncthreads();
    const int per = L * dn;
    for (int e = tid; e < per; e += kJacThreads) {
        const int m = e / dn, r = e - m * dn, cc = r / nc, i = r - cc * nc;
        const int jlo = max(0, m - i - R), jhi = min(nc - 1, m - i);
        const double* gr = G + ((size_t)m * nc + i) * nc;
        double s = 0.0;
        for (int j = jlo; j <= jhi; ++j) s = fma(gr[j], sD[cc * nc + j], s);
        sg[e] = s;
    }
    __syncthreads();
    double* o = out + ((size_t)b * N + v) * per;
    for (int e = tid; e < per; e += kJacThreads) {
        const int m = e / dn, r = e - m * dn, cc = r / nc, q = r - cc * nc;
        o[e] = sign * invT * diff_pullback(sg + (size_t)m * dn + cc * nc, q, n);
    }
    if (out_tf)
        for (int m = tid; m < L; m += kJacThreads) {
            double s = 0.0;                      // v_m = (1/2) sum D g_m: the row's value (G carries the factor 2)
            for (int k = 0; k < dn; ++k) s = fma(sD[k], sg[(size_t)m * dn + k], s);
            out_tf[((size_t)b * N + v) * L + m] = sign * (-2.0 * 0.5 * s * invT);
        }
}

// ------------------------------------------------------------------------------------------------ angular rate
// One workgroup per (row, vehicle), dim 2.  With d1 = diff(P), d2 = diff(d1) (degree n each):
//   q = d2_y d1_x - d2_x d1_y, s = |d1|^2 (degree 2n);  num = q^2, den = s^2 (degree 4n), elevated by 4R;
//   row_k = max_rate^2 - num_k / den_k,   d row_k = -(d num_k - r_k d den_k) / den_k,   d row_k / d tf = 2 r_k / tf.
// Variable u = c (n+1) + r is control point r of coordinate c.  A row whose quotient is not finite gets NaN.
__global__ __launch_bounds__(kJacThreads) void k_ang_rate_jac(const double* __restrict__ Y, const double* __restrict__ tf,
                                                              const double* __restrict__ W, int N, int nc, int R,
                                                              double* __restrict__ out, double* __restrict__ out_tf)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, v = blockIdx.x, b = blockIdx.y, n = nc - 1, NV = 2 * nc;
    const int L2 = 2 * n + 1, L4 = 4 * n + 1, La = 4 * (n + R) + 1, R4 = 4 * R;
    const double* Wn = W;                                 // [L2][nc]
    const double* W2n = Wn + (size_t)L2 * nc;             // [L4][L2]
    const double* E4 = W2n + (size_t)L4 * L2;             // [L4][La]
    double* sA = lds;                 // A / T         [nc][nc]
    double* sA2 = sA + nc * nc;       // (A / T)^2     [nc][nc]
    double* s1 = sA2 + nc * nc;       // d1            [2][nc]
    double* s2 = s1 + 2 * nc;         // d2            [2][nc]
    double* sq = s2 + 2 * nc;         // q, s          [2][L2]
    double* sdq = sq + 2 * L2;        // dq_u, ds_u    [NV][2][L2]
    double* snd = sdq + NV * 2 * L2;  // num, den      [2][L4]
    double* sdn = snd + 2 * L4;       // dnum_u, dden_u [NV][2][L4]
    double* se = sdn + NV * 2 * L4;   // elevated num, den [2][La]
    const double T = tf[b], invT = 1.0 / T;
    const double* P = Y + ((size_t)b * N + v) * NV;
    for (int e = tid; e < nc * nc; e += kJacThreads) sA[e] = diff_coef(e / nc, e % nc, n) * invT;
    __syncthreads();
    for (int e = tid; e < nc * nc; e += kJacThreads) {
        const int i = e / nc, q = e - i * nc;
        double s = 0.0;
        for (int l = 0; l < nc; ++l) s = fma(sA[i * nc + l], sA[l * nc + q], s);
        sA2[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < 4 * nc; e += kJacThreads) {
        const int which = e / NV, r = e - which * NV, cc = r / nc, i = r - cc * nc;
        const double* M = which ? sA2 : sA;
        double s = 0.0;
        for (int q = 0; q < nc; ++q) s = fma(M[i * nc + q], P[cc * nc + q], s);
        (which ? s2 : s1)[r] = s;
    }
    __syncthreads();
    // degree-2n products: q, s and their derivatives (u: coordinate c = u / nc, control point r = u % nc)
    for (int e = tid; e < (NV + 1) * 2 * L2; e += kJacThreads) {
        const int u = e / (2 * L2) - 1, w = (e / L2) & 1, k = e % L2;
        double acc = 0.0;
        for (int i = max(0, k - n); i <= min(n, k); ++i) {
            const int j = k - i;
            double t;
            if (u < 0) {
                t = w == 0 ? s2[nc + i] * s1[j] - s2[i] * s1[nc + j] : s1[i] * s1[j] + s1[nc + i] * s1[nc + j];
            } else {
                const int cc = u / nc, r = u - cc * nc;
                const double a_j = sA[j * nc + r], a2_i = sA2[i * nc + r];
                if (w == 0)    // d q: x: d2_y a - a2 d1_y ; y: a2 d1_x - d2_x a
                    t = cc == 0 ? s2[nc + i] * a_j - a2_i * s1[nc + j] : a2_i * s1[j] - s2[i] * a_j;
                else           // d s = 2 d1_c a
                    t = 2.0 * s1[cc * nc + i] * a_j;
            }
            acc = fma(Wn[(size_t)k * nc + i], t, acc);
        }
        (u < 0 ? sq : sdq + (size_t)u * 2 * L2)[w * L2 + k] = acc;
    }
    __syncthreads();
    // degree-4n products: num = q q, den = s s, d num = 2 q dq, d den = 2 s ds
    for (int e = tid; e < (NV + 1) * 2 * L4; e += kJacThreads) {
        const int u = e / (2 * L4) - 1, w = (e / L4) & 1, k = e % L4;
        const double* f = sq + w * L2;
        const double* h = u < 0 ? f : sdq + (size_t)u * 2 * L2 + w * L2;
        double acc = 0.0;
        for (int i = max(0, k - 2 * n); i <= min(2 * n, k); ++i) acc = fma(W2n[(size_t)k * L2 + i], f[i] * h[k - i], acc);
        (u < 0 ? snd : sdn + (size_t)u * 2 * L4)[w * L4 + k] = u < 0 ? acc : 2.0 * acc;
    }
    __syncthreads();
    for (int e = tid; e < 2 * La; e += kJacThreads) {
        const int w = e / La, k = e - w * La;
        double acc = 0.0;
        for (int j = max(0, k - R4); j <= min(L4 - 1, k); ++j) acc = fma(E4[(size_t)j * La + k], snd[w * L4 + j], acc);
        se[e] = acc;
    }
    __syncthreads();
    double* o = out + ((size_t)b * N + v) * La * NV;
    for (int e = tid; e < La * NV; e += kJacThreads) {
        const int k = e / NV, u = e - k * NV;
        const double num = se[k], den = se[La + k], rk = num / den;
        double dn_ = 0.0, dd_ = 0.0;
        const double* pn = sdn + (size_t)u * 2 * L4;
        for (int j = max(0, k - R4); j <= min(L4 - 1, k); ++j) {
            const double ej = E4[(size_t)j * La + k];
            dn_ = fma(ej, pn[j], dn_);
            dd_ = fma(ej, pn[L4 + j], dd_);
        }
        o[e] = isfinite(rk) ? -(dn_ - rk * dd_) / den : NAN;
    }
    if (out_tf)
        for (int k = tid; k < La; k += kJacThreads) {
            const double rk = se[k] / se[La + k];
            out_tf[((size_t)b * N + v) * La + k] = isfinite(rk) ? 2.0 * rk * invT : NAN;
        }
}

// ------------------------------------------------------------------------------------------------ objectives
// euclidean (optimization.py:462-489): f = sum |P_{i+1} - P_i|, d f / d P_i = u_{i-1} - u_i with u_i the unit segment
// (a zero-length segment gives NaN).  One workgroup per row, out[B][N d][nc].
__global__ __launch_bounds__(kJacThreads) void k_euclid_grad(const double* __restrict__ Y, int N, int dim, int nc,
                                                             double* __restrict__ out)
{
    const int b = blockIdx.x, n = nc - 1;
    const double* Yb = Y + (size_t)b * N * dim * nc;
    for (int e = threadIdx.x; e < N * dim * nc; e += kJacThreads) {
        const int row = e / nc, i = e - row * nc, v = row / dim, cc = row - v * dim;
        const double* Pv = Yb + (size_t)v * dim * nc;
        double g = 0.0;
        for (int seg = i - 1; seg <= i; ++seg) {
            if (seg < 0 || seg >= n) continue;
            double q = 0.0;
            for (int k = 0; k < dim; ++k) {
                const double t = Pv[k * nc + seg + 1] - Pv[k * nc + seg];
                q = fma(t, t, q);
            }
            const double u = (Pv[cc * nc + seg + 1] - Pv[cc * nc + seg]) / sqrt(q);
            g += seg == i - 1 ? u : -u;
        }
        out[(size_t)b * N * dim * nc + e] = g;
    }
}

// accel (order 2) / jerk (order 3), optimization.py:503-539: f = sum_v sum_m (d/2) sum G_mij <Q_i, Q_j>, Q = diff^order(P);
// d f / d Q = H Q (H = sum_m Gd_m), pulled back through diff `order` times.  out[B][N d][nc], out_tf[B] (f ~ tf^(-2 order)).
// One workgroup per row.
__global__ __launch_bounds__(kJacThreads) void k_deriv_energy_grad(const double* __restrict__ Y, const double* __restrict__ tf,
                                                                   const double* __restrict__ H, int N, int dim, int nc, int order,
                                                                   double* __restrict__ out, double* __restrict__ out_tf)
{
    extern __shared__ double lds[];
    const int b = blockIdx.x, n = nc - 1, rows = N * dim, len = rows * nc, tid = threadIdx.x;
    double* a = lds;
    double* c2 = lds + len;
    double* red = c2 + len;           // [kJacThreads]
    const double invT = 1.0 / tf[b];
    const double* Yb = Y + (size_t)b * len;
    for (int e = tid; e < len; e += kJacThreads) a[e] = Yb[e];
    __syncthreads();
    for (int k = 0; k < order; ++k) {           // Q = diff^order(P), row by row
        double* src = (k & 1) ? c2 : a;
        double* dst = (k & 1) ? a : c2;
        for (int e = tid; e < len; e += kJacThreads) {
            const int row = e / nc, i = e - row * nc;
            double s = 0.0;
            for (int q = max(0, i - 1); q <= min(n, i + 1); ++q) s = fma(diff_coef(i, q, n), src[row * nc + q], s);
            dst[e] = s * invT;
        }
        __syncthreads();
    }
    double* Q = (order & 1) ? c2 : a;
    double* g = (order & 1) ? a : c2;
    double part = 0.0;
    for (int e = tid; e < len; e += kJacThreads) {
        const int row = e / nc, i = e - row * nc;
        double s = 0.0;
        for (int j = 0; j < nc; ++j) s = fma(H[i * nc + j], Q[row * nc + j], s);
        g[e] = s;
        part = fma(0.5 * s, Q[e], part);        // f = (1/2) sum Q (H Q)
    }
    red[tid] = part;
    __syncthreads();
    for (int k = 0; k < order; ++k) {
        double* src = (k & 1) ? Q : g;
        double* dst = (k & 1) ? g : Q;
        for (int e = tid; e < len; e += kJacThreads) {
            const int row = e / nc, q = e - row * nc;
            dst[e] = diff_pullback(src + row * nc, q, n) * invT;
        }
        __syncthreads();
    }
    double* res = (order & 1) ? Q : g;
    for (int e = tid; e < len; e += kJacThreads) out[(size_t)b * len + e] = res[e];
    if (out_tf && tid == 0) {
        double f = 0.0;
        for (int k = 0; k < kJacThreads; ++k) f += red[k];
        out_tf[b] = -2.0 * order * f * invT;
    }
}

// ------------------------------------------------------------------------------------------------ launchers
int launch_temporal_sep_jac(obtg_ctx* c, const double* dY, int B, double* d_out)
{
    if (B <= 0 || c->n_pairs == 0) return OBTG_OK;
    int rc = jac_tables(c);
    if (rc) return rc;
    const int nc = c->deg + 1, L = 2 * c->deg + c->R + 1;
    const size_t gbytes = sizeof(double) * (size_t)L * nc * nc, dbytes = sizeof(double) * c->dim * nc;
    const bool in_lds = gbytes <= kJacLdsG;
    const long long items = (long long)B * c->n_pairs;
    const unsigned grid = (unsigned)std::min<long long>(items, (long long)c->n_cus * (in_lds ? 2 : 8));
    ScopedKernelTimer t(c, OBTG_K_JAC);
    if (in_lds)
        hipLaunchKernelGGL(k_tsep_jac<true>, dim3(grid), dim3(kJacThreads), gbytes + dbytes, c->stream, dY, c->d_obs.as<double>(),
                           c->d_pairs.as<int>(), c->d_jac.as<double>(), B, c->n_pairs, c->n_veh, c->dim, nc, L, c->R, d_out);
    else
        hipLaunchKernelGGL(k_tsep_jac<false>, dim3(grid), dim3(kJacThreads), dbytes, c->stream, dY, c->d_obs.as<double>(),
                           c->d_pairs.as<int>(), c->d_jac.as<double>(), B, c->n_pairs, c->n_veh, c->dim, nc, L, c->R, d_out);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_speed_jac(obtg_ctx* c, const double* dY, const double* d_tf, int B, int is_max, double* d_out, double* d_out_tf)
{
    if (B <= 0) return OBTG_OK;
    int rc = jac_tables(c);
    if (rc) return rc;
    const int nc = c->deg + 1, L = 2 * c->deg + c->R + 1;
    const size_t lds = sizeof(double) * ((size_t)c->dim * nc + (size_t)L * c->dim * nc);
    if (lds > 64 * 1024) return OBTG_ERR_UNSUPPORTED;
    ScopedKernelTimer t(c, OBTG_K_JAC);
    hipLaunchKernelGGL(k_speed_jac, dim3(c->n_veh, B), dim3(kJacThreads), lds, c->stream, dY, d_tf, c->d_jac.as<double>(), c->n_veh,
                       c->dim, nc, L, c->R, is_max ? -1.0 : 1.0, d_out, d_out_tf);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

size_t ang_rate_jac_lds_bytes(int n, int R)
{
    const size_t nc = n + 1, NV = 2 * nc, L2 = 2 * n + 1, L4 = 4 * n + 1, La = 4 * (n + R) + 1;
    return sizeof(double) * (2 * nc * nc + 4 * nc + 2 * L2 + NV * 2 * L2 + 2 * L4 + NV * 2 * L4 + 2 * La);
}

int launch_ang_rate_jac(obtg_ctx* c, const double* dY, const double* d_tf, int B, double* d_out, double* d_out_tf)
{
    if (c->dim != 2) return OBTG_ERR_ARG;
    if (B <= 0) return OBTG_OK;
    int rc = jac_tables(c);
    if (rc) return rc;
    if (c->jac_off_ang < 0) return OBTG_ERR_UNSUPPORTED;            // deg > 15 or 4 R > 1000
    const size_t lds = ang_rate_jac_lds_bytes(c->deg, c->R);
    if (lds > 64 * 1024) return OBTG_ERR_UNSUPPORTED;
    ScopedKernelTimer t(c, OBTG_K_JAC);
    hipLaunchKernelGGL(k_ang_rate_jac, dim3(c->n_veh, B), dim3(kJacThreads), lds, c->stream, dY, d_tf,
                       c->d_jac.as<double>() + c->jac_off_ang, c->n_veh, c->deg + 1, c->R, d_out, d_out_tf);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_euclidean_grad(obtg_ctx* c, const double* dY, int B, double* d_out)
{
    if (B <= 0) return OBTG_OK;
    ScopedKernelTimer t(c, OBTG_K_JAC);
    hipLaunchKernelGGL(k_euclid_grad, dim3(B), dim3(kJacThreads), 0, c->stream, dY, c->n_veh, c->dim, c->deg + 1, d_out);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_deriv_energy_grad(obtg_ctx* c, const double* dY, const double* d_tf, int B, int order, double* d_out, double* d_out_tf)
{
    if (order < 1 || order > 4) return OBTG_ERR_ARG;
    if (B <= 0) return OBTG_OK;
    int rc = jac_tables(c);
    if (rc) return rc;
    const int nc = c->deg + 1, L = 2 * c->deg + c->R + 1;
    const size_t lds = sizeof(double) * (2 * (size_t)c->n_veh * c->dim * nc + kJacThreads);
    if (lds > 64 * 1024) return OBTG_ERR_UNSUPPORTED;
    ScopedKernelTimer t(c, OBTG_K_JAC);
    hipLaunchKernelGGL(k_deriv_energy_grad, dim3(B), dim3(kJacThreads), lds, c->stream, dY, d_tf,
                       c->d_jac.as<double>() + (size_t)L * nc * nc, c->n_veh, c->dim, nc, order, d_out, d_out_tf);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

}  // namespace obtg
