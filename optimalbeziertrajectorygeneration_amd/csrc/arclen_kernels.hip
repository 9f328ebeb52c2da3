// True arc length of Bezier curves for gfx950 (MI355X): obtg_bern_arc_length and the objective obtg_arc_length_obj
// (include/obtg.h states the contract).  What the reference has here is the length of the control polygon
// (optimization.py:462-489 _euclideanObjective), an upper bound of this quantity; nothing of the reference integrates along a curve.
//
// Rule: L = int_0^1 |c'(t)| dt by adaptive bisection with the 8-point Gauss-Legendre rule per panel.  A panel [a, a + w] has
// the nodes t_k = fma(w, h_k, a), h_k = (1 + x_k) / 2, and the estimate G = w sum_k g_k |c'(t_k)|, g_k = omega_k / 2.  Its two
// halves are evaluated together; it is accepted when |G - (G_l + G_r)| <= tol w, tol = eps_rel S, S the length of the control
// polygon (a majorant of L known before the search), and then contributes G_l + G_r to len and |G - G_l - G_r| to err.  Else
// the right half waits on a stack and the left half is next: depth first, left to right, a and w dyadic and so exact.  A panel
// of width 2^-48 is accepted whatever the test says (OBTG_MD_DEPTH_CAP); once max_nodes panel estimates are used up, the
// panels that wait are accepted with the estimate they have (OBTG_MD_NODE_CAP) and add nothing to err.
// The sum is returned inside [chord, S], the bracket L lies in: one that passes an end (the quadrature's error can exceed the
// room a straight or a monotone one-dimensional curve leaves) is that end, and grad the end's gradient.
//
// Floor of eps_rel: one estimate is K = 3 n + d + 9 rounded operations deep (n = degree, d = dimension: the node 1, the basis
// 2 (n - 1), a difference of control points 1, a velocity component n + 1, the norm d + 1, weight, 8-term sum and width 5,
// G_l + G_r 1), relative to n sum_i B_i |P_(i+1) - P_i| <= n S.  So rounding alone can put |G - G_l - G_r| at 2 K n 2^-53 S w,
// and an eps_rel below 2 K n 2^-53 is raised to that (degree 10, planar: 9.1e-14; degree 31 in space: 7.2e-13).
//
// Kernel form: one curve per 16-lane ROW of the wavefront (four curves per wave, one wave per workgroup).  Lanes 0-7 of the
// row are the 8 nodes of the left half, lanes 8-15 those of the right half.  A lane evaluates the curve's hodograph at its
// own global parameter: the Bernstein basis B^(n-1)(t) by the de Casteljau recurrence on the basis (as bern_device.h
// envelope_block: products and sums of non-negative numbers) in registers, then c'_c(t) = n sum_i B_i (P_c,i+1 - P_c,i) in
// index order, the differences read from the row's block of LDS.  So a waiting panel is (a, w, G) and no coefficients, and the
// basis is at hand for the gradient.  The 8-term sums are a fixed-order butterfly over the row's half (1, 2, 4), which
// leaves the same bits in every lane.  Every branch below depends on values that are the same in all lanes of a row.
//
// Gradient (the same launch): for every node of an accepted pair, with q_k = w g_k and u = c'(t_k) / |c'(t_k)|,
//     grad[c][i] += q_k u_c n (B_(i-1)^(n-1)(t_k) - B_i^(n-1)(t_k)),     B_(-1) = B_n = 0,
// the derivative of the returned len for the panel set the search ended on (a node with |c'| = 0 adds nothing; under
// OBTG_MD_NODE_CAP the waiting panels' nodes are evaluated once more for it).  A lane sums A[c][j] = sum q_k u_c B_j in
// registers, one butterfly over the row (1, 2, 4, 8) at the end, grad[c][i] = n (A[c][i-1] - A[c][i]).
// At a cusp the integrand of the gradient jumps (u turns around) while that of the length only has a kink: the gradient's
// error there is a larger multiple of eps_rel than the value's (a CPU prototype: 1.5e-9 at eps_rel = 1e-10).
//
// NCMAX: the template bound on the control points; every loop is unrolled over it and guarded by the run-time count, and every
// multiply-add is an explicit fma (the unit is compiled with -ffp-contract=off), so a curve's bits do not depend on the
// instantiation that serves it, nor on M, its row, the other rows or the entry point.
#include <cfloat>

#include "obtg_internal.h"

namespace obtg {

constexpr int kArcRows = 4;            // curves per wave: a 16-lane row each
constexpr int kArcDepth = 48;          // bisections below [0, 1]: a panel of width 2^-48 is accepted
constexpr int kArcMaxNC = 32;

// h_k = (1 + x_k) / 2 and g_k = omega_k / 2 of the 8-point rule, each the binary64 nearest to the 60-digit value
// (tests/arc_length_ref.py kernel_constants)
__device__ const double kArcH[8] = { 0x1.454e34f533998p-6, 0x1.a06d536d82f88p-4, 0x1.e5dad4f9af698p-3, 0x1.a214dac30e32fp-2,
                                     0x1.2ef5929e78e69p-1, 0x1.86894ac19425ap-1, 0x1.cbf255924fa0fp-1, 0x1.f5d58e5856633p-1 };
__device__ const double kArcG[8] = { 0x1.9ea1d04ca0374p-5, 0x1.c76fb531d2b96p-4, 0x1.413c50a255615p-3, 0x1.736360b199343p-3,
                                     0x1.736360b199343p-3, 0x1.413c50a255615p-3, 0x1.c76fb531d2b96p-4, 0x1.9ea1d04ca0374p-5 };

struct ArcParams {
    const double* __restrict__ c;      // [M][DIM][K]
    double* __restrict__ len;          // [M]
    double* __restrict__ err;          // [M] nullable
    int* __restrict__ nodes;           // [M] nullable
    int* __restrict__ status;          // [M] nullable
    double* __restrict__ grad;         // [M][DIM][K] (the GRAD kernels)
    long M;
    int K, max_nodes;
    double eps_rel;                    // not below the floor (the launcher has seen to it)
};

__host__ __device__ inline double arc_eps_floor(int n, int dim) { return 2.0 * n * (3 * n + dim + 9) * 0x1p-53; }

__device__ __forceinline__ double arc_row_xor(double v, int o) { return __shfl_xor(v, o, 16); }
__device__ __forceinline__ double arc_sum8(double v)
{
    v += arc_row_xor(v, 1); v += arc_row_xor(v, 2); v += arc_row_xor(v, 4);
    return v;
}

// doubles of LDS per row: the hodograph's differences [DIM][n], then the stack of (a, w, G)
__host__ __device__ inline int arc_row_doubles(int dim, int nc) { return dim * (nc - 1) + 3 * kArcDepth; }

template <int NCMAX, int DIM, bool GRAD>
__global__ __launch_bounds__(kWave) void k_arc_length(const ArcParams p)
{
    constexpr int NH = NCMAX - 1;                 // the hodograph's coefficients, at most
    extern __shared__ double lds[];
    const int lane = threadIdx.x, row = lane >> 4, l16 = lane & 15;
    const bool right = (l16 & 8) != 0;
    const int nc = p.K, n = nc - 1;
    const long curve = (long)blockIdx.x * kArcRows + row;
    if (curve >= p.M) return;                     // the whole row leaves; nothing below synchronises across rows
    double* dh = lds + (size_t)row * arc_row_doubles(DIM, nc);
    double* stk = dh + DIM * n;
    const double* P = p.c + (size_t)curve * DIM * nc;
    const double hk = kArcH[l16 & 7], gk = kArcG[l16 & 7], nn = (double)n;

    int bad = 0;
    for (int e = l16; e < DIM * n; e += 16) {
        const int c = e / n, i = e - c * n;
        const double p0 = P[c * nc + i], p1 = P[c * nc + i + 1];
        bad |= !(fabs(p0) <= DBL_MAX) || !(fabs(p1) <= DBL_MAX);
        dh[e] = p1 - p0;
    }
    bad |= __shfl_xor(bad, 1, 16); bad |= __shfl_xor(bad, 2, 16); bad |= __shfl_xor(bad, 4, 16); bad |= __shfl_xor(bad, 8, 16);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double S = 0.0;                               // the control polygon's length, segment by segment in index order
    for (int i = 0; i < n; ++i) {
        double q = dh[i] * dh[i];
#pragma unroll
        for (int c = 1; c < DIM; ++c) q = fma(dh[c * n + i], dh[c * n + i], q);
        S += __builtin_sqrt(q);
    }
    if (bad || !(S <= DBL_MAX)) {                 // a non-finite control point (or a polygon that overflows): NaN, as obtg_bern_extrema
        const double nan = __builtin_nan("");
        if (l16 == 0) {
            p.len[curve] = nan;
            if (p.err) p.err[curve] = nan;
            if (p.nodes) p.nodes[curve] = 0;
            if (p.status) p.status[curve] = OBTG_MD_OK;
        }
        if (GRAD)
            for (int e = l16; e < DIM * nc; e += 16) p.grad[(size_t)curve * DIM * nc + e] = nan;
        return;
    }
    const double tol = p.eps_rel * S;

    double wb[NH], v[DIM];
    // |c'(t)|; wb: B^(n-1)(t), v: c'(t)
    auto eval = [&](const double t) -> double {
        const double s = 1.0 - t;
#pragma unroll
        for (int i = 0; i < NH; ++i) wb[i] = i == 0 ? 1.0 : 0.0;
#pragma unroll
        for (int r = 1; r < NH; ++r)
            if (r < n) {
#pragma unroll
                for (int i = r; i >= 1; --i) wb[i] = fma(t, wb[i - 1], s * wb[i]);
                wb[0] = s * wb[0];
            }
        double ss = 0.0;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            double dl = 0.0;
#pragma unroll
            for (int i = 0; i < NH; ++i)
                if (i < n) dl = fma(wb[i], dh[c * n + i], dl);
            v[c] = nn * dl;
            ss = c == 0 ? v[c] * v[c] : fma(v[c], v[c], ss);
        }
        return __builtin_sqrt(ss);
    };
    double A[GRAD ? DIM : 1][GRAD ? NH : 1];
    if (GRAD) {
#pragma unroll
        for (int c = 0; c < DIM; ++c)
#pragma unroll
            for (int j = 0; j < NH; ++j) A[c][j] = 0.0;
    }
    // this lane's node of weight q, as eval left it
    auto gather = [&](const double q, const double speed) {
        if (!GRAD) return;
        const double f = speed > 0.0 ? q / speed : 0.0;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const double fc = f * v[c];
#pragma unroll
            for (int j = 0; j < NH; ++j)
                if (j < n) A[c][j] = fma(fc, wb[j], A[c][j]);
        }
    };

    // the root: both halves of the row on [0, 1]
    double a = 0.0, w = 1.0;
    double G = arc_sum8(gk * eval(fma(1.0, hk, 0.0)));
    double len = 0.0, err = 0.0;
    int nodes = 1, sp = 0, status = OBTG_MD_OK;
    bool capped = false;
    for (;;) {
        if (nodes > p.max_nodes - 2) { capped = true; break; }
        const double hw = 0.5 * w;
        const double speed = eval(fma(hw, hk, right ? a + hw : a));
        const double part = hw * arc_sum8(gk * speed), other = arc_row_xor(part, 8);
        const double Gl = right ? other : part, Gr = right ? part : other;
        nodes += 2;
        const double both = Gl + Gr, e = fabs(G - both);
        const bool ok = e <= tol * w;
        if (ok || w <= 0x1p-48) {
            if (!ok) status = OBTG_MD_DEPTH_CAP;
            len += both;
            err += e;
            gather(hw * gk, speed);
            if (sp == 0) break;
            --sp;
            a = stk[3 * sp]; w = stk[3 * sp + 1]; G = stk[3 * sp + 2];
        } else {
            if (l16 == 0) { stk[3 * sp] = a + hw; stk[3 * sp + 1] = hw; stk[3 * sp + 2] = Gr; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            ++sp;
            w = hw; G = Gl;
        }
    }
    if (capped) {                                 // what waits is accepted as it is: the current panel, then the stack from its top
        if (status == OBTG_MD_OK) status = OBTG_MD_NODE_CAP;
        for (;;) {
            len += G;
            if (GRAD) {
                const double speed = eval(fma(w, hk, a));
                gather(right ? 0.0 : w * gk, speed);
            }
            if (sp == 0) break;
            --sp;
            a = stk[3 * sp]; w = stk[3 * sp + 1]; G = stk[3 * sp + 2];
        }
    }
    // The bracket every curve's length lies in, chord <= L <= S: a sum that leaves it (a quadrature error larger than the room
    // the curve leaves, as on a straight or a monotone one-dimensional curve) is moved to the end it passed, which is nearer to L,
    // and the gradient is then that end's.  Both ends as rounded here; a NaN sum compares false and stays.
    double ce[DIM], chord;
    {
        double q = 0.0;
#pragma unroll
        for (int c = 0; c < DIM; ++c) { ce[c] = P[c * nc + n] - P[c * nc]; q = c == 0 ? ce[c] * ce[c] : fma(ce[c], ce[c], q); }
        chord = __builtin_sqrt(q);
    }
    int clamp = 0;
    if (len > S) { len = S; clamp = 1; }
    else if (len < chord) { len = chord; clamp = -1; }
    if (l16 == 0) {
        p.len[curve] = len;
        if (p.err) p.err[curve] = err;
        if (p.nodes) p.nodes[curve] = nodes;
        if (p.status) p.status[curve] = status;
    }
    if (GRAD && clamp > 0) {                      // dS/dP: the unit vectors of the two segments at a control point (a segment of length 0: none)
        double* g = p.grad + (size_t)curve * DIM * nc;
        for (int i = l16; i < nc; i += 16) {
            double qm = 0.0, qp = 0.0;
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const double dm = i >= 1 ? dh[c * n + (i >= 1 ? i - 1 : 0)] : 0.0, dp = i < n ? dh[c * n + (i < n ? i : 0)] : 0.0;
                qm = c == 0 ? dm * dm : fma(dm, dm, qm);
                qp = c == 0 ? dp * dp : fma(dp, dp, qp);
            }
            qm = __builtin_sqrt(qm); qp = __builtin_sqrt(qp);
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const double um = qm > 0.0 ? dh[c * n + (i >= 1 ? i - 1 : 0)] / qm : 0.0, up = qp > 0.0 ? dh[c * n + (i < n ? i : 0)] / qp : 0.0;
                g[c * nc + i] = um - up;
            }
        }
    } else if (GRAD && clamp < 0) {               // d chord / dP: the chord's unit vector at the two ends (chord > len >= 0 here)
        double* g = p.grad + (size_t)curve * DIM * nc;
        for (int i = l16; i < nc; i += 16)
#pragma unroll
            for (int c = 0; c < DIM; ++c) g[c * nc + i] = i == 0 ? -(ce[c] / chord) : i == n ? ce[c] / chord : 0.0;
    } else if (GRAD) {
        double* g = p.grad + (size_t)curve * DIM * nc;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                double s = A[c][j];
                s += arc_row_xor(s, 1); s += arc_row_xor(s, 2); s += arc_row_xor(s, 4); s += arc_row_xor(s, 8);
                A[c][j] = s;
            }
#pragma unroll
            for (int i = 0; i < NCMAX; ++i)
                if (i < nc && (i & 15) == l16)
                    g[c * nc + i] = nn * ((i >= 1 ? A[c][i - 1] : 0.0) - (i < n ? A[c][i < NH ? i : 0] : 0.0));
        }
    }
}

// obtg_arc_length_obj's last step: out[b] = sum_v len[b][v] in vehicle order, status[b] the worst of the row's vehicles
__global__ __launch_bounds__(kWave) void k_arc_rowsum(const double* __restrict__ len, const int* __restrict__ st, int B, int n_veh,
                                                      double* __restrict__ out, int* __restrict__ status)
{
    const int b = blockIdx.x * kWave + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    int worst = OBTG_MD_OK;
    for (int v = 0; v < n_veh; ++v) {
        s += len[(size_t)b * n_veh + v];
        worst = st[(size_t)b * n_veh + v] > worst ? st[(size_t)b * n_veh + v] : worst;
    }
    out[b] = s;
    if (status) status[b] = worst;
}

// =====================================================================================
//  launchers
// =====================================================================================
bool arc_length_supported(int dim, int K) { return dim >= 1 && dim <= 3 && K >= 2 && K <= kArcMaxNC; }

// the instantiations: the control-point counts of OBTG_NC_SEP that are worth a kernel of their own, rounded up to the next
// of 6, 11, 16, 21; everything else at 32
#define OBTG_ARC_NC(X) X(6) X(11) X(16) X(21) X(32)

template <int DIM, bool GRAD>
static void (*arc_kernel(int nc))(const ArcParams)
{
#define OBTG_CASE(NC_) if (nc <= NC_) return k_arc_length<NC_, DIM, GRAD>;
    OBTG_ARC_NC(OBTG_CASE)
#undef OBTG_CASE
    return nullptr;
}

int launch_arc_length(obtg_ctx* c, const double* d_c, long M, int dim, int K, double eps_rel, int max_nodes, double* d_len,
                      double* d_err, int* d_nodes, int* d_status, double* d_grad)
{
    if (M <= 0) return OBTG_OK;
    if (!arc_length_supported(dim, K)) return OBTG_ERR_UNSUPPORTED;
    ArcParams p{};
    p.c = d_c; p.len = d_len; p.err = d_err; p.nodes = d_nodes; p.status = d_status; p.grad = d_grad;
    p.M = M; p.K = K; p.max_nodes = max_nodes;
    const double floor = arc_eps_floor(K - 1, dim);
    p.eps_rel = eps_rel < floor ? floor : eps_rel;
    void (*kern)(const ArcParams) = nullptr;
    if (d_grad) kern = dim == 1 ? arc_kernel<1, true>(K) : dim == 2 ? arc_kernel<2, true>(K) : arc_kernel<3, true>(K);
    else kern = dim == 1 ? arc_kernel<1, false>(K) : dim == 2 ? arc_kernel<2, false>(K) : arc_kernel<3, false>(K);
    if (!kern) return OBTG_ERR_UNSUPPORTED;
    const size_t lds = sizeof(double) * kArcRows * (size_t)arc_row_doubles(dim, K);
    ScopedKernelTimer t(c, OBTG_K_ARC_LENGTH);
    hipLaunchKernelGGL(kern, dim3((unsigned)((M + kArcRows - 1) / kArcRows)), dim3(kWave), lds, c->stream, p);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

int launch_arc_length_obj(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, double* d_out, int* d_status,
                          double* d_grad)
{
    if (B <= 0) return OBTG_OK;
    const size_t items = (size_t)B * c->n_veh;
    DevBuf& ws = c->ws_misc[WS_L_ROWS];           // len[B][n_veh], then status[B][n_veh]
    int rc = ws.reserve((sizeof(double) + sizeof(int)) * items);
    if (rc) return rc;
    double* d_len = ws.as<double>();
    int* d_st = reinterpret_cast<int*>(d_len + items);
    if ((rc = launch_arc_length(c, dY, (long)items, c->dim, c->deg + 1, eps_rel, max_nodes, d_len, nullptr, nullptr, d_st, d_grad)))
        return rc;
    ScopedKernelTimer t(c, OBTG_K_ARC_LENGTH);
    hipLaunchKernelGGL(k_arc_rowsum, dim3((unsigned)((B + kWave - 1) / kWave)), dim3(kWave), 0, c->stream, d_len, d_st, B,
                       c->n_veh, d_out, d_status);
    OBTG_HIP(c, hipGetLastError());
    return OBTG_OK;
}

}  // namespace obtg
