// Device functions of the keep-out rows (keepout_kernels.hip; include/obtg.h "keep-out obstacles"): a curve against a convex
// obstacle {p : a_f . p <= b_f}.  Per face f the polynomial g_f(t) = a_f . c(t) - b_f has the curve's own degree; the row is
//     min over t in [0, 1] of G(t),  G(t) = max over the obstacle's faces of g_f(t)      (> 0 outside, minus the depth inside).
// Every multiply-add below is an explicit fma and every other product stands alone: the same bits whatever contraction the
// including unit is compiled under.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "md_device.h"
#include "keepout_features.h"

namespace obtg {

constexpr int kKoMaxFaces = 16;      // faces per obstacle (above: OBTG_ERR_UNSUPPORTED)
constexpr int kKoMaxK = 32;          // control points per curve: a child of a split is half a wavefront
constexpr int kKoStack = 32;         // sub-curves waiting per item; one more: OBTG_MD_DEPTH_CAP
constexpr int kKoWaves = 2;          // waves (items) per workgroup

__device__ __forceinline__ void ko_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double ko_lane(double v, int src)      // src wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
// Smallest value of each 32-lane half, in every lane of the half.  (A DPP form -- quad_perm, row_half_mirror, row_mirror,
// row_bcast15 -- was measured 12 % SLOWER on C3's batch: the kernel is bound by issue, not by this chain's latency, and the
// register moves cost more issue slots than the five cross-lane reads.  DESIGN.md 4.24.)
__device__ __forceinline__ double ko_half_min(double v)
{
#pragma unroll
    for (int o = 16; o; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
constexpr int kKoLowLast = 0, kKoHighLast = 32;       // a lane of either half to read its minimum from
constexpr int kKoFeatRec = 7;        // doubles per feature record

// One wave's LDS, in doubles -- the ONE statement of the layout, for the kernel and for every launch's dynamic size:
//     kKoStack frames of (dim K + 3) | kKoMaxFaces faces of (dim + 1) | ed
//     ed: moving E[dim][K] | D[dim][K];  Euclidean: kKoMaxFeatures records;  pair: D[dim][K], behind the records where both
constexpr int ko_lds_pair_d(bool euclid) { return euclid ? kKoMaxFeatures * kKoFeatRec : 0; }      // D's offset in ed (pair forms)
// A macro and not a function, `pitch` (= dim K + 3) the kernel's own variable: token for token the expression the kernel had before
// the pair forms.  As an inlined constexpr function the same sum changed the scalar address arithmetic, and with it the instruction
// streams, of the six forms built before (tried twice).
#define OBTG_KO_LDS_WAVE_DOUBLES(DIM, K, pitch, MV, EU, PR)                                                                          \
    (kKoStack * pitch + kKoMaxFaces * (DIM + 1) + (MV ? 2 * DIM * K : 0) + (EU ? kKoMaxFeatures * kKoFeatRec : 0) + (PR ? DIM * K : 0))
inline size_t ko_lds_bytes(int dim, int K, bool moving, bool euclid, bool pair)       // a launch's dynamic LDS
{
    const int pitch = dim * K + 3;
    return sizeof(double) * kKoWaves * (size_t)OBTG_KO_LDS_WAVE_DOUBLES(dim, K, pitch, moving, euclid, pair);
}
__device__ __forceinline__ double ko_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// Coefficient of g_f at the control point p: a . p - b for the face h = (a[0 .. DIM-1], b), summed in coordinate order --
// fma(a[0], p[0], -b), then fma(a[c], p[c], .): operand for operand the negation of keep_in_coeff (bern_device.h), so the
// bits are its bits with the sign flipped.
template <int DIM>
__device__ __forceinline__ double keep_out_coeff(const double* __restrict__ h, const double (&p)[DIM])
{
    double g = __builtin_fma(h[0], p[0], -h[DIM]);
#pragma unroll
    for (int c = 1; c < DIM; ++c) g = __builtin_fma(h[c], p[c], g);
    return g;
}

// Slope of g_f along the direction d (the curve's derivative): a . d, in coordinate order.
template <int DIM>
__device__ __forceinline__ double keep_out_slope(const double* __restrict__ h, const double (&d)[DIM])
{
    double s = h[0] * d[0];
#pragma unroll
    for (int c = 1; c < DIM; ++c) s = __builtin_fma(h[c], d[c], s);
    return s;
}

// Which faces carry the envelope block at the minimiser t* (0 < t* < 1), from every face's value g[f] and slope dg[f] there
// (pt = c(t*), dir = c'(t*)).  f1 = argmax g (the first of equals).  The co-activity rule: a face f != f1 is co-active iff
//     dg[f] and dg[f1] have opposite signs   and   g[f1] - g[f] <= 2 tol (1 + |dg[f]| / |dg[f1]|);
// among several the one with the largest g[f] (the first of equals) is f2.  dg[f1] == 0: a smooth minimum, no f2.  The bound
// is what G(t*) - min G <= tol leaves: the dyadic t* may sit tol / |slope| from the kink where the two faces cross.
//     lam1 = dg[f2] / (dg[f2] - dg[f1]),  lam2 = 1 - lam1          (both in [0, 1]; lam1 = 1 and f2 = -1 without a second face)
struct KoActive {
    int f1, f2;
    double lam1;
};
template <int DIM>
__device__ __forceinline__ KoActive keep_out_active(const double* __restrict__ hf, const int F, const double (&pt)[DIM],
                                                    const double (&dir)[DIM], const double tol, const bool interior)
{
    KoActive a;
    a.f1 = 0; a.f2 = -1; a.lam1 = 1.0;
    double g1 = keep_out_coeff<DIM>(hf, pt);
    for (int f = 1; f < F; ++f) {
        const double g = keep_out_coeff<DIM>(hf + f * (DIM + 1), pt);
        if (g > g1) { g1 = g; a.f1 = f; }
    }
    const double s1 = keep_out_slope<DIM>(hf + a.f1 * (DIM + 1), dir);
    if (!interior || s1 == 0.0) return a;
    double g2 = -INFINITY, s2 = 0.0;
    for (int f = 0; f < F; ++f) {
        if (f == a.f1) continue;
        const double* h = hf + f * (DIM + 1);
        const double g = keep_out_coeff<DIM>(h, pt), s = keep_out_slope<DIM>(h, dir);
        const bool opposite = (s > 0.0 && s1 < 0.0) || (s < 0.0 && s1 > 0.0);
        if (opposite && g1 - g <= 2.0 * tol * (1.0 + fabs(s) / fabs(s1)) && g > g2) { g2 = g; s2 = s; a.f2 = f; }
    }
    if (a.f2 >= 0) a.lam1 = s2 / (s2 - s1);
    return a;
}

// ---- the Euclidean metric (obtg_keep_out_euclid_*; include/obtg.h "Euclidean keep-out clearance")
// The faces are the NORMALISED ones (csrc/keepout_features.h), and the obstacle's features come with them: per feature a record
// of kKoFeatRec doubles, Gram^-1 (a pair's 00, 01, 11, 0, 0, 0; a triple's 00, 01, 02, 11, 12, 22) and the feature's faces packed
// a byte each into the low bytes of the seventh slot (0xff: no third face).  The signed distance at a point p with
// g_f = a^_f . p - b^_f (keep_out_coeff):
//     max_f g_f <= 0:  D = max_f g_f                                   (inside: minus the depth; the callers never come here)
//     otherwise        D = the largest candidate: a face's g_f, or a feature's sqrt(g_S . mu) with mu = Gram_S^-1 g_S all >= 0.
// Every candidate (S, lambda = mu / value) is dual feasible, so every candidate is a lower bound of the distance and the largest
// is the distance; with u = sum lambda_k a^_k and beta = sum lambda_k b^_k, D(q) >= u . q - beta for EVERY q.
// (kKoMaxFeatures, features per obstacle: keepout_features.h; the host refuses more.  kKoFeatRec: above, with the LDS layout)

// The value of feature `rec` at p, or -INFINITY when a multiplier is negative (or the quadratic form is not positive); mu out.
//   pair:    mu0 = fma(i01, g1, i00 g0), mu1 = fma(i11, g1, i01 g0);  q = fma(g1, mu1, g0 mu0)
//   triple:  mu0 = fma(i02, g2, fma(i01, g1, i00 g0)), mu1 = fma(i12, g2, fma(i11, g1, i01 g0)), mu2 = fma(i22, g2, fma(i12, g1, i02 g0));
//            q = fma(g2, mu2, fma(g1, mu1, g0 mu0))
//   value = sqrt(q)
template <int DIM>
__device__ __forceinline__ double ko_feature_value(const double* __restrict__ hf, const double* __restrict__ rec, const double (&p)[DIM],
                                                   double (&mu)[3], int (&fc)[3])
{
    const long long pk = __double_as_longlong(rec[6]);
    fc[0] = (int)(pk & (kKoMaxFaces - 1)); fc[1] = (int)((pk >> 8) & (kKoMaxFaces - 1)); fc[2] = (int)((pk >> 16) & 0xff);
    if (fc[2] != 0xff) fc[2] &= kKoMaxFaces - 1;        // (a face index stays inside the wave's face area whatever the record holds)
    const double g0 = keep_out_coeff<DIM>(hf + fc[0] * (DIM + 1), p), g1 = keep_out_coeff<DIM>(hf + fc[1] * (DIM + 1), p);
    double q;
    if (fc[2] == 0xff) {
        fc[2] = -1;
        mu[0] = __builtin_fma(rec[1], g1, rec[0] * g0);
        mu[1] = __builtin_fma(rec[2], g1, rec[1] * g0);
        mu[2] = 0.0;
        q = __builtin_fma(g1, mu[1], g0 * mu[0]);
    } else {
        const double g2 = keep_out_coeff<DIM>(hf + fc[2] * (DIM + 1), p);
        mu[0] = __builtin_fma(rec[2], g2, __builtin_fma(rec[1], g1, rec[0] * g0));
        mu[1] = __builtin_fma(rec[4], g2, __builtin_fma(rec[3], g1, rec[1] * g0));
        mu[2] = __builtin_fma(rec[5], g2, __builtin_fma(rec[4], g1, rec[2] * g0));
        q = __builtin_fma(g2, mu[2], __builtin_fma(g1, mu[1], g0 * mu[0]));
    }
    if (!(mu[0] >= 0.0 && mu[1] >= 0.0 && mu[2] >= 0.0 && q > 0.0)) return -INFINITY;
    return sqrt(q);
}

// The maximiser at p (every argument but `lane` wave-uniform; call only where max_f g_f(p) > 0).  Candidates in this order:
// the faces 0 .. F - 1, then the features 0 .. nf - 1 in table order; lane l looks at face l and at features l and l + 64, and
// the wave's largest wins, the FIRST of equals in that order.  Every lane then forms the winner's dual pair again from LDS (the
// same instructions in every lane, so the same bits):
//     a face:     ub = (a^_f, b^_f), v = g_f
//     a feature:  lambda_k = mu_k / v;  ub[c] = lambda_0 a^_0[c], then fma(lambda_k, a^_k[c], .), c = DIM the same on b^.
// fc: the winner's faces (-1 padded), obstacle-local.
template <int DIM>
struct KoDual {
    double v;
    double ub[DIM + 1];
    int fc[3];
};
template <int DIM>
__device__ __forceinline__ KoDual<DIM> keep_out_euclid_point(const double* __restrict__ hf, const int F, const double* __restrict__ ft,
                                                             const int nf, const double (&p)[DIM], const int lane)
{
    double mu[3];
    int fc[3];
    double bv = -INFINITY;
    int bc = 0x7fffffff;
    if (lane < F) { bv = keep_out_coeff<DIM>(hf + lane * (DIM + 1), p); bc = lane; }
    for (int j = lane; j < nf; j += kWave) {
        const double v = ko_feature_value<DIM>(hf, ft + j * kKoFeatRec, p, mu, fc);
        if (v > bv) { bv = v; bc = F + j; }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oc = __shfl_xor(bc, o);
        if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
    }
    bc = __builtin_amdgcn_readfirstlane(bc);
    if (bc >= F + nf) bc = 0;                  // (never with finite input: lane 0 always holds face 0 or better)
    KoDual<DIM> r;
    if (bc < F) {
        const double* h = hf + bc * (DIM + 1);
#pragma unroll
        for (int c = 0; c <= DIM; ++c) r.ub[c] = h[c];
        r.v = keep_out_coeff<DIM>(h, p);
        r.fc[0] = bc; r.fc[1] = -1; r.fc[2] = -1;
    } else {
        r.v = ko_feature_value<DIM>(hf, ft + (bc - F) * kKoFeatRec, p, mu, r.fc);
        const double l0 = mu[0] / r.v, l1 = mu[1] / r.v, l2 = mu[2] / r.v;
        const double *h0 = hf + r.fc[0] * (DIM + 1), *h1 = hf + r.fc[1] * (DIM + 1);
#pragma unroll
        for (int c = 0; c <= DIM; ++c) r.ub[c] = __builtin_fma(l1, h1[c], l0 * h0[c]);
        if (r.fc[2] >= 0) {
            const double* h2 = hf + r.fc[2] * (DIM + 1);
#pragma unroll
            for (int c = 0; c <= DIM; ++c) r.ub[c] = __builtin_fma(l2, h2[c], r.ub[c]);
        }
    }
    return r;
}

// A moving obstacle's offset on the vehicle's parameter, E(s) = q(s r) with r = tf / T_o, at the vehicle's degree: lane i
// returns E_i for i < K and 0 above (include/obtg.h "moving keep-out obstacles" fixes this arithmetic).  q: the Km = m + 1
// control points of one coordinate of the motion, 1 <= Km <= K; every argument but `lane` is wave-uniform.
//   restriction to [0, r]: de Casteljau at r, each level b = fma(r, up, (1 - r) b) with 1 - r rounded once; point j of the
//       left piece is lane 0's value after level j.  r == 1: fma(1, up, 0 b) = up, the identity.  r > 1: the polynomial's
//       continuation, the same instructions;
//   elevation: K - Km single-degree steps, degree k -> k + 1: E_i = fma(w, E_(i-1), (1 - w) E_i), w = (double)i / (k + 1);
//       w = 0 at i = 0 and w = 1 at i = k + 1 (lane k + 1 holds 0 before the step), so the ends are exact.
__device__ __forceinline__ double keep_out_motion_points(const double* __restrict__ q, const int Km, const int K, const double r,
                                                         const int lane)
{
    double b = lane < Km ? q[lane] : 0.0, l = b;
    const double omr = 1.0 - r;
    for (int lv = 1; lv < Km; ++lv) {
        const double up = wave_next_lane(b);
        if (lane <= Km - 1 - lv) b = __builtin_fma(r, up, omr * b);
        const double first = ko_lane(b, 0);
        if (lane == lv) l = first;
    }
    for (int k = Km - 1; k < K - 1; ++k) {
        const double prev = __shfl_up(l, 1);
        const double w = (double)lane / (double)(k + 1);
        if (lane <= k + 1) l = __builtin_fma(w, prev, (1.0 - w) * l);
    }
    return l;
}

// One level of the de Casteljau recurrence on the Bernstein basis held a lane per index (lane i: B_i), the arithmetic of
// envelope_block / keep_in_envelope_block (bern_device.h):  w[i] = fma(t, w[i-1], s w[i]) for i >= 1,  w[0] = s w[0].
// prev: lane i - 1's value (anything in lane 0).
__device__ __forceinline__ double keep_out_basis_level(const int lane, const double w, const double prev, const double t, const double s)
{
    return lane == 0 ? s * w : __builtin_fma(t, prev, s * w);
}

}  // namespace obtg
