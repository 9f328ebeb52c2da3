// Device functions shared by the branch-and-bound searches on Bezier curves: the _minDist family (gjk_kernels.hip) and the
// collision checks (coll_kernels.hip).  Both units are compiled with -ffp-contract=off: the expressions below are the
// reference's, operation for operation (bezier.py:985-1027 deCasteljauSplit, bezier.py:1544-1558 norm).
#pragma once
#include <hip/hip_runtime.h>

#include "obtg_internal.h"

namespace obtg {

constexpr int kMdQuadMaxK = 16;      // control points per curve of the forms that give a child a 16-lane row of the wavefront

__device__ __forceinline__ double norm_seq(double ax, double ay, double az, double bx, double by, double bz)
{
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    double s = 0.0;
    s += dx * dx; s += dy * dy; s += dz * dz;
    return __builtin_sqrt(s);
}

// numpy's argmin over n distances: the smallest, the first of equals -- and the first NaN wins
template <int N>
__device__ __forceinline__ int np_argmin(const double (&dd)[N])
{
    int am = 0;
    for (int i = 1; i < N; ++i) if (dd[i] < dd[am]) am = i;
    for (int i = 0; i < N; ++i) if (dd[i] != dd[i]) { am = i; break; }
    return am;
}

// _upperbound (bezier.py:1499-1516): the smallest of the four end-point distances of c1[3][KA] and c2[3][KB]; am: which one
// (bit 1: curve 1's last point, bit 0: curve 2's).  PLANAR: every z is +0, and norm_seq with dz = 0 is s + 0 * 0 = s.
template <bool PLANAR>
__device__ __forceinline__ double md_upper_bound(const double* c1, int KA, const double* c2, int KB, int& am)
{
    double dd[4];
    if constexpr (PLANAR) {
        auto n2 = [](double ax, double ay, double bx, double by) {
            const double dx = ax - bx, dy = ay - by;
            double s = 0.0;
            s += dx * dx; s += dy * dy;
            return __builtin_sqrt(s);
        };
        dd[0] = n2(c1[0], c1[KA], c2[0], c2[KB]);
        dd[1] = n2(c1[0], c1[KA], c2[KB - 1], c2[2 * KB - 1]);
        dd[2] = n2(c1[KA - 1], c1[2 * KA - 1], c2[0], c2[KB]);
        dd[3] = n2(c1[KA - 1], c1[2 * KA - 1], c2[KB - 1], c2[2 * KB - 1]);
    } else {
        dd[0] = norm_seq(c1[0], c1[KA], c1[2 * KA], c2[0], c2[KB], c2[2 * KB]);
        dd[1] = norm_seq(c1[0], c1[KA], c1[2 * KA], c2[KB - 1], c2[2 * KB - 1], c2[3 * KB - 1]);
        dd[2] = norm_seq(c1[KA - 1], c1[2 * KA - 1], c1[3 * KA - 1], c2[0], c2[KB], c2[2 * KB]);
        dd[3] = norm_seq(c1[KA - 1], c1[2 * KA - 1], c1[3 * KA - 1], c2[KB - 1], c2[2 * KB - 1], c2[3 * KB - 1]);
    }
    am = np_argmin(dd);
    return dd[am];
}

// _upperboundPoly (bezier.py:1535-1547): the nearer end point of c[3][K] to the polygon's closest point; am: 1 = the last point
__device__ __forceinline__ double md_upper_bound_poly(const double* c, int K, double cx, double cy, double cz, int& am)
{
    const double dd[2] = { norm_seq(c[0], c[K], c[2 * K], cx, cy, cz), norm_seq(c[K - 1], c[2 * K - 1], c[3 * K - 1], cx, cy, cz) };
    am = np_argmin(dd);
    return dd[am];
}

// The lane above's value (lane 63: zero): one DPP move per half of the double, no LDS round trip.
__device__ __forceinline__ double wave_next_lane(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// deCasteljauSplit of rows [row0, row0 + nrows) of a node's six coordinate rows (rows 0..2: curve 1 at t1, rows 3..5:
// curve 2 at t2), BOTH pieces kept: as split_rows3_wave_t, where the left piece's point L is lane (r, 0)'s value at level L
// and the right piece's point i is lane (r, i)'s value at level K - 1 - i -- never the same lane at the same level before
// the last one, so a level is still one store per lane.
template <int KC>
__device__ __forceinline__ void split_both_t(const double* c1, const double* c2, int K, double t1, double t2, double* blob,
                                             int row0, int nrows, double* dump)
{
    if (KC > 0) K = KC;
    const int lane = threadIdx.x & 63;
    const int rq = lane / K, il = lane - rq * K, row = row0 + rq;
    const bool valid = rq < nrows;
    const bool second = row >= 3;
    const int r3 = second ? row - 3 : row;
    double w = valid ? (second ? c2 : c1)[r3 * K + il] : 0.0;
    const double t = second ? t2 : t1, u = 1 - t;
    double* outL = blob + (second ? 6 * K : 0) + r3 * K;          // left piece's row; the right piece's is 3 K further
    double* outR = outL + 3 * K + il;
    const bool first = valid && il == 0;
    const int my_level = valid ? K - 1 - il : -1;
    double* mine = dump + lane;
    auto level = [&](int L) {
        double* a = first ? outL + L : (my_level == L ? outR : mine);
        *a = w;
        const double up = wave_next_lane(w);
        w = u * w + t * up;
    };
    if constexpr (KC > 0) {
#pragma unroll
        for (int L = 0; L < KC - 1; ++L) level(L);
    } else {
        for (int L = 0; L < K - 1; ++L) level(L);
    }
    // the last level's value: point K - 1 of the left piece and point 0 of the right one
    double* a = first ? outL + (K - 1) : mine;
    double* b = first ? outR : mine;
    *a = w; *b = w;
}

}  // namespace obtg
