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
