// Host geometry of the Euclidean keep-out rows (include/obtg.h "Euclidean keep-out clearance"): the
// normalised faces of one convex obstacle {p : a_f . p <= b_f} and the table of its FEATURES -- the corners of a polygon, the
// edges and vertices of a polyhedron -- with the inverse Gram matrix of each.  Plain C++: no HIP, no project header, so that a
// host compiler alone builds it (tests/native/keepout_features_host.cpp; exported as obtg_keep_out_features).
//
// Arithmetic, in this order (plain double operations, no contraction is relied on: every product below stands alone or is
// written as std::fma):
//   normalisation   s = a[0] a[0], then s = fma(a[c], a[c], s); n = sqrt(s); a^[c] = a[c] / n, b^ = b / n.  |a| = 1 gives n = 1
//                   and the face is left bit for bit; |a| = 0 or a non-finite entry gives a NaN normal (the device's NaN rule).
//   Gram entries    G_kl = a^_k . a^_l, summed in coordinate order as fma(a^_k[c], a^_l[c], .), the diagonal too.
//   pair (i < j)    det = G_ii G_jj - G_ij G_ij;  non-parallel iff det > kKoFeatDetMin;
//                   Gram^-1 = (G_jj / det, -G_ij / det, G_ii / det)                      entries (00, 01, 11)
//   triple          the symmetric cofactors C_00 = G_jj G_kk - G_jk G_jk, C_01 = G_ik G_jk - G_ij G_kk, C_02 = G_ij G_jk - G_ik G_jj,
//                   C_11 = G_ii G_kk - G_ik G_ik, C_12 = G_ij G_ik - G_ii G_jk, C_22 = G_ii G_jj - G_ij G_ij,
//                   det = fma(G_ik, C_02, fma(G_ij, C_01, G_ii C_00)); non-singular iff det > kKoFeatDetMin;
//                   Gram^-1 = C / det                                                    entries (00, 01, 02, 11, 12, 22)
//   the point       p = A^T (Gram^-1 b^): the intersection of a 2-D pair or a 3-D triple, the point of a 3-D pair's common
//                   line nearest the origin.
//   face test       face m (not of the set) admits p iff a^_m . p - b^_m <= kKoFeatTol (1 + |b^_m|): tolerant, so that a
//                   feature is included rather than left out (a feature left out can only make a row smaller; a set that is
//                   no feature changes nothing: every candidate is a lower bound of the distance).
//   3-D edge        the line p + t v, v = a^_i x a^_j, clipped by every other face m: with s = a^_m . v and
//                   r = kKoFeatTol (1 + |b^_m|) - (a^_m . p - b^_m):  |s| <= kKoFeatDetMin: empty iff r < 0;  s > 0: t <= r / s;
//                   s < 0: t >= r / s.  The pair is an edge iff the interval is not empty (a single point counts).  This, not
//                   "shares a vertex", finds the edge of an unbounded wedge.
// Table order: every pair (i, j), i < j, in lexicographic order, then (d = 3) every triple (i, j, k), i < j < k, in
// lexicographic order.  More than kKoMaxFeatures features: the count is still returned, nothing is stored beyond the room.
#pragma once
#include <cmath>

namespace obtg {

constexpr int kKoFeatMaxFaces = 16;          // faces per obstacle
constexpr int kKoMaxFeatures = 128;          // features per obstacle (above: OBTG_ERR_UNSUPPORTED from the Euclidean calls)
constexpr double kKoFeatTol = 1e-9;          // the face test's tolerance, times (1 + |b^|)
constexpr double kKoFeatDetMin = 1e-12;      // a Gram determinant at or below this: parallel faces / a singular triple

// H[F][d + 1] -> Hn[F][d + 1]
inline void keep_out_normalise(const double* H, int F, int d, double* Hn)
{
    for (int f = 0; f < F; ++f) {
        const double* h = H + f * (d + 1);
        double s = h[0] * h[0];
        for (int c = 1; c < d; ++c) s = std::fma(h[c], h[c], s);
        const double n = std::sqrt(s);
        for (int c = 0; c <= d; ++c) Hn[f * (d + 1) + c] = h[c] / n;
    }
}

namespace ko_feat {
inline double dot(const double* a, const double* b, int d)
{
    double s = a[0] * b[0];
    for (int c = 1; c < d; ++c) s = std::fma(a[c], b[c], s);
    return s;
}
inline bool admits(const double* Hn, int F, int d, const double* p, int i, int j, int k)
{
    for (int m = 0; m < F; ++m) {
        if (m == i || m == j || m == k) continue;
        const double* h = Hn + m * (d + 1);
        if (!(dot(h, p, d) - h[d] <= kKoFeatTol * (1.0 + std::fabs(h[d])))) return false;
    }
    return true;
}
}  // namespace ko_feat

// The features of one obstacle from its normalised faces Hn[F][d + 1], d 2 or 3, 1 <= F <= 16.  idx[.][3]: the faces of a
// feature, ascending, -1 padded; ginv[.][6]: a pair's (00, 01, 11, 0, 0, 0), a triple's (00, 01, 02, 11, 12, 22); both with room
// for `room` features.  Returns the number of features found, which may exceed `room`.
inline int keep_out_enumerate(const double* Hn, int F, int d, int room, int* idx, double* ginv)
{
    using namespace ko_feat;
    int n = 0;
    const int w = d + 1;
    for (int i = 0; i < F; ++i)
        for (int j = i + 1; j < F; ++j) {
            const double *hi = Hn + i * w, *hj = Hn + j * w;
            const double gii = dot(hi, hi, d), gij = dot(hi, hj, d), gjj = dot(hj, hj, d);
            const double det = gii * gjj - gij * gij;
            if (!(det > kKoFeatDetMin)) continue;
            const double v00 = gjj / det, v01 = -gij / det, v11 = gii / det;
            const double m0 = std::fma(v01, hj[d], v00 * hi[d]), m1 = std::fma(v11, hj[d], v01 * hi[d]);
            double p[3] = {0.0, 0.0, 0.0};
            for (int c = 0; c < d; ++c) p[c] = std::fma(m1, hj[c], m0 * hi[c]);
            bool is_feature;
            if (d == 2) is_feature = admits(Hn, F, d, p, i, j, -1);
            else {
                const double v[3] = {hi[1] * hj[2] - hi[2] * hj[1], hi[2] * hj[0] - hi[0] * hj[2], hi[0] * hj[1] - hi[1] * hj[0]};
                double lo = -INFINITY, hi_t = INFINITY;
                is_feature = true;
                for (int m = 0; m < F && is_feature; ++m) {
                    if (m == i || m == j) continue;
                    const double* h = Hn + m * w;
                    const double s = dot(h, v, d), r = kKoFeatTol * (1.0 + std::fabs(h[d])) - (dot(h, p, d) - h[d]);
                    if (std::fabs(s) <= kKoFeatDetMin) { if (!(r >= 0.0)) is_feature = false; }
                    else if (s > 0.0) hi_t = std::fmin(hi_t, r / s);
                    else lo = std::fmax(lo, r / s);
                }
                is_feature = is_feature && lo <= hi_t;
            }
            if (!is_feature) continue;
            if (n < room) {
                idx[3 * n] = i; idx[3 * n + 1] = j; idx[3 * n + 2] = -1;
                double* g = ginv + 6 * n;
                g[0] = v00; g[1] = v01; g[2] = v11; g[3] = g[4] = g[5] = 0.0;
            }
            ++n;
        }
    if (d != 3) return n;
    for (int i = 0; i < F; ++i)
        for (int j = i + 1; j < F; ++j)
            for (int k = j + 1; k < F; ++k) {
                const double *hi = Hn + i * w, *hj = Hn + j * w, *hk = Hn + k * w;
                const double gii = dot(hi, hi, d), gij = dot(hi, hj, d), gik = dot(hi, hk, d), gjj = dot(hj, hj, d), gjk = dot(hj, hk, d),
                             gkk = dot(hk, hk, d);
                const double c00 = gjj * gkk - gjk * gjk, c01 = gik * gjk - gij * gkk, c02 = gij * gjk - gik * gjj,
                             c11 = gii * gkk - gik * gik, c12 = gij * gik - gii * gjk, c22 = gii * gjj - gij * gij;
                const double det = std::fma(gik, c02, std::fma(gij, c01, gii * c00));
                if (!(det > kKoFeatDetMin)) continue;
                const double v[6] = {c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det};
                const double bi = hi[d], bj = hj[d], bk = hk[d];
                const double m0 = std::fma(v[2], bk, std::fma(v[1], bj, v[0] * bi)), m1 = std::fma(v[4], bk, std::fma(v[3], bj, v[1] * bi)),
                             m2 = std::fma(v[5], bk, std::fma(v[4], bj, v[2] * bi));
                double p[3];
                for (int c = 0; c < d; ++c) p[c] = std::fma(m2, hk[c], std::fma(m1, hj[c], m0 * hi[c]));
                if (!admits(Hn, F, d, p, i, j, k)) continue;
                if (n < room) {
                    idx[3 * n] = i; idx[3 * n + 1] = j; idx[3 * n + 2] = k;
                    for (int e = 0; e < 6; ++e) ginv[6 * n + e] = v[e];
                }
                ++n;
            }
    return n;
}

}  // namespace obtg
