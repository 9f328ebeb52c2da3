// The grid of the planar hull-pair sweeps (gjk_kernels.hip k_gjk_swarm_planar, k_pair_sweep, k_pair_sweep_tiled) as pure
// integer arithmetic: a row's dynamic LDS, how many workgroups a row gets, how many passes a workgroup makes over one
// staging, how many hull pairs a pass holds -- and the index rule by which a workgroup finds its pairs.  Every hull pair is
// evaluated exactly once only if the host's split and the kernel's rule agree, and the split depends on the card's CU count,
// so it lives in one place that needs no GPU to check: plain C++17, no HIP header, no allocation, no global state
// (tests/test_sweep_shape.py compiles it for the host and walks every workgroup of the bench shapes, of the toy shapes of
// tests/test_gpu_sweep_shapes.py and of a grid of sizes, at the CU counts a partitioned card reports).
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <limits.h>
#include <algorithm>

#if defined(__HIPCC__)
#define OBTG_SS_HD __host__ __device__
#else
#define OBTG_SS_HD
#endif

namespace obtg {

// MODE 0: the sweep of rows that fit LDS; MODE 1: the finite-difference de-duplication pass; MODE 2: tiled (large rows)
template <int MODE>
OBTG_SS_HD constexpr size_t planar_lds_bytes(int cap_obj, int vpq, int chunk)
{
    // objects | rec int2[chunk], plist u32[chunk] | ext int[2 cap_obj] | MODE 1: list int[chunk]; MODE 0, 2: ord u16[chunk]
    // (14 bytes per pair for the sweeps: five workgroups of 1264 pairs and 72 objects per CU)
    return 16 * (size_t)cap_obj * vpq + 12 * (size_t)chunk + 8 * (size_t)cap_obj + (MODE == 1 ? 4 : 2) * (size_t)chunk;
}

// a workgroup's dynamic LDS when per_cu of them share a CU's 160 KB (1040 bytes of static LDS per workgroup, rounded up)
constexpr size_t lds_share(int per_cu) { return (size_t)160 * 1024 / per_cu - 1280; }
constexpr size_t kLdsDefaultMax = 48 * 1024;      // what a launch may ask for without raising the kernel's limit
constexpr size_t kLdsLaunchMax = 64 * 1024;       // ... and with it, for the sweeps

// The switches that force a shape (A/B runs and tests/test_gpu_sweep_shapes.py); kSweepUnset: the variable is not set.
constexpr int kSweepUnset = INT_MIN;
struct SweepKnobs {
    int wgs = kSweepUnset;             // OBTG_SWEEP_WGS: workgroups per row (at least 1)
    int passes = kSweepUnset;          // OBTG_SWEEP_PASSES: passes per workgroup (at least 1; more where a pass would not fit LDS)
    int tile_a = kSweepUnset;          // OBTG_TILE_A: the tiled forms' tile height, 4 .. 32
};

// The one place that reads them.  Per launch, not once: A/B runs and the tests change them between calls.  The tile
// height goes into a context's chunk tables, which are cached until its pair list or polygons change: only their builder
// asks for it (tile_too), a launch reads the two switches of its grid and no more.
inline SweepKnobs sweep_knobs_from_env(bool tile_too = true)
{
    SweepKnobs k;
    if (const char* e = getenv("OBTG_SWEEP_WGS")) k.wgs = atoi(e);
    if (const char* e = getenv("OBTG_SWEEP_PASSES")) k.passes = atoi(e);
    if (tile_too) if (const char* e = getenv("OBTG_TILE_A")) k.tile_a = atoi(e);
    return k;
}

// Tiles are TA x 64 blocks of the pair matrix.  A workgroup's lanes refill from its tile only, so the taller the tile
// the fewer lanes idle at its end -- as long as the four workgroups a CU can hold (register bound of the tiled
// kernels) still fit its 160 KB of LDS.  C4 (16 points): TA = 8 / 12 / 13 / 14 -> 17.96 / 14.25 / 13.80 /
// 16.11 ms per sweep (14 costs a workgroup per CU).
inline int tile_height(int nc, const SweepKnobs& knobs)
{
    const int vpq = nc | 1, occ = 4;
    const size_t budget = lds_share(occ);
    int ta = 8;
    while (ta < 32 && planar_lds_bytes<2>(ta + 1 + 64, vpq, (ta + 1) * 64) <= budget) ++ta;
    if (knobs.tile_a != kSweepUnset) ta = std::max(4, std::min(32, knobs.tile_a));     // (experiments)
    return ta;
}

struct SweepShape {
    int wgs = 1, passes = 1, chunk = 0, per_cu = 1;
    size_t lds = 0;
};

// n_hull_pairs: the row's hull pairs; n_obj: the objects a workgroup stages (vehicles + polygons + point obstacles, which
// the pair sweep stages too); nc: points per hull; n_cus: compute units of the device; waves_per_simd: workgroups per CU
// that the kernel's registers allow; chunk_target: hull pairs per workgroup of a large batch.
inline SweepShape sweep_shape(int n_hull_pairs, int n_obj, int nc, int n_cus, int B, int waves_per_simd, int chunk_target,
                              const SweepKnobs& knobs)
{
    const int np = n_hull_pairs, vpq = nc | 1;
    const size_t fixed = planar_lds_bytes<0>(n_obj, vpq, 0);
    SweepShape sh;
    // workgroups per CU: what the kernel's registers allow, fewer while the row's objects leave no room for 256 pairs
    int per_cu = nc <= 11 ? waves_per_simd : 1;
    size_t budget = 0;
    for (; per_cu >= 1; --per_cu) {
        budget = lds_share(per_cu);
        if (per_cu == 1) budget = kLdsLaunchMax;                   // one workgroup per CU: the launch limit
        if (fixed + 14 * 256 <= budget) break;
    }
    if (per_cu < 1) per_cu = 1;
    const int chunk_max = fixed + 14 * 256 <= budget ? (int)std::min<size_t>((budget - fixed) / 14, 65535) : 256;
    int W = std::max(1, (np + chunk_target - 1) / chunk_target);
    // Small batches (a rank's share of a row-sharded iteration, bench.py --mode rows): as many workgroups per row as ONE
    // round of resident workgroups has room for beside the row's dynamics group -- a second round costs a whole
    // workgroup's latency again (B = 145 at C3: 6 per row 0.040 ms, 8 per row 0.052, the old rule's 16 per row 0.068;
    // B = 289: 3 per row 0.061, 8 per row 0.080) -- and three per row while the launch is two or three rounds
    // (B = 577: 0.104 against 0.109 / 0.116 for 4 / 2); tools/r04_small_batch_scan.sh, profiles/r04_experiments/.
    {
        const long slots = (long)per_cu * std::max(1, n_cus);
        if ((long)B * (W + 1) < slots) {
            const int fill = (int)((slots - B + B / 2) / std::max(1, B));         // round((slots - B) / B)
            W = std::max(W, std::min(fill, std::max(1, np / 128)));
        } else if ((long)B * (W + 1) < 3 * slots) W = std::max(W, std::min(3, std::max(1, np / 128)));
    }
    while ((np + W - 1) / W > chunk_max && (np + W - 1) / W > 256) ++W;           // the row's objects leave less LDS
    int Q = 1;
    if (knobs.wgs != kSweepUnset) W = std::max(1, knobs.wgs);
    if (knobs.passes != kSweepUnset) Q = std::max(1, knobs.passes);
    const int per_wg = (np + W - 1) / W;
    while ((per_wg + Q - 1) / Q > chunk_max && (per_wg + Q - 1) / Q > 64) ++Q;   // (a forced shape may need passes to fit)
    sh.passes = Q;
    sh.chunk = (per_wg + Q - 1) / Q;
    sh.wgs = (np + sh.passes * sh.chunk - 1) / (sh.passes * sh.chunk);
    sh.per_cu = per_cu;
    sh.lds = planar_lds_bytes<0>(n_obj, vpq, sh.chunk);
    return sh;
}

// Host mirror of the kernels' index rule (MODE 0, the pass loop of k_gjk_swarm_planar): workgroup w of a row takes, in its
// pass q (seg0 = q * chunk), the pairs [cbase, cbase + n) with cbase = w * passes * chunk + seg0 and
// n = clamp(n_pairs - cbase, 0, chunk).  A change there is a change here.
struct SweepPass { int cbase, n; };
inline SweepPass sweep_pass(int n_pairs, int passes, int chunk, int w, int q)
{
    const int cbase = w * passes * chunk + q * chunk;
    const int left = n_pairs - cbase;
    return SweepPass{ cbase, left < 0 ? 0 : (left < chunk ? left : chunk) };
}

}  // namespace obtg
