/*
 * obtg.h -- C ABI of libobtg_hip.so: MI355X (gfx950) evaluation of the constraint /
 * cost hot path that SciPy SLSQP calls on every iteration of the reference
 * (caslabuiowa/OptimalBezierTrajectoryGeneration).
 *
 * The reference has no FFI layer (it is pure Python); the seam this ABI replaces is
 * the set of Python callables SLSQP invokes.  Each entry point names the reference
 * function(s) it stands in for (paths relative to the reference checkout).  The
 * Python look-alikes in optimalbeziertrajectorygeneration_amd/ bind these symbols
 * with ctypes; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - plain C symbols, POD arguments, no exceptions, no global state outside the ctx;
 *   - all floating point is IEEE binary64; all index / flag arrays are int32 (traces int16);
 *   - return value: 0 = OBTG_OK, negative = argument / device error (obtg_strerror).
 *     Per-item algorithmic outcomes (collision, iteration caps) go to flag/status
 *     arrays, never to the return code;
 *   - "host" entry points take caller-allocated HOST buffers, block until the result
 *     is in `out`, and leave the device idle.  "_dev" entry points take DEVICE
 *     pointers, enqueue on the context's stream and return immediately
 *     (obtg_sync() or the caller's own stream sync completes them);
 *   - a context is used by one thread at a time (SLSQP is serial); distinct contexts
 *     are independent.  There is NO CPU fallback: obtg_ctx_create fails when no
 *     gfx950 device is usable.
 *
 * Shapes: N = n_veh vehicles, d = dim, n = deg (n+1 control points), R = deg_elev,
 * M = n_point_obs.  One "evaluation row" of control points is
 *     Y[(N*d)][(n+1)]  row-major float64  (the `y` of reshapeVector, optimization.py:242-285)
 * and batched calls take B such rows back to back (B = n_x+1 for one SLSQP Jacobian).
 */
#ifndef OBTG_H
#define OBTG_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct obtg_ctx obtg_ctx;

enum {
    OBTG_OK = 0,
    OBTG_ERR_ARG = -1,        /* bad argument (null pointer, negative size, unsupported dim ...) */
    OBTG_ERR_DEVICE = -2,     /* HIP runtime error (see obtg_last_error) */
    OBTG_ERR_NO_DEVICE = -3,  /* no usable gfx950 device */
    OBTG_ERR_OOM = -4,        /* device or host allocation failed */
    OBTG_ERR_UNSUPPORTED = -5 /* degree / size outside what the kernels support */
};

/* per-item GJK status (status[] arrays) */
enum {
    OBTG_ST_OK = 0,
    OBTG_ST_MD_CAP = 1,  /* minimumDistance's `while True` (gjk/gjk.py:277) exceeded md_cap rounds */
    OBTG_ST_MAXITER = 2, /* gjkNew exhausted maxIter (flag = -1, gjk/gjk.py:269-270) */
    OBTG_ST_CYCLE = 3    /* minimumDistance returned exactly to an earlier (simplex, direction) state: the
                          * reference's loop depends on nothing else, so it never exits on this input.
                          * Reported by the 3-D state machine (any z != 0) and by the curve-distance entry points
                          * (obtg_min_dist, obtg_min_dist2poly: inner calls, seen as OBTG_MD_GJK_CAP; since round 6 their
                          * planar calls carry the checkpoint too); the planar hull SWEEPS are guarded by md_cap alone. */
};

/* per-item minDist status */
enum {
    OBTG_MD_OK = 0,
    OBTG_MD_NODE_CAP = 1,  /* node budget exhausted (reference: runs for seconds / forever) */
    OBTG_MD_DEPTH_CAP = 2, /* deeper than max_depth (reference: RecursionError / cnt > 1000, bezier.py:1310) */
    OBTG_MD_GJK_CAP = 3    /* an inner gjkNew never returns: a proven cycle of its minimumDistance loop, or md_cap rounds */
};

const char* obtg_strerror(int code);

/* ABI revision.  Bumped whenever an EXISTING symbol changes meaning (new symbols alone do not bump it), so that a caller
 * bound against an older header can notice at load time.
 *   4  round 4: obtg_ctx_set_stream(ctx, NULL) selects the NULL (legacy default) stream -- the handle is taken as given.
 *      Until then NULL meant "the context's own non-blocking stream"; that meaning moved to obtg_ctx_use_own_stream.
 *      A caller written against revision <= 3 that passes NULL to get the private stream back still links and runs, but
 *      now serialises with the legacy stream: call obtg_ctx_use_own_stream instead.
 *   5  round 5: nothing changed meaning; new: obtg_abi_version, obtg_fast_kernels, obtg_ctx_ang_rate_order_in_effect, obtg_temporal_sep_active[_dev],
 *      obtg_comm_* and obtg_temporal_sep_min_gather_dev (the collective behind the C ABI); 9 control points (degree 8)
 *      joined the specialised counts.
 *   6  round 6: nothing changed meaning; new: obtg_source_hash, obtg_libm_pow_matches.
 *   7  nothing changed meaning; new: the exact derivatives obtg_temporal_sep_jac[_dev], obtg_speed_jac[_dev],
 *      obtg_ang_rate_jac[_dev], obtg_euclidean_grad, obtg_deriv_energy_grad and the kernel-stats id OBTG_K_JAC
 *      (OBTG_K_COUNT moved from 8 to 9).
 *      Later, still 7: new: the collision checks obtg_coll_check, obtg_coll_check2poly (timed under OBTG_K_MIN_DIST).
 *      Later, still 7: new: the true Bernstein extrema obtg_bern_extrema[_dev] (timed under OBTG_K_BERN) and
 *      obtg_temporal_sep_true_min[_dev] (timed under OBTG_K_TEMPORAL_SEP).
 *      Later, still 7: new: obtg_ctx_set_fd_view_structured.  obtg_constraint_sweep_dev with dY = NULL inside a view now
 *      takes the structured step where it applies: the same arrays with the same bits, so no meaning changed.
 *      Later, still 7: new: the envelope Jacobian of the true-minimum rows, obtg_temporal_sep_true_min_jac[_dev] (timed
 *      under OBTG_K_TEMPORAL_SEP).
 *      Later, still 7: new: obtg_min_dist_mixed, `_minDist` on curves of different degree (timed under OBTG_K_MIN_DIST).
 *      Later, still 7: new: the true speed rows obtg_speed_true_min[_dev] and their envelope Jacobian
 *      obtg_speed_true_min_jac[_dev] (timed under OBTG_K_SPEED).
 *      Later, still 7: new: the true angular-rate rows obtg_ang_rate_true_min[_dev], their envelope Jacobian
 *      obtg_ang_rate_true_min_jac[_dev] and the rows' polynomials obtg_ang_rate_poly[_dev] (timed under OBTG_K_ANG_RATE).
 *      Later, still 7: new: the acceleration-bound rows obtg_accel[_dev], their true minima obtg_accel_true_min[_dev] and the
 *      envelope Jacobian obtg_accel_true_min_jac[_dev] (timed under OBTG_K_SPEED).
 *      Later, still 7: new: the jerk-bound rows obtg_jerk[_dev], their true minima obtg_jerk_true_min[_dev] and the envelope
 *      Jacobian obtg_jerk_true_min_jac[_dev] (timed under OBTG_K_SPEED).
 *      Later, still 7: new: the true arc length obtg_bern_arc_length[_dev] and the objective obtg_arc_length_obj[_dev], timed
 *      under a kernel-stats id of their own, OBTG_K_ARC_LENGTH = 9.  OBTG_K_COUNT stays 9, the ids of revision 7 as callers
 *      have sized their arrays by it; OBTG_K_END = 10 is the end of the ids obtg_kernel_stats answers for.
 *      Later, still 7: new: the curvature-bound rows obtg_curvature_true_min[_dev], their envelope Jacobian
 *      obtg_curvature_true_min_jac[_dev], their polynomials obtg_curvature_poly[_dev] and the curvature range of free curves
 *      obtg_bern_curvature[_dev] (timed under OBTG_K_ANG_RATE; no kernel id added).
 *      Later, still 7: new: the space-curvature rows of 3-D vehicles obtg_space_curvature_true_min[_dev], their envelope Jacobian
 *      obtg_space_curvature_true_min_jac[_dev], their polynomials obtg_space_curvature_poly[_dev] and the largest curvature of
 *      free space curves obtg_bern_space_curvature[_dev] (timed under OBTG_K_ANG_RATE; no kernel id added).
 *      Later, still 7: new: the keep-in region obtg_ctx_set_keep_in, its rows obtg_keep_in[_dev] (obtg_len_keep_in), their true
 *      margins obtg_keep_in_true_min[_dev] and the envelope Jacobian obtg_keep_in_true_min_jac[_dev] (timed under OBTG_K_SPEED;
 *      no kernel id added).
 *      Later, still 7: new: the keep-out obstacles obtg_ctx_set_keep_out (obtg_len_keep_out), their true clearances
 *      obtg_keep_out_true_min[_dev], the envelope Jacobian obtg_keep_out_true_min_jac[_dev] and the clearance of free curves
 *      obtg_bern_keep_out[_dev] (timed under OBTG_K_SPEED; no kernel id added).
 *      Later, still 7: new: keep-out obstacles that move along a known path: obtg_ctx_set_keep_out_motion, the clearances
 *      obtg_keep_out_moving_true_min[_dev], the envelope Jacobian with its tf column obtg_keep_out_moving_true_min_jac[_dev] and
 *      free curves against one moving obstacle obtg_bern_keep_out_moving[_dev] (timed under OBTG_K_SPEED; no kernel id added).
 *      Later, still 7: new: the read-only query obtg_sweep_shape (which form and grid the hull-pair sweeps take).
 *      Later, still 7: new: the Euclidean keep-out clearance: the host geometry obtg_keep_out_features, the rows
 *      obtg_keep_out_euclid_true_min[_dev], the envelope Jacobian obtg_keep_out_euclid_true_min_jac[_dev] and free curves
 *      obtg_bern_keep_out_euclid[_dev] (timed under OBTG_K_SPEED; no kernel id added).
 *      Later, still 7: new: polytopic vehicle-to-vehicle separation: the region obtg_ctx_set_pair_keep_out
 *      (obtg_len_pair_keep_out), the rows obtg_pair_keep_out_true_min[_dev] and obtg_pair_keep_out_euclid_true_min[_dev] and
 *      their envelope Jacobians obtg_pair_keep_out_true_min_jac[_dev], obtg_pair_keep_out_euclid_true_min_jac[_dev] (timed
 *      under OBTG_K_SPEED; no kernel id added).
 *      Later, still 7: new: the proximity rows ("come close", "stay close"): the items obtg_ctx_set_proximity
 *      (obtg_len_proximity), their polynomials obtg_proximity_poly[_dev], the certified extrema obtg_proximity_true[_dev] and
 *      the envelope Jacobian obtg_proximity_true_jac[_dev] (timed under OBTG_K_TEMPORAL_SEP; no kernel id added).  New symbols
 *      alone do not move the number: no existing meaning changed. */
#define OBTG_ABI_VERSION 7
int obtg_abi_version(void);

/* Which sources this library was built from: the first 16 hex digits of a sha256 over a compile unit's source, the headers of
 * csrc/ and its compiler flags.  unit: "gjk_kernels", "bern_kernels", "jac_kernels", "coll_kernels", "extrema_kernels", "capi", "tables", "comm", "libm_check", or "all" (NULL =
 * "all"); NULL is returned for a name that is none of these.  Counter files under profiles/ record the hash of the kernels they
 * were taken on; bench.py drops a counter whose hash is not the running library's instead of reporting it as measured. */
const char* obtg_source_hash(const char* unit);

/* 1 when this host's libm rounds pow(x, 2.0) exactly as the device's restatement of it does (csrc/libm_pow2.h: glibc 2.35,
 * the FMA build) on a few thousand inputs, 0 when not.  `a**2` in the reference (gjk/gjk.py:460; optimization.py:343-459 on the
 * bounds) is libm's pow; with 0 the device's closest points / distances can differ from a reference run on THIS host by one
 * ulp (and `_minDist` searches that feed them back can take another path), although they still equal the committed fixtures.
 * Evaluated once per process, no device needed. */
int obtg_libm_pow_matches(void);

/* Which specialised (template-instantiated) kernel families exist for curves of `deg` in `dim` dimensions -- a bit mask:
 *   1  separation / speed rows, one-vs-many, structured separation Jacobian blocks (2-D and 3-D)
 *   2  angular rate at DEG_ELEV = 0, the hull sweeps on deg + 1 points per object, the one-launch steps
 *   4  DEG_ELEV > 0: separation + dynamics in one launch, the elevated structured step
 * 0: every family of that shape runs on the any-degree kernels (one wave per item).  The list itself lives in ONE place,
 * csrc/obtg_internal.h (OBTG_NC_*); callers that pick a code path by degree ask here instead of repeating it. */
int obtg_fast_kernels(int dim, int deg);
/* last HIP error string seen by this context (empty when none) */
const char* obtg_last_error(const obtg_ctx*);
/* number of usable gfx950 devices (0 when none / no HIP runtime) */
int obtg_device_count(void);
/* every exported symbol, NUL-separated list terminated by an empty string (for load tests) */
const char* obtg_abi_symbols(void);

/* Pinned (page-locked) host memory.  The host-buffer entry points accept any host pointer; buffers from
 * obtg_host_alloc are DMA targets as they are (PCIe rate), pageable buffers (e.g. a plain NumPy array) are staged
 * through a pinned ring inside the context, chunk by chunk, overlapped with the transfer. */
int obtg_host_alloc(size_t bytes, void** out);
int obtg_host_free(void* p);

/* ---- context -------------------------------------------------------------------------
 * Replaces: BezOptimization.__init__ (optimization.py:21-63) as far as the constraint
 * closures need it, plus the class-level matrix caches of bezier.py:48-52 and the
 * "warm the caches" idiom of the drivers (Examples/Example1_DubinsCarTimeOptimal.py:133-136):
 * coefficient tables for (deg, deg_elev) are built once here and stay device-resident.
 * point_obs[M][d] are the pointObstacles that temporalSeparationConstraints appends as
 * constant curves (optimization.py:86-98).  device = HIP ordinal (>= 0). */
int obtg_ctx_create(obtg_ctx** out, int n_veh, int dim, int deg, int deg_elev,
                    int n_point_obs, const double* point_obs, int device);
void obtg_ctx_destroy(obtg_ctx*);
/* Streams.  A context starts on a stream of its own, created non-blocking: NOT ordered with the null stream.
 * obtg_ctx_set_stream: every later call goes to the caller's HIP stream, the handle taken as given -- NULL is the null
 * stream itself, which is torch's default stream: a torch user who passes torch.cuda.current_stream().cuda_stream gets
 * launches ordered with torch's own work whichever stream that is.  obtg_ctx_use_own_stream: back to the private stream.
 * (Until round 4 NULL meant "own stream", and torch's default stream, handle 0, silently un-ordered a caller's work.) */
int obtg_ctx_set_stream(obtg_ctx*, void* hip_stream);
int obtg_ctx_use_own_stream(obtg_ctx*);
/* DEG_ELEV is a module constant read at call time (optimization.py:17): allow changing it */
int obtg_ctx_set_deg_elev(obtg_ctx*, int deg_elev);
/* Angular rate with DEG_ELEV > 0 (optimization.py:578-611).  The reference elevates the position by R first and
 * forms every product at degree n+R (a degree-4(n+R) square: 441 coefficients from degree-220 operands at R = 100).
 * Elevation commutes with diff/mul/add, so by default (elevate_first = 0) the library forms numerator and
 * denominator at degree 4n from the original control points and elevates both by 4R before the element-wise
 * quotient -- the same control points up to rounding (both orders pass the same exact-rational quotient test), an order of
 * magnitude less arithmetic.  elevate_first = 1 keeps the reference's order of operations (generic kernel).
 * 2 = "exact": the default order, then the rows of vehicles that nearly stop -- a control point of |v|^2 three orders
 * below the curve's largest, where every float64 evaluation of the quotient, the reference's included, loses up to
 * 1e-8 to cancellation -- once more in double-double arithmetic, rounded once.  The pass's tables carry 64 bits, so those
 * rows are then within the row's condition number times 2^-64 of the exact rational value, 2^11 times closer than any
 * float64 evaluation: element by element 2.3e-13 relative on the worst-conditioned fixture (tests/golden/nearstop.npz,
 * where the float64 rows are 4e-10 off), 5.75e-15 of the vehicle's largest entry -- not "a few 1e-16", as this comment said
 * until tests/test_gpu_constraint_rows.py measured it.  One more (small) launch behind the dynamics launch; not in the
 * structured step. */
int obtg_ctx_set_ang_rate_order(obtg_ctx*, int elevate_first);
/* The order that is IN EFFECT for the context's present shape -- 0, 1 or 2 as above, negative = error.  A request holds
 * only where its kernels exist: DEG_ELEV = 0 has one order (0); without a products-then-elevation kernel for (deg, R) --
 * deg + 1 outside obtg_fast_kernels & 2, deg > 15, 4 R > 1000 -- the any-degree kernel runs, which elevates first (1),
 * and the double-double pass of order 2 is not run.  Callers that report which order produced their numbers ask here. */
int obtg_ctx_ang_rate_order_in_effect(obtg_ctx*);
int obtg_sync(obtg_ctx*);

/* sizes of one evaluation row's outputs, in doubles */
int obtg_len_temporal_sep(const obtg_ctx*); /* C(N+M,2) * (2n+R+1) */
int obtg_len_speed(const obtg_ctx*);        /* N * (2n+R+1)        */
int obtg_len_ang_rate(const obtg_ctx*);     /* N * (4(n+R)+1)      */
int obtg_num_pairs(const obtg_ctx*);        /* C(N+M,2)            */

/* ---- Bernstein constraint sweeps (host buffers) ----------------------------------------
 * obtg_temporal_sep: _temporalSeparationConstraints (optimization.py:311-346) through the
 *   closure of optimization.py:83-107: for every pair i<j of the N+M objects, in
 *   lexicographic order, ((v_i - v_j).normSquare().elev(R)).cpts - max_sep^2.
 *   normSquare keeps the reference's (d/2) factor (bezier.py:884).
 * obtg_speed: _maxSpeedConstraints / _minSpeedConstraints (optimization.py:349-422):
 *   per vehicle diff() [derivative then elev(1), bezier.py:497-519], normSquare, elev(R);
 *   is_max ? bound^2 - cpts : cpts - bound^2.  tf[B]: final time of each row.
 * obtg_ang_rate: _maxAngularRateConstraints -> _angularRateSqr (optimization.py:425-459,
 *   578-611), dim must be 2: max_rate^2 - num.cpts/den.cpts element-wise (inf/nan kept).
 * Limits.  A separation or speed row holds at most 1024 coefficients (2n + R + 1 <= 1024; beyond: OBTG_ERR_UNSUPPORTED);
 *   the angular rate stops at n + R = 250 outside the specialised counts.  Shapes on the any-degree kernels (dim 1,
 *   n + 1 outside obtg_fast_kernels & 1, R > 512) form the unnormalised sum  sum_j C(2n,j) c_j C(R,k-j)  of the product's
 *   coefficients c_j BEFORE dividing by C(2n+R,k), as obtg_bern_elev does, so their rows are finite only while
 *       C(R, R/2) 4^n (d/2) max|D|^2  <  DBL_MAX,
 *   D the control points of v_i - v_j (speed: of the derivative elevated by one).  At n = 2, R = 900 that allows |D| beyond
 *   1e18; at 1024 coefficients (n = 2, R = 1019, d = 2) it is |D| < 9, where the reference's elevation matrix, built from
 *   ratios, stays finite.  The specialised kernels (R <= 512) multiply by that matrix and have no such condition.
 *   The any-degree angular rate (n + 1 outside obtg_fast_kernels & 2, or the position elevated first) likewise divides
 *   C(4m,k) num_k by C(4m,k) den_k, m = n + R, both formed as plain sums: finite only while C(4m, 2m) times the largest
 *   coefficient of (y''x' - x''y')^2 stays below DBL_MAX -- no limit in practice up to m = 200; at the kernel's last
 *   m = 250, C(1000, 500) = 2.7e299 leaves 6e8 for that coefficient, which goes with tf^-6 (positions within +-10:
 *   tf > 2).  k_dynamics_elev (R > 0 on the specialised counts) scales its binomial row and has no such condition.
 * Accuracy.  Every element of these rows is within K 2^-53 M of its exact rational value, M the same formula on magnitudes
 *   (the first difference v_i - v_j as |v_i - v_j|: a swarm far from the origin loses nothing) and K the count of rounded
 *   operations: d T + 20 at R = 0 and d (n + 1) + Te + 28 at R > 0, T and Te the terms of the element's product and
 *   elevation sums, the speed rows 14 more (tests/constraint_rows_ref.py; the angular rate: its quotient form). */
int obtg_temporal_sep(obtg_ctx*, const double* Y, int B, double max_sep, double* out);
int obtg_speed(obtg_ctx*, const double* Y, const double* tf, int B, double bound, int is_max, double* out);
int obtg_ang_rate(obtg_ctx*, const double* Y, const double* tf, int B, double max_rate, double* out);
/* ---- Non-finite control points in the REDUCED separation forms -----------------------------------------------------
 * obtg_temporal_sep keeps inf / nan element by element.  Every form that reduces a pair's row -- obtg_temporal_sep_min
 * [_range][_dev], obtg_temporal_sep_active[_dev], obtg_temporal_sep_min_gather_dev, obtg_temporal_sep_fd_min_rows_dev,
 * obtg_temporal_sep_min_dev inside a view, obtg_one_vs_many_min[_spans][_dev], on the specialised and on the any-degree
 * kernels, in every launch form -- answers by the pair's FULL ROW: the 2n+R+1 values obtg_temporal_sep returns for that
 * pair on the same context (the same DEG_ELEV).
 *   1. A CLEAN row -- every element finite -- reduces to the bits of the minimum over those elements (the active form: to
 *      the elements themselves), as it always did.
 *   2. A DIRTY row -- any element NaN or +-inf, which includes finite control points whose products overflow -- reduces to
 *      NaN.  obtg_temporal_sep_active: all k values NaN and out_idx = 0 .. k-1 (in range; -1 is never written); k = 1
 *      still is obtg_temporal_sep_min, NaN for NaN.  This is what the reference's reduced form returns
 *      (Examples/SequentialSwarm.py:65, `dv.normSquare().elev(10).cpts.min()`: elev is a dense np.dot with the elevation
 *      matrix, bezier.py:469-495, so one non-finite coefficient makes the whole elevated row NaN, and ndarray.min() keeps
 *      it) and what the true-minimum families below state.  The values are inequality rows of SLSQP, whose iterates do
 *      become non-finite: a finite or +inf ("feasible") answer to such an iterate hides it.
 *   3. obtg_one_vs_many_min_spans: a pair whose spans do not overlap returns `no_overlap` whatever its control points hold
 *      (the reference returns None before it looks at them); a pair that overlaps follows 1 and 2 on the CUT curves.
 * Every reduction has one definition, RowMin (csrc/bern_device.h): the minimum, and whether any value was not finite.
 * Not covered: the full rows themselves.  Their element-wise pattern may be NARROWER than the reference's all-NaN row --
 * band-limited elevation sums skip the 0 * nan terms of np.dot -- which rule 2 does not depend on: one non-finite element
 * makes the row dirty.  The searches with data-dependent loops (gjk*, min_dist*, obtg_gjk_true_pairs) promise nothing on
 * non-finite input; obtg_coll_check and obtg_coll_check2poly return the reference's value for it (see there);
 * obtg_min_dist_robust and obtg_min_dist2poly_robust return NaN for it without searching (see there). */
/* fused per-pair minimum of the elevated separation control points minus max_sep^2
 * (the `dv.normSquare().min()` variant commented at optimization.py:338 and used by
 * Examples/SequentialSwarm.py:65): out[B][C(N+M,2)].  A pair with a non-finite element in its full row: NaN (rules 1, 2 above). */
int obtg_temporal_sep_min(obtg_ctx*, const double* Y, int B, double max_sep, double* out);
/* SURVEY.md 8(f) item 4 as the survey words it -- "feed SLSQP only active / near-active constraint rows": per pair the k
 * SMALLEST of its 2n+R+1 elevated separation control points (minus max_sep^2) -- among equal values the lower
 * control-point index is taken first --, listed in ascending control-point INDEX.  1 <= k <= 4 (and k <= 2n+R+1):
 * out_val[B][P][k], out_idx[B][P][k] (nullable) = which control points they are.  k is fixed, so the constraint vector
 * has a constant length P k -- what SLSQP needs -- and in index order a row follows one control point, a polynomial in
 * x, for as long as the membership of the set stands: the rows kink only where the k-th and (k+1)-th smallest cross (in
 * value order they would kink at every crossing inside the set as well).  k = 1 is obtg_temporal_sep_min.  The specialised kernels select in the epilogue of their reduced form (one lane holds a pair's
 * control points: a branch-free insertion into four registers per value); other degrees write the rows to a workspace and
 * select in a second launch.  Same values as the corresponding entries of obtg_temporal_sep, bit for bit.
 * A pair with a non-finite element in its full row (rule 2 above): out_val NaN in all k places, out_idx 0 .. k-1 -- no
 * control point is "the smallest" of such a row, and an index is always one that can be gathered with.
 * optimization.py:337-338 is where the reference builds the full rows / leaves the minimum commented out. */
int obtg_temporal_sep_active(obtg_ctx*, const double* Y, int B, double max_sep, int k, double* out_val, int* out_idx);
/* the same restricted to pairs [pair_begin, pair_begin+pair_count) of the lexicographic list:
 * out[B][pair_count].  With pair_begin = 0, pair_count = N-1 this is the one-vs-many constraint
 * of Examples/SequentialSwarm.py:43-70 (vehicle 0 against every other one).  Non-finite rows: NaN (rules 1, 2 above). */
int obtg_temporal_sep_min_range(obtg_ctx*, const double* Y, int B, double max_sep,
                                int pair_begin, int pair_count, double* out);

/* Structured finite differences of the temporal-separation family (the `jac`
 * entry a driver adds next to optimization.py:83-107).  Perturbation t sets element (pert_row[t],
 * pert_col[t]) of the evaluation row Y0[(n_veh*dim)][deg+1] to pert_val[t] -- one control-point
 * coordinate of vehicle v_t = pert_row[t] / dim -- so only the n_obj-1 pairs containing v_t change.
 * out_blk[n_pert][n_obj-1][2n+R+1]: block t holds, for the partners u = 0..n_obj-1, u != v_t in
 * increasing order, the constraint values of pair {v_t, u} under perturbation t; they equal the
 * corresponding entries of obtg_temporal_sep on the fully perturbed row bit for bit, the rest of
 * that row equals the unperturbed evaluation.  n_x (N-1) pair evaluations instead of n_x C(N,2).
 * OBTG_ERR_UNSUPPORTED for shapes outside the specialised kernels (use the batch form then). */
int obtg_temporal_sep_fd(obtg_ctx*, const double* Y0, int n_pert, const int* pert_row, const int* pert_col,
                         const double* pert_val, double max_sep, double* out_blk);
int obtg_temporal_sep_fd_dev(obtg_ctx*, const double* dY0, int n_pert, const int* d_pert_row,
                             const int* d_pert_col, const double* d_pert_val, double max_sep, double* d_out_blk);

/* ---- one curve against K others (Examples/SequentialSwarm.py:43-70, the sequential planner's constraint) ----------
 * out[b][k] = min over the elevated control points of |one_b - many_k|^2 (normSquare's (d/2) factor kept), minus
 * max_sep^2: `dv = vehTraj - tempTraj; dv.normSquare().elev(DEG_ELEV).cpts.min() - maxSep**2` (the example hard-codes
 * elev(10); here DEG_ELEV is the context's).  one[B][dim][deg+1] are B candidates of the one curve (B = 1 for a plain
 * callback, n_x + 1 for a finite-difference batch of the vehicle being planned), many[K][dim][deg+1] the curves it is
 * checked against.  No pair table: the context fixes (dim, deg, DEG_ELEV) only -- its vehicle count is not used -- and K
 * may differ from call to call (the planner's K grows by one per vehicle).  Degrees with a specialised kernel
 * (obtg_fast_kernels(dim, deg) & 1), others OBTG_ERR_UNSUPPORTED.  A pair whose elevated control points are not all finite
 * (a NaN or +-inf control point in either curve, products that overflow): NaN, as the reference's `.min()` (rules 1, 2 above;
 * the full row of a pair is obtg_temporal_sep's for the two curves as vehicles of one context). */
int obtg_one_vs_many_min(obtg_ctx*, const double* one, int B, const double* many, int K, double max_sep, double* out /*[B][K]*/);
int obtg_one_vs_many_min_dev(obtg_ctx*, const double* d_one, int B, const double* d_many, int K, double max_sep, double* d_out);
/* The same for curves that live on DIFFERENT time spans: one_span[B][2], many_span[K][2] hold (t0, tf) per curve.  The
 * reference's Bezier.sub does this through _temporalAlignment (bezier.py:347-374, 903-941 -> split 533-572 ->
 * deCasteljauSplit 985-1027): both curves are cut down to the overlap [a, e] = [max t0, min tf] -- a curve that starts
 * before a is split at (a - t0)/(tf - t0) and its right piece kept, then, if it ends after e, that piece is split at
 * (e - a)/(tf - a) and its left piece kept; an end that already is the overlap's is not touched -- and the difference,
 * normSquare, elev and minimum run on the pieces.  Pairs with a >= e (disjoint or touching spans: the reference returns
 * None) get `no_overlap`, whatever their control points hold (rule 3 above); a pair that overlaps and whose CUT curves give
 * a non-finite elevated control point gets NaN.  A call whose spans are all equal takes no split and equals
 * obtg_one_vs_many_min bit for bit.
 * Degrees without a specialised kernel run a runtime-degree form up to 2 deg + DEG_ELEV + 1 <= 1024 (the any-degree
 * separation kernel's limit); beyond, and for any span with t0 >= tf: OBTG_ERR_ARG.
 * _dev: the curves and the output are device pointers; the spans stay HOST arrays (16 bytes per curve: they are checked
 * without a round trip to the device; the call returns once they are copied, the kernel runs asynchronously on the
 * context's stream). */
int obtg_one_vs_many_min_spans(obtg_ctx*, const double* one, const double* one_span, int B, const double* many,
                               const double* many_span, int K, double max_sep, double no_overlap, double* out /*[B][K]*/);
int obtg_one_vs_many_min_spans_dev(obtg_ctx*, const double* d_one, const double* one_span, int B, const double* d_many,
                                   const double* many_span, int K, double max_sep, double no_overlap, double* d_out);

/* ---- same sweeps on DEVICE pointers, asynchronous on the context's stream ---------------
 * pair_begin/pair_count select a contiguous block of the lexicographic pair list (the
 * pair-partitioned multi-GPU mode); out rows then hold only that block:
 * out[B][pair_count*(2n+R+1)].  Pass 0, obtg_num_pairs() for everything.  obtg_temporal_sep_min_dev and
 * obtg_temporal_sep_active_dev follow the non-finite rules of their host forms (NaN for a dirty row, indices 0 .. k-1),
 * with dY and inside a view alike. */
int obtg_temporal_sep_dev(obtg_ctx*, const double* dY, int B, double max_sep,
                          int pair_begin, int pair_count, double* d_out);
int obtg_temporal_sep_min_dev(obtg_ctx*, const double* dY, int B, double max_sep,
                              int pair_begin, int pair_count, double* d_out);
int obtg_temporal_sep_active_dev(obtg_ctx*, const double* dY, int B, double max_sep, int k,
                                 int pair_begin, int pair_count, double* d_out_val, int* d_out_idx /*nullable*/);
int obtg_speed_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, int is_max,
                   double* d_out);
int obtg_ang_rate_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double max_rate,
                      double* d_out);
/* speed and angular-rate constraints of the same rows in one launch (they share the derivative
 * curves: for d = 2 the speed curve is the angular rate's denominator before squaring,
 * optimization.py:380 vs 605).  Either output may be NULL. */
int obtg_dynamics_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double speed_bound,
                      int speed_is_max, double max_rate, double* d_out_speed, double* d_out_ang);
/* BOTH speed bounds from one pass.  The reference exposes minSpeedConstraints and maxSpeedConstraints
 * (optimization.py:135-169, 349-422): the same elevated |v|^2 curve, once as cpts - vmin^2 and once as vmax^2 - cpts.
 * While d_out2 is set (device, [B][N*(2n+R+1)]; NULL = off), every pass that writes speed rows through
 * obtg_dynamics[_fd]_dev or obtg_constraint_sweep_dev also writes the rows of this second bound from the curve it
 * has in registers -- no second launch, no second evaluation of the derivative curves. */
int obtg_ctx_set_second_speed_bound(obtg_ctx*, double bound, int is_max, double* d_out2);

/* ---- finite-difference batch on the device --------------------------------------------
 * Replaces the n_x+1 serial calls SciPy's approx_derivative makes: builds
 * dY[B][N*d][n+1] with row 0 = Y and row k = Y with the k-th free control point
 * (interior columns, row-major as x.reshape(numRows,numCols), optimization.py:283)
 * advanced by h.  n_fixed_cols = columns pinned at each end (1: end points; 2: + speed
 * columns).  B <= N*d*(n+1-2*n_fixed_cols) + 1. */
int obtg_fd_batch_dev(obtg_ctx*, const double* dY0, int n_fixed_cols, double h, int B, double* dY);

/* The same batch WITHOUT writing it: a VIEW.  Between obtg_fd_view_begin and obtg_fd_view_end every `_dev` sweep
 * (temporal_sep[_min], speed, ang_rate, dynamics, gjk_swarm, pair_sweep) may be called with dY = NULL and the view's B:
 * it then evaluates the virtual batch whose row 0 is dY0 and whose row b >= 1 is dY0 with its (b-1)-th free control point
 * advanced by h -- bit for bit the rows obtg_fd_batch_dev(dY0, n_fixed_cols, h, B) writes.  Kernels with an on-the-fly
 * form build the rows while staging their inputs (the B x 11 KB batch never travels through HBM); for the others the
 * batch is written to a context buffer, once per view.  Results are identical either way.  dY0 must stay valid until the
 * view ends.  obtg_pair_sweep_fd_dev / obtg_dynamics_fd_dev are the one-call forms (a view around a single sweep);
 * obtg_fd_forms_on_the_fly: bit 0 = the pair sweep is one launch forming its rows itself, bit 1 = the dynamics launch. */
int obtg_fd_view_begin(obtg_ctx*, const double* dY0, int n_fixed_cols, double h, int B);
/* A RANGE of that batch's rows: the view's local row b is batch row row_begin + b (B rows).  What one of G processes
 * opens when an SLSQP iteration's n_x + 1 rows are sharded over G GPUs (distributed.shard_rows): no rank
 * writes or reads rows it does not own.  The structured step's form of it: obtg_constraint_sweep_fd_structured_rows_dev. */
int obtg_fd_view_begin_rows(obtg_ctx*, const double* dY0, int n_fixed_cols, double h, int row_begin, int B);
int obtg_fd_view_end(obtg_ctx*);
int obtg_fd_forms_on_the_fly(const obtg_ctx*);
int obtg_pair_sweep_fd_dev(obtg_ctx*, const double* dY0, int n_fixed_cols, double h, int B, double max_sep,
                           double* d_out_sep, int max_iter, int md_cap, int* d_flag, double* d_p1, double* d_p2,
                           double* d_dist, int* d_nsup, int* d_status);
int obtg_dynamics_fd_dev(obtg_ctx*, const double* dY0, int n_fixed_cols, double h, const double* d_tf, int B,
                         double speed_bound, int speed_is_max, double max_rate, double* d_out_speed, double* d_out_ang);

/* ---- GJK (gjk/gjk.py:230-270 gjkNew, 273-360 minimumDistance) ---------------------------
 * Generic point sets: pts[n_pts][3], poly_off[n_poly+1]; pair k = (pair_a[k], pair_b[k]).
 * Outputs per pair: flag in {-1,0,1} (gjk.py:234-237); p1/p2 = closest points on poly1/poly2
 * and dist when flag == 1 (NaN otherwise); n_support = number of supportPts calls;
 * support_trace (nullable) [n_pairs][trace_cap][2] int16 = (index into poly1, index into
 * poly2) of every supportPts call in order (bit-exact parity target); status as OBTG_ST_*.
 * The reference's decision sequence is followed exactly, including its early exits. */
int obtg_gjk_pairs(obtg_ctx*, const double* pts, int n_pts, const int* poly_off, int n_poly,
                   const int* pair_a, const int* pair_b, int n_pairs, int max_iter, int md_cap,
                   int* flag, double* p1, double* p2, double* dist,
                   short* support_trace, int trace_cap, int* n_support, int* status);

/* Batched swarm sweep: hulls of the N vehicles of each of the B rows (control polygons,
 * 2-D padded with z = 0 as bezier.py:1294-1308 does) plus the static polygons registered
 * with obtg_ctx_set_polygons (object ids N .. N+n_poly-1).  Pair list is device-resident
 * after obtg_ctx_set_hull_pairs.  Outputs are DEVICE arrays:
 * d_flag[B][n_pairs] int32, d_p1/d_p2[B][n_pairs][3], d_dist[B][n_pairs],
 * d_nsup[B][n_pairs] int32 (nullable), d_status[B][n_pairs] int32 (nullable).
 * obtg_ctx_set_polygons drops the pair list (object ids change meaning): the sweeps return OBTG_ERR_ARG until
 * obtg_ctx_set_hull_pairs has been called again. */
int obtg_ctx_set_polygons(obtg_ctx*, const double* pts, int n_pts, const int* poly_off, int n_poly);
int obtg_ctx_set_hull_pairs(obtg_ctx*, const int* pair_a, const int* pair_b, int n_pairs);
int obtg_gjk_swarm_dev(obtg_ctx*, const double* dY, int B, int max_iter, int md_cap,
                       int* d_flag, double* d_p1, double* d_p2, double* d_dist,
                       int* d_nsup, int* d_status);
/* The N x N pair sweep of a batch in ONE launch: obtg_temporal_sep_dev (all pairs) and
 * obtg_gjk_swarm_dev for the same B rows.  The workgroups of the planar gjkNew sweep have the row's
 * control points in LDS anyway; each also writes its share of the row's temporal-separation block
 * (part before, part after its gjkNew phases, staggered between workgroups), whose HBM stores then
 * drain under the VALU-bound gjkNew work of the other wavefronts.  Outputs are those of the two
 * separate calls, bit for bit.  Rows whose hulls exceed 48 KB of LDS (256 vehicles of degree 15) take the
 * tiled form of the same idea when the hull pair list holds every vehicle pair: a chunk of the tiled sweep
 * stages one TA x 64 tile of the pair matrix and writes that tile's separation rows.  3-D rows: the 3-D
 * sweep's workgroups run their part of the separation block first (obtg_constraint_sweep_dev: and of the
 * speed rows), one launch as well.  Point obstacles (constant curves in the separation pairs, optimization.py:86-98; no
 * part of the hull sweep) are staged behind the hull objects by the planar grid: one launch too, for rows within 48 KB.
 * Shapes without such a kernel (DEG_ELEV > 0, de-duplication on, point obstacles with large or 3-D rows) fall back to the
 * two launches. */
int obtg_pair_sweep_dev(obtg_ctx*, const double* dY, int B, double max_sep, double* d_out_sep,
                        int max_iter, int md_cap, int* d_flag, double* d_p1, double* d_p2,
                        double* d_dist, int* d_nsup, int* d_status);
/* EVERY constraint family of the batch in one call: obtg_pair_sweep_dev (temporal separation + gjkNew hull sweep) and
 * obtg_dynamics_dev (max/min speed + angular rate; d_out_ang may be NULL) of the same B rows -- what one evaluation of an
 * SLSQP step needs, as the library's best launch sequence for the shape (ONE launch for planar DEG_ELEV = 0 rows and 3-D
 * rows; two for planar DEG_ELEV > 0: the gjkNew sweep, and the separation rows with the speed / angular-rate groups).  Outputs are those of the two separate calls, bit for bit.  dY may be NULL inside an obtg_fd_view.
 * Inside a view, with dY = NULL, B the view's B and d_out_ang given, the call says "these rows are x + h e_b": on planar
 * DEG_ELEV = 0 shapes whose brute-force step is one launch and which the structured step covers (see
 * obtg_constraint_sweep_fd_structured_dev) the ONE launch is that step (k_step_fd_structured; row-range views included,
 * still timed as OBTG_K_PAIR_SWEEP) -- the same arrays, bit for bit, d_nsup / d_status written when given, without
 * evaluating row 0's pairs and vehicles once per row.  Every other shape (3-D, DEG_ELEV > 0, deg + 1 = 21, de-duplication
 * on, a materialised view, d_out_ang = NULL) and every call with a batch of the caller's (dY != NULL) runs the brute-force
 * launches as before; OBTG_ERR_UNSUPPORTED is never returned for want of a structured kernel.
 * obtg_ctx_set_fd_view_structured(ctx, 0) turns the routing off for a context. */
int obtg_constraint_sweep_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double max_sep, double* d_out_sep,
                              double speed_bound, int speed_is_max, double max_rate, double* d_out_speed,
                              double* d_out_ang, int max_iter, int md_cap, int* d_flag, double* d_p1, double* d_p2,
                              double* d_dist, int* d_nsup, int* d_status);
/* ---- the collective behind the C ABI: one process per GPU, RCCL over xGMI ------------------------
 * For callers that bind this library without PyTorch (INTEGRATION.md route 2); the Python layer's distributed.py does the
 * same through torch.distributed.  RCCL is loaded at run time (librccl.so.1, or the file OBTG_RCCL_LIB names): without it
 * these calls return OBTG_ERR_UNSUPPORTED and nothing else in the library is affected.
 *   rank 0:      obtg_comm_unique_id(id)             -- 128 bytes, handed to the other ranks by the caller's own means
 *                                                       (a file, a socket, MPI: the library opens no connection of its own)
 *   every rank:  obtg_comm_create(&comm, n_ranks, rank, id, device)      (collective: returns when all ranks have called)
 * obtg_comm_all_gather_dev: bytes_per_rank bytes of d_send from every rank into d_recv[n_ranks][bytes_per_rank], on the
 * CONTEXT's stream (ordered with its launches; obtg_sync completes it).
 * obtg_temporal_sep_min_gather_dev: what north_star names -- the swarm's pair list partitioned over the ranks (contiguous
 * balanced blocks of the lexicographic list, the first P mod G ranks one pair more), each rank evaluating the per-pair
 * separation minima of ITS block for the B rows (every rank holds all control points: dY, or an open view with dY = NULL),
 * ONE all-gather of 8 B P bytes in all, and d_min_all[B][P] complete on every rank.  The reference loops over every pair
 * in one process (optimization.py:311-346); the minimum per pair is its commented form at optimization.py:338.  Every
 * rank's block is obtg_temporal_sep_min_dev's: NaN for a pair with a non-finite element in its full row. */
typedef struct obtg_comm obtg_comm;
int obtg_comm_unique_id(unsigned char* id /*[128]*/);
int obtg_comm_create(obtg_comm** out, int n_ranks, int rank, const unsigned char* id /*[128]*/, int device);
void obtg_comm_destroy(obtg_comm*);
int obtg_comm_size(const obtg_comm*);
int obtg_comm_rank(const obtg_comm*);
const char* obtg_comm_last_error(const obtg_comm*);   /* NULL: the calling thread's last failure without a communicator (obtg_comm_unique_id, obtg_comm_create) */
int obtg_comm_all_gather_dev(obtg_comm*, obtg_ctx*, const void* d_send, void* d_recv, size_t bytes_per_rank);
int obtg_temporal_sep_min_gather_dev(obtg_ctx*, obtg_comm*, const double* dY, int B, double max_sep, double* d_min_all /*[B][P]*/);
/* The two pieces of it for callers with a collective of their own (MPI, a host-staged exchange): rank's block of the pair
 * list, and rank blocks [n_ranks][B * ceil(P / n_ranks)] (rank r's `count_r` minima of row 0, then of row 1, ...: what
 * obtg_temporal_sep_min_dev(pair_begin, pair_count) writes, padded to the largest block) -> rows d_rows[B][P]. */
/* What a rank of a ROW-sharded finite-difference step sends when the per-pair minima of every row are wanted in one place
 * (distributed.SparseMinimaGather): batch row b >= 1 differs from row 0 only in the n_obj - 1 pairs of the vehicle
 * it advances, so for the rows [row_begin, row_begin + n_rows) of the batch over dY0 (obtg_fd_view_begin's rows, row_begin >= 1)
 * d_out[n_rows][n_obj - 1] holds, per row, the minima of exactly those pairs, partners ascending -- evaluated from dY0
 * directly (n_rows (n_obj - 1) pair evaluations; no [B][P] block is formed), the same bits as the corresponding entries of
 * obtg_temporal_sep_min_dev inside the view -- NaN for NaN: a pair with a non-finite element in its full row is NaN in both
 * (rules 1, 2 of the reduced forms).  Row 0's P minima are obtg_temporal_sep_min_dev(dY0, 1, ...). */
int obtg_temporal_sep_fd_min_rows_dev(obtg_ctx*, const double* dY0, int n_fixed_cols, double h, int row_begin, int n_rows,
                                      double max_sep, double* d_out);
int obtg_pair_block(const obtg_ctx*, int n_ranks, int rank, int* begin, int* count);
int obtg_unpack_pair_blocks_dev(obtg_ctx*, const double* d_blocks, int B, int n_ranks, double* d_rows);

/* The whole finite-difference step as ONE launch that does not repeat row 0's work (SURVEY.md 8(f) item 1 for every
 * family; what SciPy's approx_derivative needs from optimization.py:83-187 per SLSQP iteration).  The rows of the view
 * (dY0, n_fixed_cols, h, B) differ from row 0 in ONE vehicle each: the launch evaluates row 0 in full and streams its
 * results into all B rows, while one workgroup per row evaluates only the N-1 separation pairs, the hull pairs and the
 * vehicle its advanced control point touches.  Outputs are those of obtg_constraint_sweep_dev inside the same view,
 * bit for bit (the same device functions evaluate every pair); the launch is bound by its stores instead of by gjkNew.
 * Planar shapes (obtg_fast_kernels & 4: deg + 1 in {4, 6, 8, 9, 11}, with or without point obstacles -- constant curves of the separation pair table,
 * optimization.py:86-98 --, angular rate wanted, a row's objects within 40 KB of LDS), any
 * DEG_ELEV with 2 deg + DEG_ELEV + 1 <= 512 -- for DEG_ELEV > 0 (where the brute-force step is two launches) the separation
 * streams are the elevated rows and the dynamics groups are the elevated kernel's; at DEG_ELEV = 0 also deg + 1 = 16 and, for
 * deg + 1 in {11, 16}, rows of up to 158 KB (256 vehicles of degree 15 are 70 KB: two workgroups per CU):
 * OBTG_ERR_UNSUPPORTED otherwise -- the brute-force call gives the same numbers.  d_tf is read per row: the speed /
 * angular-rate rows of row 0 are copied only into rows whose tf equals tf[0] bit for bit, any other row is evaluated in full.  A different evaluation strategy from
 * "every row in full" with the same bits: obtg_constraint_sweep_dev inside a view routes to it where it applies, so bench.py's
 * headline value is this launch and variants.fd_structured repeats it through this entry point.  The call is a view
 * of its own (begin .. end around its launch): with a view of the caller's open on the context it returns OBTG_ERR_ARG
 * instead of replacing and closing that view.
 * ..._rows_dev: the same for the row RANGE [row_begin, row_begin + B) of the batch (what obtg_fd_view_begin_rows views; d_tf and
 * every output hold the range's B rows): what one of G processes calls when an SLSQP iteration's n_x + 1 rows are sharded over
 * G GPUs.  The unperturbed row is evaluated by every rank (it is the source of the streams); a range that
 * does not hold the batch's row 0 has a perturbed row as its local row 0.  Bit for bit the rows of the whole-batch call. */
int obtg_constraint_sweep_fd_structured_dev(obtg_ctx*, const double* dY0, int n_fixed_cols, double h, const double* d_tf,
                                            int B, double max_sep, double* d_out_sep, double speed_bound, int speed_is_max,
                                            double max_rate, double* d_out_speed, double* d_out_ang, int max_iter, int md_cap,
                                            int* d_flag, double* d_p1, double* d_p2, double* d_dist, int* d_nsup,
                                            int* d_status);
int obtg_constraint_sweep_fd_structured_rows_dev(obtg_ctx*, const double* dY0, int n_fixed_cols, double h, int row_begin,
                                                 const double* d_tf, int B, double max_sep, double* d_out_sep, double speed_bound,
                                                 int speed_is_max, double max_rate, double* d_out_speed, double* d_out_ang,
                                                 int max_iter, int md_cap, int* d_flag, double* d_p1, double* d_p2, double* d_dist,
                                                 int* d_nsup, int* d_status);
/* Finite-difference de-duplication (off by default).  The rows of one
 * SLSQP Jacobian differ from row 0 in ONE vehicle, so all pairs not involving it have row 0's
 * inputs bit for bit.  When on, obtg_gjk_swarm[_dev] compares every row with row 0 (bitwise, per
 * vehicle), runs gjkNew only for pairs with a changed hull and copies row 0's outputs for the
 * rest.  Results are identical to the brute-force sweep for any input. */
int obtg_ctx_set_fd_dedup(obtg_ctx*, int on);
/* Structured routing of obtg_constraint_sweep_dev inside a view (see there; on by default, and off by default for contexts
 * created while the environment holds OBTG_FD_VIEW_STRUCTURED=0).  Off: the view's rows are evaluated in full, row by row,
 * by the brute-force launch.  The outputs are the same bits either way: the switch is for A/B timing on one build and for
 * tests that want the brute-force launch as the independent side.  obtg_pair_sweep_dev / obtg_dynamics_dev are not routed. */
int obtg_ctx_set_fd_view_structured(obtg_ctx*, int on);
/* Trip-count history of the planar sweep (on by default).  Each obtg_gjk_swarm[_dev] call keeps one
 * byte per (row, pair): the number of support scans gjkNew took.  The next call evaluates every
 * workgroup's pairs in descending order of that count, so that the lanes of a wavefront finish and
 * refill together (SLSQP's consecutive calls see nearly the same geometry).  Scheduling only:
 * every pair is evaluated in full and the outputs do not depend on the order.  Off = list order. */
int obtg_ctx_set_gjk_history(obtg_ctx*, int on);
/* Which form and grid the hull-pair sweep of B rows takes on this context, as the launchers would decide it now (the
 * environment's OBTG_SWEEP_WGS / OBTG_SWEEP_PASSES / OBTG_TILE_A included): a read-only question for tests and A/B runs that
 * force a shape and want to know that it is in effect.  Launches nothing; may build what the launch would (the context's
 * tables, the tiled forms' chunk tables).
 *   which = 0: the plain gjkNew sweep, obtg_gjk_swarm[_dev];  which = 1: obtg_pair_sweep_dev, and with want_dyn != 0
 *   obtg_constraint_sweep_dev with every family wanted (brute-force launches; the structured step of a view is not asked).
 *   out[0] form: 1 = one launch of the planar sweep (rows that fit LDS), 2 = the tiled sweep (large rows), 3 = the general
 *          kernel (3-D, polygons with more points than a hull, ...; out[1 .. 4] are 0), 4 = the finite-difference
 *          de-duplicated sequence (which = 0 with obtg_ctx_set_fd_dedup on), 0 = two launches (which = 1 only: the plain
 *          sweep, which out[1 .. 4] then describe, and the separation rows)
 *   out[1] workgroups per row, out[2] passes of a workgroup over one staging, out[3] hull pairs per pass (tiled: chunks per
 *          row, 1, the longest chunk), out[4] tile height (tiled forms, else 0),
 *   out[5] lanes that must be idle before a batch of them refills (OBTG_REFILL_MIN, read once per process),
 *   out[6] shift of the trip-count bins of the history order (OBTG_HIST_SHIFT, once per process),
 *   out[7] 1: the speed / angular-rate groups ride in the sweep's grid (which = 1, want_dyn). */
int obtg_sweep_shape(obtg_ctx*, int B, int which, int want_dyn, int* out /*[8]*/);
/* host-buffer form of the same sweep (B rows of Y in, arrays out) */
int obtg_gjk_swarm(obtg_ctx*, const double* Y, int B, int max_iter, int md_cap,
                   int* flag, double* p1, double* p2, double* dist, int* nsup, int* status);

/* Robust curve <-> curve minimum distance (NOT the reference's algorithm): breadth-first
 * branch & bound on the parameter square with bounds that are valid for the curves themselves -- upper: distances
 * between end points of sub-curves; lower: gap of the two control polygons projected on the direction between the
 * sub-curves' mid points.  res[n_pairs][3] = (dist, t1, t2) with dist within a relative eps of the true minimum, or
 * below eps x (largest coordinate) when the curves touch, when status == OBTG_MD_OK; OBTG_MD_NODE_CAP (node budget max_nodes or the internal frontier of 1024 nodes per
 * pair exhausted) and OBTG_MD_DEPTH_CAP (level 48) return the best distance found so far, an upper bound.
 * info[n_pairs][4] = (nodes, levels, largest frontier, status).  Use where `_minDist`'s known defects matter
 * (bezier.py:1283-1408 on gjkNew: non-minimal hull distances used as lower bounds, unbounded loops).
 * In every status dist is the distance between the points of the curves at (t1, t2), which are multiples of a power of 1/2
 * in [0, 1], to within 22 x 2^-53 x (largest coordinate) of rounding (measured: 5.4; tests/test_gpu_robust_distance.py).
 * eps down to 1e-12 has been held to exact rationals: a result with OBTG_MD_OK meets the contract; where eps x dist is below
 * the rounding of the coordinates the search cannot close and ends with OBTG_MD_NODE_CAP.  A curve whose control points
 * are all the same point is searched along the other curve's parameter only.
 * Non-finite input: a pair with a NaN or an inf in any coordinate of either curve is not searched and returns
 * res = (NaN, -1, -1), info = (0, 0, 0, OBTG_MD_OK), status OBTG_MD_OK -- NaN for NaN, the rule of the true-minimum row
 * families --; the other pairs of the call are not affected. */
int obtg_min_dist_robust(obtg_ctx*, const double* curves, int n_curves, int K, const int* pair_a, const int* pair_b,
                         int n_pairs, double eps, int max_nodes, double* res, int* info, int* status);
/* The curve <-> polygon form of the robust search (NOT the reference's `_minDist2Poly`, bezier.py:1411-1496): branch &
 * bound on the curve parameter with bounds that hold for the curve itself -- upper: true distances from sub-curve end
 * points to the polygon's convex hull; lower: the certified lower bound of the true distance between the sub-curve's
 * control hull and the polygon's hull (obtg_gjk_true_pairs' algorithm).  res[n_pairs][5] = (dist, t, closest point on the
 * polygon's hull[3]); info / status as obtg_min_dist_robust.
 * dist is the distance between the curve's point at t and the returned polygon point, a point of the hull, to within
 * 10 x 2^-53 x (largest coordinate) of rounding (measured: 2.3) -- also where the curve touches the polygon.
 * Non-finite input: a pair with a NaN or an inf in any coordinate of its curve or of its polygon is not searched and
 * returns res = (NaN, -1, NaN, NaN, NaN), info = (0, 0, 0, OBTG_MD_OK), status OBTG_MD_OK; the other pairs are not affected. */
int obtg_min_dist2poly_robust(obtg_ctx*, const double* curves, int n_curves, int K, const double* pts, int n_pts,
                              const int* poly_off, int n_poly, const int* pair_curve, const int* pair_poly, int n_pairs,
                              double eps, int max_nodes, double* res, int* info, int* status);
/* True distance between the convex hulls of two point sets (opt-in; NOT gjkNew, which stops at a non-minimal distance
 * on ~30 % of separated pairs and never exits on some 3-D inputs -- SURVEY.md 8(a) G2): a textbook GJK whose exit test
 * is a certificate, dist >= hull distance >= lower with dist - lower <= eps * dist.  Same point-set / pair conventions as
 * obtg_gjk_pairs.  flag 1 separated (p1 / p2 = closest points, dist), 0 intersecting or touching (dist 0);
 * lower, iters, status are nullable; status 0 = converged with that certificate, 1 = iteration cap, 2 = stalled at
 * rounding level before the certificate closed (dist is still a distance between hull points, `lower` still a proven
 * lower bound: compare the two). */
int obtg_gjk_true_pairs(obtg_ctx*, const double* pts, int n_pts, const int* poly_off, int n_poly,
                        const int* pair_a, const int* pair_b, int n_pairs, double eps, int max_iter,
                        int* flag, double* p1, double* p2, double* dist, double* lower, int* iters, int* status);
/* ---- curve <-> curve / curve <-> polygon minimum distance --------------------------------
 * Bezier.minDist -> _minDist (bezier.py:840-852, 1283-1408) and Bezier.minDist2Poly ->
 * _minDist2Poly (bezier.py:854-857, 1411-1496): branch and bound over de Casteljau
 * subdivisions with gjkNew lower bounds.  curves[n_curves][3][K] (2-D curves carry a zero
 * z row).  res[n_pairs][3] = (alpha, t1, t2); for the polygon form res[n_pairs][5] =
 * (alpha, t1, closest point on polygon[3]).  info[n_pairs][4] (nullable) = nodes visited,
 * gjkNew calls, max depth, status; status[n_pairs] as OBTG_MD_*. */
int obtg_min_dist(obtg_ctx*, const double* curves, int n_curves, int K,
                  const int* pair_a, const int* pair_b, int n_pairs,
                  double eps, int max_iter, int md_cap, int max_depth, int max_nodes,
                  double* res, int* info, int* status);
/* `_minDist` (bezier.py:1283-1408) on curves of DIFFERENT degree, as the reference takes them: poly1 / poly2 are each
 * curve's own control points, t1 = p1idx[0] / c1.deg, t2 = p2idx[0] / c2.deg, and each curve is split by its own de
 * Casteljau.  Curve i has K_i = curve_off[i + 1] - curve_off[i] control points (2 <= K_i <= 32; curve_off[0] = 0) and is
 * stored as [3][K_i] row-major at cpts + 3 * curve_off[i]; 2-D curves carry a zero z row.  res, info and status as for
 * obtg_min_dist.  OBTG_ERR_ARG: null pointers, offsets that do not ascend or any K_i < 2, pair indices out of range;
 * OBTG_ERR_UNSUPPORTED: any K_i > 32 (or a max_depth above 760, whose frames no workgroup's LDS holds).  Where every K_i
 * is equal the call is obtg_min_dist on the same arrays, bit for bit. */
int obtg_min_dist_mixed(obtg_ctx*, const double* cpts, const int* curve_off, int n_curves,
                        const int* pair_a, const int* pair_b, int n_pairs,
                        double eps, int max_iter, int md_cap, int max_depth, int max_nodes,
                        double* res, int* info, int* status);
int obtg_min_dist2poly(obtg_ctx*, const double* curves, int n_curves, int K,
                       const double* pts, int n_pts, const int* poly_off, int n_poly,
                       const int* pair_curve, const int* pair_poly, int n_pairs,
                       double eps, int max_iter, int md_cap, int max_depth, int max_nodes,
                       double* res, int* info, int* status);
/* ---- curve <-> curve / curve <-> polygon collision check --------------------------------
 * Bezier.collCheck -> _collCheckBez2Bez (bezier.py:859-862, 1561-1614) and Bezier.collCheck2Poly ->
 * _collCheckBez2Poly (bezier.py:864-867, 1617-1651): depth-first subdivision at 0.5 that asks gjkNew for its flag
 * alone and stops at the first separated pair of hulls.  Layouts as obtg_min_dist / obtg_min_dist2poly; at most 16
 * control points per curve and 16 vertices per polygon (more: OBTG_ERR_UNSUPPORTED).
 * res[n_pairs] is the reference's return value: curve <-> curve 1 (hulls separated: no collision), -1 (its `cnt > 100`),
 * 0.0 or the smallest end-point distance met on the way; curve <-> polygon 1 or 0.  `cnt > 100` is part of that value,
 * not a status: there is no max_depth.  info[n_pairs][4] (nullable) = nodes visited (every one makes one gjkNew
 * call), gjkNew calls, max depth (the reference's cnt, at most 100), status; status[n_pairs]: OBTG_MD_OK,
 * OBTG_MD_NODE_CAP (max_nodes visited: the reference does not return in reasonable time) or OBTG_MD_GJK_CAP (an
 * inner gjkNew that never returns: a proven cycle or md_cap rounds).  res is 0 beside a status other than OBTG_MD_OK.
 * max_iter, md_cap or max_nodes below 1: OBTG_ERR_ARG (a search of max_nodes = 1 visits the root and, unless it ends
 * there, stops with OBTG_MD_NODE_CAP).
 * Non-finite input (NaN, +inf or -inf in a control point or a vertex) is not an error: both calls return what the
 * reference returns for it, whatever that is, with OBTG_MD_OK -- its comparisons with NaN are all false, so a curve
 * with a NaN control point can come back as 1, "no collision"; others walk to cnt = 100 and return -1 (curve form) or 0
 * (polygon form).  A call that holds a non-finite coordinate runs the 3-D gjkNew machine even when every z is +0: the
 * reference's 0 * inf and 0 * nan are NaN, terms the planar machine does not form. */
int obtg_coll_check(obtg_ctx*, const double* curves, int n_curves, int K,
                    const int* pair_a, const int* pair_b, int n_pairs,
                    double eps, int max_iter, int md_cap, int max_nodes,
                    double* res, int* info, int* status);
int obtg_coll_check2poly(obtg_ctx*, const double* curves, int n_curves, int K,
                         const double* pts, int n_pts, const int* poly_off, int n_poly,
                         const int* pair_curve, const int* pair_poly, int n_pairs,
                         int max_iter, int md_cap, int max_nodes,
                         double* res, int* info, int* status);

/* ---- true extrema of Bernstein polynomials over [0, 1] ---------------------------------------
 * What Bezier.min / Bezier.max are for (bezier.py:631-667, 727-763; Examples/3D_Plots.py:167-172 calls them) -- NOT the
 * reference's recursion, which splits a child at a parameter outside the child's span (bezier.py:659-661 with 560-561)
 * and returns values below the minimum or does not return.  A stated contract instead, like the `_robust` searches.
 * c[M][K]: M independent rows of K Bernstein coefficients, 1 <= K <= 64 (41 is the separation polynomial of a degree-20
 * curve); K > 64 is OBTG_ERR_ARG.  For the minimum (want_max = 0), with s = max |c_k| of the row and
 * tol = max(eps_abs, eps_rel * s):
 *   val[M]      the polynomial's value at t_star in [0, 1], as de Casteljau subdivision at 1/2 gives it in binary64;
 *   bound[M]    a lower bound of the polynomial on [0, 1]: the smallest coefficient over the sub-curves the search kept.
 *               bound <= min p <= val up to rounding, and with status OBTG_MD_OK val - bound <= tol;
 *   nodes[M]    sub-curves examined (the row itself is 1).  If the row's smallest coefficient is its first or last one,
 *               val IS that coefficient (same bits), t_star is 0 or 1 and nodes is 1;
 *   status[M]   OBTG_MD_OK; OBTG_MD_NODE_CAP: max_nodes sub-curves examined without reaching tol; OBTG_MD_DEPTH_CAP: more
 *               than 32 sub-curves waiting at once (the search is depth-first, so this is a depth of more than 32
 *               bisections: only a tol below the rounding of the row, tol = 0 included, gets there).  val / bound are then
 *               still a valid bracket, the best of both so far.
 * want_max = 1 is, bit for bit, the negated result of the minimum of the negated row (bound is then an upper bound).
 * A row with a non-finite coefficient: val, t_star, bound NaN, nodes 0, status OBTG_MD_OK.
 * The search is depth-first bisection at 1/2 (every split a pair of averages per level).  A row's result depends on its
 * coefficients alone: not on M, the other rows, its position or the launch; host and _dev entry give the same bits.
 * t_star, bound, nodes are nullable (and status in the _dev form). */
int obtg_bern_extrema(obtg_ctx*, const double* c /*[M][K]*/, int M, int K, int want_max,
                      double eps_rel, double eps_abs, int max_nodes,
                      double* val /*[M]*/, double* t_star /*[M], nullable*/, double* bound /*[M], nullable*/,
                      int* nodes /*[M], nullable*/, int* status /*[M]*/);
int obtg_bern_extrema_dev(obtg_ctx*, const double* d_c, int M, int K, int want_max, double eps_rel, double eps_abs,
                          int max_nodes, double* d_val, double* d_t_star, double* d_bound, int* d_nodes, int* d_status);
/* The tight continuous-time separation: for every row b and every pair of the context's N+M objects, in the order of
 * obtg_temporal_sep, the MINIMUM over t in [0, 1] of ((v_i - v_j).normSquare())(t) - max_sep^2 (optimization.py:311-346
 * bounds this polynomial from below by its control points; bezier.py:631-667 is the reference's sketch of the minimum).
 * normSquare's (d/2) factor and Python's max_sep**2 are kept: the value is on the scale of every other separation row.
 * DEG_ELEV does not enter -- elevation does not change the polynomial -- so the context's R is not read.  The 2n+1
 * coefficients are formed by the device definition of obtg_temporal_sep's rows at R = 0, so out equals
 * obtg_bern_extrema(eps_abs = 0) of those rows bit for bit, and a pair whose smallest coefficient is an end coefficient
 * gives the bits of obtg_temporal_sep_min at R = 0 (a row with a non-finite coefficient: NaN in both).  out[B][P], t_star[B][P] (where the minimum is taken), status[B][P]
 * as above.  Degrees with a specialised kernel (obtg_fast_kernels & 1) form the coefficients in registers: nothing but Y
 * is read and 8 to 20 bytes per pair are written; other degrees up to 31 go through a workspace of obtg_temporal_sep's
 * R = 0 rows (two launches; the context's DEG_ELEV and tables are not touched); beyond: OBTG_ERR_UNSUPPORTED.
 * _dev: dY may be NULL inside an obtg_fd_view (the batch is then written once per view). */
int obtg_temporal_sep_true_min(obtg_ctx*, const double* Y, int B, double max_sep, double eps_rel, int max_nodes,
                               double* out /*[B][P]*/, double* t_star /*[B][P], nullable*/, int* status /*[B][P], nullable*/);
int obtg_temporal_sep_true_min_dev(obtg_ctx*, const double* dY, int B, double max_sep, double eps_rel, int max_nodes,
                                   double* d_out, double* d_t_star, int* d_status);
/* obtg_temporal_sep_true_min with its envelope (Danskin) Jacobian.  out, t_star, status are, bit for bit, those of
 * obtg_temporal_sep_true_min with the same arguments: the search is the same.  jac[B][P][d][n+1] (d = dim, n = deg) is the
 * partial derivative of the pair's polynomial p -- the one that call minimises, normSquare's (d/2) factor included -- taken
 * AT THE RETURNED t_star with respect to the control points Y[a*d + c][i] of the pair's first object a:
 *     jac[c][i] = d * B_i^n(t_star) * Delta_c(t_star),   Delta = v_a - v_b,
 * which is sum_k B_k^2n(t_star) J_k over obtg_temporal_sep_jac's R = 0 blocks J_k.  The conventions are that entry point's:
 * the second object's block is the exact negation and is not stored, a point obstacle has no variable, a pair of two
 * obstacles is all zeros.  For g(Y) = min_t p(t; Y) this is dg/dY wherever the minimiser is unique (the envelope theorem);
 * where two minimisers tie it is one element of the subdifferential.  t_star is the search's dyadic point with
 * p(t_star) - min p <= tol, not a polished root of p': at a smooth interior minimum |t_star - t_min| is of the order
 * sqrt(tol / p''), and the block differs from the one at t_min by that times the mixed second derivative of p.
 * t_star = 0 or 1 leaves column 0 or n alone non-zero (the others are exact zeros).  A row with a non-finite coefficient gets a
 * NaN block, like val (status OBTG_MD_OK).  With a status other than OBTG_MD_OK the block is still the derivative at the
 * returned t_star.
 * B_i^n(t_star) comes from the de Casteljau recurrence on the basis, Delta_c(t_star) from those weights in index order, every
 * multiply-add an explicit fma (csrc/bern_device.h envelope_block): a block depends on the pair's control points and t_star
 * alone -- not on B, the row's position, the entry point (host and _dev: same bits) or the kernel form.  Kernel form: shapes
 * with a specialised kernel (obtg_fast_kernels & 1) form the blocks at the end of the search launch -- nothing but Y is read,
 * one launch; other degrees up to 31 run the value path and then one launch that forms the blocks from Y and t_star (a context
 * created while the environment holds OBTG_TRUE_MIN_JAC_FUSED=0 does so on every shape: same bits); beyond:
 * OBTG_ERR_UNSUPPORTED.  t_star and status are nullable; _dev: dY may be NULL inside an obtg_fd_view. */
int obtg_temporal_sep_true_min_jac(obtg_ctx*, const double* Y, int B, double max_sep, double eps_rel, int max_nodes,
                                   double* out /*[B][P]*/, double* t_star /*[B][P], nullable*/, int* status /*[B][P], nullable*/,
                                   double* jac /*[B][P][d][n+1]*/);
int obtg_temporal_sep_true_min_jac_dev(obtg_ctx*, const double* dY, int B, double max_sep, double eps_rel, int max_nodes,
                                       double* d_out, double* d_t_star, int* d_status, double* d_jac);
/* The tight continuous-time speed bound: for every row b and vehicle v the MINIMUM over t in [0, 1] of
 *     q(t) = sign * (v.diff().normSquare())(t) + offset,   (sign, offset) = (-1, +bound^2) for is_max, (+1, -bound^2) otherwise
 * (optimization.py:349-422 bounds q from below by its elevated control points): feasible iff >= 0 for either bound; for is_max
 * it is bound^2 - max over t of (d/2)|dv/dt|^2.  normSquare's (d/2) factor and Python's bound**2 are kept.  DEG_ELEV does not
 * enter and the context's R is not read.  The 2n+1 coefficients are the bits of obtg_speed's rows on a context with
 * DEG_ELEV = 0 (diff with its trailing elev(1), the product, fma(sign, c, offset)), so out, t_star, status are the bits of
 * obtg_bern_extrema(eps_abs = 0, want_max = 0) on those rows: out[B][N], t_star[B][N], status[B][N] as there.  An end
 * coefficient that is the row's smallest is returned as is (t_star 0 or 1).  A row with a non-finite coefficient: val and
 * t_star NaN, status OBTG_MD_OK.  tf <= 0 is the caller's business, as in obtg_speed.  Degrees with a specialised kernel
 * (obtg_fast_kernels & 1) form the coefficients in registers, one launch; other degrees up to 31 go through a workspace of
 * obtg_speed's R = 0 rows (two launches; the context's DEG_ELEV and tables are not touched); above 31: OBTG_ERR_UNSUPPORTED.
 * t_star and status are nullable.  _dev: dY may be NULL inside an obtg_fd_view (the batch is then written once per view);
 * d_tf is device memory, [B]. */
int obtg_speed_true_min(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double bound, int is_max, double eps_rel,
                        int max_nodes, double* out /*[B][N]*/, double* t_star /*[B][N], nullable*/, int* status /*[B][N], nullable*/);
int obtg_speed_true_min_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, int is_max, double eps_rel,
                            int max_nodes, double* d_out, double* d_t_star, int* d_status);
/* obtg_speed_true_min with its envelope (Danskin) Jacobian.  out, t_star, status are, bit for bit, those of
 * obtg_speed_true_min with the same arguments.  With n = deg, d = dim, T = tf[b], w = B^(n-1)(t_star) and the velocity
 * c'_c(t_star) = (n/T) sum_i w_i (P_c,i+1 - P_c,i) of vehicle v:
 *     jac[B][N][d][n+1]:  jac[c][i] = sign * d * c'_c(t_star) * (n/T) * (w_(i-1) - w_i),   w_(-1) = w_n = 0
 *     jac_tf[B][N] (nullable):  -2 (q(t_star) - offset) / T, q(t_star) - offset = sign (d/2) |c'(t_star)|^2 from the same w
 * -- the partial derivatives of q AT THE RETURNED t_star with respect to the vehicle's own control points Y[v*d + c][i] and to
 * tf at fixed control points; the derivative of min_t q wherever the minimiser is unique (obtg_temporal_sep_true_min_jac says
 * what it is otherwise, and how close t_star is to the minimiser).  t_star = 0 leaves columns 0 and 1 as the only non-zero
 * ones, t_star = 1 columns n-1 and n.  A row with a non-finite coefficient gets a NaN block and a NaN jac_tf (status
 * OBTG_MD_OK); with another status the block is still the derivative at the returned t_star.  Every multiply-add is an explicit
 * fma (csrc/bern_device.h speed_envelope_block): a block depends on the vehicle's control points, tf and t_star alone, not on
 * the entry point (host and _dev: same bits) or the kernel form -- in the search launch where the shape has a specialised
 * kernel, else (and on every shape in a context created under OBTG_TRUE_MIN_JAC_FUSED=0) the value path and one more launch
 * from Y, tf and t_star.  Degrees above 31: OBTG_ERR_UNSUPPORTED.  _dev: dY may be NULL inside an obtg_fd_view. */
int obtg_speed_true_min_jac(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double bound, int is_max, double eps_rel,
                            int max_nodes, double* out /*[B][N]*/, double* t_star /*[B][N], nullable*/, int* status /*[B][N], nullable*/,
                            double* jac /*[B][N][d][n+1]*/, double* jac_tf /*[B][N], nullable*/);
int obtg_speed_true_min_jac_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, int is_max, double eps_rel,
                                int max_nodes, double* d_out, double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf);
/* The tight continuous-time angular-rate bound (dim 2).  With x' = x.diff(), x'' = x'.diff() (each the derivative followed by
 * elev(1), degree n: optimization.py:543-574), den = x'^2 + y'^2 and num = y'' x' - x'' y' -- the weights and the numerator
 * of _angularRate's rational curve, degree 2n -- |angular rate| <= max_rate for all t is, because den >= 0, the pair
 *     p_+(t) = max_rate den(t) - num(t) >= 0  (side 0, left turns),     p_-(t) = max_rate den(t) + num(t) >= 0  (side 1, right turns).
 * NOTE THE UNITS: these rows are max_rate * speed^2 -+ (turn rate * speed^2), NOT obtg_ang_rate's maxAngRate^2 - omega^2; a
 * vehicle is feasible iff both are >= 0, 2 rows per vehicle whatever DEG_ELEV is (it does not enter; the context's R is not
 * read).  They are meant for trajectories that do not stop: where the speed vanishes both polynomials vanish with it.
 * obtg_ang_rate_poly: the Bernstein coefficients of both sides, out[B][N][2][2n+1],
 *     p_k = fma(max_rate, den_k, -+num_k),  den_k / num_k the equal-degree products above (csrc/bern_device.h ang_row_coeff
 *     states every operation; they are not the bits of obtg_ang_rate's intermediate products).
 * obtg_ang_rate_true_min: out[B][N][2] = min over t in [0, 1] of p_+ / p_-, t_star and status as in obtg_speed_true_min; by
 *     DEFINITION the bits of obtg_bern_extrema(eps_abs = 0, want_max = 0) on obtg_ang_rate_poly's rows.  A row with a
 *     non-finite coefficient: val and t_star NaN, status OBTG_MD_OK.  A vehicle at rest: all coefficients zero, val +0.0.
 * obtg_ang_rate_true_min_jac: the same out, t_star, status bit for bit, and the envelope (Danskin) block of every row at its
 *     t_star.  With T = tf[b], w = B^(n-1)(t_star), u = B^(n-2)(t_star), entries out of range 0, sigma = +1 / -1 for side 0 / 1,
 *         A_i = (n/T)(w_(i-1) - w_i),    C_i = (n(n-1)/T^2)(u_(i-2) - 2 u_(i-1) + u_i),
 *         jac[B][N][2][2][n+1]:  jac[side][0][i] = 2 max_rate x' A_i - sigma (y'' A_i - y' C_i)
 *                                jac[side][1][i] = 2 max_rate y' A_i - sigma (x' C_i - x'' A_i)
 *         jac_tf[B][N][2] (nullable):  (-2 max_rate den + 3 sigma num) / T,
 *     x', y', x'', y'', den, num at t_star from the same w and u (csrc/bern_device.h ang_envelope_block, every multiply-add an
 *     explicit fma: host and _dev, fused and two-launch forms give the same bits).  t_star = 0 / 1 leave the first / last three
 *     columns as the only non-zero ones.  A row with a non-finite coefficient gets a NaN block and a NaN jac_tf (status
 *     OBTG_MD_OK); with another status the block is still the derivative at the returned t_star; a vehicle at rest has a zero
 *     block.
 * Checks as in obtg_speed_true_min[_jac] (t_star, status, jac_tf nullable; B == 0 is OBTG_OK); dim != 2: OBTG_ERR_ARG, as
 * obtg_ang_rate; degrees above 31: OBTG_ERR_UNSUPPORTED.  Degrees 3, 5, 7, 8, 10, 15, 20 form the coefficients in registers, one
 * launch (with the blocks too, unless the context was created under OBTG_TRUE_MIN_JAC_FUSED=0: then one more launch); other
 * degrees from 1 to 31 go through a workspace of obtg_ang_rate_poly's rows (two launches, three with blocks).  Every launch
 * is timed under OBTG_K_ANG_RATE.  tf <= 0 is the caller's business.  _dev: dY may be NULL inside an obtg_fd_view; d_tf is
 * device memory, [B]. */
int obtg_ang_rate_poly(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double max_rate, double* out /*[B][N][2][2n+1]*/);
int obtg_ang_rate_poly_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double max_rate, double* d_out);
int obtg_ang_rate_true_min(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double max_rate, double eps_rel, int max_nodes,
                           double* out /*[B][N][2]*/, double* t_star /*[B][N][2], nullable*/, int* status /*[B][N][2], nullable*/);
int obtg_ang_rate_true_min_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double max_rate, double eps_rel,
                               int max_nodes, double* d_out, double* d_t_star, int* d_status);
int obtg_ang_rate_true_min_jac(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double max_rate, double eps_rel,
                               int max_nodes, double* out /*[B][N][2]*/, double* t_star /*nullable*/, int* status /*nullable*/,
                               double* jac /*[B][N][2][2][n+1]*/, double* jac_tf /*[B][N][2], nullable*/);
int obtg_ang_rate_true_min_jac_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double max_rate, double eps_rel,
                                   int max_nodes, double* d_out, double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf);
/* The curvature bound (dim 2): |kappa| <= max_curv on the whole path, a minimum turning radius of 1 / max_curv.  With x', x''
 * (each the derivative followed by elev(1), degree n) formed on T = 1 -- curvature does not depend on the time span, so no
 * entry point takes tf -- den = x'^2 + y'^2 and num = y'' x' - x'' y' are the 2n+1 Bernstein coefficients den_k, num_k that
 * obtg_ang_rate_poly's rows are made of at tf = 1 (csrc/bern_device.h curvature_row_coeff: ang_row_coeff's fma sequence and
 * weights), and signed curvature is kappa(t) = num(t) / (den(t) sqrt(den(t))), left turns positive.  Two rows per vehicle,
 * sigma = +1 (side 0, left turns) and sigma = -1 (side 1, right turns):
 *     m_sigma = max over t in [0, 1] of max(0, sigma kappa(t)),      row_sigma = max_curv - m_sigma,
 * a vehicle respects the bound iff both rows are >= 0.  The clamp at 0 is deliberate: a vehicle that never turns right has
 * side 1 equal to max_curv exactly.  The family is meant for trajectories that do not stop.
 * obtg_curvature_poly: out[B][N][2][2n+1], num_k then den_k.
 * obtg_curvature_true_min: out[B][N][2] = row_sigma, t_star[B][N][2], status[B][N][2].  kappa is not a polynomial, so the search
 *     is not obtg_bern_extrema's: a depth-first bisection at 1/2 over num and den at once (each de Casteljau level the same
 *     pair of averages 0.5 a + 0.5 b on both), one wave per row.
 *     Evaluation at a point: with num and den the end coefficients of a sub-curve, sigma kappa = (sigma num) / (den sqrt(den)) in
 *     binary64; a point with den <= 0, or whose quotient is not finite, offers no value.
 *     Incumbent U: starts at max(0, sigma kappa(0), sigma kappa(1)); every bisection midpoint updates it.
 *     Upper bound of a sub-curve with coefficients (sigma num_k, den_k): d0 = 0.5 (min den_k + max den_k),
 *     g_k = fma(1.5 sqrt(d0), den_k, -0.5 (d0 sqrt(d0))) -- the tangent of the convex den^(3/2) at d0, so
 *     den(t)^(3/2) >= sum g_k B_k(t) --; lambda g_k - num_k >= 0 for EVERY k gives sigma kappa <= lambda, and a coefficient
 *     with num_k <= 0 meets it for every lambda >= 0 only if its g_k >= 0.  So: 0 if no num_k > 0; else +inf if min den_k <= 0
 *     or g at min den_k is <= 0 (that is max den_k >= 5 min den_k: the speed varies too much across the sub-curve for this
 *     tangent, and it is split further); else the largest num_k / g_k over num_k > 0.  Its excess over the sub-curve's true
 *     maximum falls with the square of the width.
 *     A sub-curve is closed when bound - U <= tol, tol = eps_rel * max(max_curv, U) with U the incumbent at the time of the
 *     test; of two open halves the one with the larger bound is followed, the other waits.
 *     With OBTG_MD_OK: m_sigma is sigma kappa(t_star) as evaluated above, t_star a bisection point in [0, 1] (0 when the value
 *     is the clamp's 0), and nothing on [0, 1] exceeds m_sigma + tol up to the rounding of the bound.  OBTG_MD_NODE_CAP:
 *     max_nodes sub-curves examined; OBTG_MD_DEPTH_CAP: more than 32 sub-curves waiting; m_sigma is then still a value met
 *     (or the clamp's 0).  Where den vanishes with num != 0 (a stop, a cusp) the bound stays infinite and the search ends
 *     on a cap, never in a spin.  num == 0 identically (degree 1, a straight path, a vehicle at rest with every coefficient
 *     zero): m_sigma = 0, t_star = 0, OBTG_MD_OK.  A row with a non-finite coefficient: out and t_star NaN, OBTG_MD_OK.
 *     A row's result depends on its control points, max_curv, eps_rel and max_nodes alone: not on B, its position, the
 *     launch form, or host versus _dev.
 * obtg_curvature_true_min_jac: the same out, t_star, status bit for bit, and jac[B][N][2][2][n+1], the derivative of row_sigma
 *     with respect to the vehicle's own control points at t_star.  With w = B^(n-1)(t_star), u = B^(n-2)(t_star),
 *     A_i = n (w_(i-1) - w_i), C_i = n (n-1) (u_(i-2) - 2 u_(i-1) + u_i)  (obtg_ang_rate_true_min_jac's on T = 1):
 *         jac[side][0][i] = -sigma [ (y'' A_i - y' C_i) / den^(3/2) - 3 num x' A_i / den^(5/2) ]
 *         jac[side][1][i] = -sigma [ (x' C_i - x'' A_i) / den^(3/2) - 3 num y' A_i / den^(5/2) ]
 *     x', y', x'', y'', den, num at t_star from the same w and u (csrc/bern_device.h curvature_envelope_block states every
 *     operation; every multiply-add an explicit fma: host and _dev, fused and two-launch forms give the same bits).  The block
 *     is zero where the returned row IS max_curv (m_sigma = 0: the clamp, num == 0), NaN for a NaN row; with a cap status it
 *     is still the derivative at the returned t_star.  There is no jac_tf: it is identically 0.
 * Checks: dim != 2: OBTG_ERR_ARG; degrees above 31: OBTG_ERR_UNSUPPORTED; t_star and status nullable; B == 0 is OBTG_OK.
 * Degrees 3, 5, 7, 8, 10, 15, 20 form the coefficients in registers, one launch (with the blocks too, unless the context was
 * created under OBTG_TRUE_MIN_JAC_FUSED=0: then one more launch); other degrees from 1 to 31 go through a workspace of
 * obtg_curvature_poly's rows (two launches, three with blocks).  Every launch is timed under OBTG_K_ANG_RATE.  _dev: dY may be
 * NULL inside an obtg_fd_view. */
int obtg_curvature_poly(obtg_ctx*, const double* Y, int B, double* out /*[B][N][2][2n+1]*/);
int obtg_curvature_poly_dev(obtg_ctx*, const double* dY, int B, double* d_out);
int obtg_curvature_true_min(obtg_ctx*, const double* Y, int B, double max_curv, double eps_rel, int max_nodes,
                            double* out /*[B][N][2]*/, double* t_star /*[B][N][2], nullable*/, int* status /*[B][N][2], nullable*/);
int obtg_curvature_true_min_dev(obtg_ctx*, const double* dY, int B, double max_curv, double eps_rel, int max_nodes, double* d_out,
                                double* d_t_star, int* d_status);
int obtg_curvature_true_min_jac(obtg_ctx*, const double* Y, int B, double max_curv, double eps_rel, int max_nodes,
                                double* out /*[B][N][2]*/, double* t_star /*nullable*/, int* status /*nullable*/,
                                double* jac /*[B][N][2][2][n+1]*/);
int obtg_curvature_true_min_jac_dev(obtg_ctx*, const double* dY, int B, double max_curv, double eps_rel, int max_nodes,
                                    double* d_out, double* d_t_star, int* d_status, double* d_jac);
/* The curvature range of M free planar curves c[M][2][K] (x row, y row; 2 <= K <= 32 control points, whatever the context's
 * shape is; K > 32: OBTG_ERR_UNSUPPORTED): the search above with max_curv = 0 (tol = eps_rel |U|) and no clamp on the sign
 * of what is reported -- the incumbent starts from the end values alone, and a sub-curve with no num_k > 0 is bounded by the
 * chord of den^(3/2) over [min den_k, max den_k] (the largest num_k / h_k; 0 if min den_k <= 0):
 *     k_max[M] = max kappa at t_max[M],    k_min[M] = -max(-kappa) at t_min[M],    status[M][2] (side 0: k_max, side 1: k_min).
 * num == 0 identically: 0 at t = 0.  A curve with a non-finite coefficient: NaN, OBTG_MD_OK.  Ends with den <= 0 (a curve that
 * starts or stops at rest) offer no value: the search goes on to interior points with tol = 0 until one does, and where none
 * ever does it ends on a cap with NaN.
 * status is nullable.  M == 0 is OBTG_OK.  Two launches, timed under OBTG_K_ANG_RATE. */
int obtg_bern_curvature(obtg_ctx*, const double* c /*[M][2][K]*/, int M, int K, double eps_rel, int max_nodes,
                        double* k_min /*[M]*/, double* t_min /*[M]*/, double* k_max /*[M]*/, double* t_max /*[M]*/,
                        int* status /*[M][2], nullable*/);
int obtg_bern_curvature_dev(obtg_ctx*, const double* d_c, int M, int K, double eps_rel, int max_nodes, double* d_k_min,
                            double* d_t_min, double* d_k_max, double* d_t_max, int* d_status);
/* The space-curvature bound (dim 3): kappa <= max_curv on the whole path of a vehicle in space, a minimum turning radius of
 * 1 / max_curv.  With c' and c'' (each the derivative followed by elev(1), degree n) formed on T = 1 -- no entry point takes
 * tf --, w = c' x c'' and den = |c'|^2 are four polynomials of 2n+1 Bernstein coefficients: the components of w are
 * obtg_curvature_poly's num on the coordinate pairs (y, z), (z, x), (x, y) (csrc/bern_device.h curvature_row_coeff), den_k is
 * the sum over j in index order of fma(x'_j, x'_(k-j), .), fma(y'_j, y'_(k-j), .), fma(z'_j, z'_(k-j), .) with the same
 * weights (space_curvature_row_coeff).  kappa(t) = |w(t)| / (den(t) sqrt(den(t))) >= 0: the norm of a vector of polynomials,
 * not a polynomial and without a sign.  One row per vehicle, no sides, no clamp:
 *     m = max over t in [0, 1] of kappa(t),      row = max_curv - m,
 * a vehicle respects the bound iff its row is >= 0.  The family is meant for trajectories that do not stop.
 * obtg_space_curvature_poly: out[B][N][4][2n+1]: wx_k, wy_k, wz_k, den_k.
 * obtg_space_curvature_true_min: out[B][N] = row, t_star[B][N], status[B][N].  A depth-first bisection at 1/2 over the four
 *     polynomials at once (each de Casteljau level the same average 0.5 a + 0.5 b on all four), one wave per row.
 *     Evaluation at a point: with (wx, wy, wz, den) the end coefficients of a sub-curve,
 *         nu = sqrt(fma(wz, wz, fma(wy, wy, wx wx))),    kappa = nu / (den sqrt(den))
 *     in binary64, in this order; a point with den <= 0, or whose value is not finite, offers no value.
 *     Incumbent U: starts at 0 (at t = 0); kappa(0), kappa(1) and every bisection midpoint update it.
 *     Upper bound of a sub-curve: nu_k from (wx_k, wy_k, wz_k) as above, one per coefficient -- the norm is convex, so
 *     |w(t)| <= sum nu_k B_k(t) --; d0 = 0.5 (min den_k + max den_k), g_k = fma(1.5 sqrt(d0), den_k, -0.5 (d0 sqrt(d0))), the
 *     tangent of the convex den^(3/2) at d0, so den(t)^(3/2) >= sum g_k B_k(t); lambda g_k - nu_k >= 0 for EVERY k gives
 *     kappa <= lambda.  So: 0 if every nu_k == 0; else +inf if min den_k <= 0 or g at min den_k is <= 0 (the speed varies too
 *     much across the sub-curve for this tangent, and it is split further); else the largest nu_k / g_k.  Its excess over
 *     the sub-curve's true maximum falls with the square of the width.
 *     A sub-curve is closed when bound - U <= tol, tol = eps_rel * max(max_curv, U) with U the incumbent at the time of the
 *     test; of two open halves the one with the larger bound is followed, the other waits.
 *     With OBTG_MD_OK: m is kappa(t_star) as evaluated above, t_star a bisection point in [0, 1], and nothing on [0, 1]
 *     exceeds m + tol up to the rounding of the bound.  OBTG_MD_NODE_CAP: max_nodes sub-curves examined; OBTG_MD_DEPTH_CAP:
 *     more than 32 sub-curves waiting; m is then still a value met (or 0).  Where den vanishes with w != 0 (a stop, a
 *     cusp) the bound stays infinite and the search ends on a cap, never in a spin.  w == 0 identically (degree 1, a
 *     straight path, a vehicle at rest): row = max_curv exactly, t_star = 0, OBTG_MD_OK from the first step.  A row with a
 *     non-finite coefficient: out and t_star NaN, OBTG_MD_OK.
 *     A row's result depends on its control points, max_curv, eps_rel and max_nodes alone: not on B, its position, the
 *     launch form, or host versus _dev.
 * obtg_space_curvature_true_min_jac: the same out, t_star, status bit for bit, and jac[B][N][3][n+1], the derivative of the row
 *     with respect to the vehicle's own control points at t_star.  With A_i, C_i obtg_curvature_true_min_jac's, v = c'(t_star),
 *     a = c''(t_star), w = v x a, wh = w / |w|, den = |v|^2:
 *         jac[d][i] = -[ (A_i (a x wh)_d + C_i (wh x v)_d) / den^(3/2) - 3 |w| v_d A_i / den^(5/2) ]
 *     (csrc/bern_device.h space_curvature_envelope_block states every operation; every multiply-add an explicit fma: host and
 *     _dev, fused and two-launch forms give the same bits).  With wh = e_z this is obtg_curvature_true_min_jac's block.  The
 *     block is zero where the returned row IS max_curv, NaN for a NaN row; with a cap status it is still the derivative at
 *     the returned t_star.  There is no jac_tf: it is identically 0.
 * Checks: a context whose dim is not 3, degrees above 31: OBTG_ERR_UNSUPPORTED; t_star and status nullable; B == 0 is OBTG_OK.
 * Control-point counts 4, 6, 8, 9, 11, 16 form the coefficients in registers, one launch (with the blocks too, unless the
 * context was created under OBTG_TRUE_MIN_JAC_FUSED=0: then one more launch); other degrees from 1 to 31 go through a
 * workspace of obtg_space_curvature_poly's rows (two launches, three with blocks).  Every launch is timed under
 * OBTG_K_ANG_RATE.  _dev: dY may be NULL inside an obtg_fd_view. */
int obtg_space_curvature_poly(obtg_ctx*, const double* Y, int B, double* out /*[B][N][4][2n+1]*/);
int obtg_space_curvature_poly_dev(obtg_ctx*, const double* dY, int B, double* d_out);
int obtg_space_curvature_true_min(obtg_ctx*, const double* Y, int B, double max_curv, double eps_rel, int max_nodes,
                                  double* out /*[B][N]*/, double* t_star /*[B][N], nullable*/, int* status /*[B][N], nullable*/);
int obtg_space_curvature_true_min_dev(obtg_ctx*, const double* dY, int B, double max_curv, double eps_rel, int max_nodes,
                                      double* d_out, double* d_t_star, int* d_status);
int obtg_space_curvature_true_min_jac(obtg_ctx*, const double* Y, int B, double max_curv, double eps_rel, int max_nodes,
                                      double* out /*[B][N]*/, double* t_star /*nullable*/, int* status /*nullable*/,
                                      double* jac /*[B][N][3][n+1]*/);
int obtg_space_curvature_true_min_jac_dev(obtg_ctx*, const double* dY, int B, double max_curv, double eps_rel, int max_nodes,
                                          double* d_out, double* d_t_star, int* d_status, double* d_jac);
/* The largest curvature of M free space curves c[M][3][K] (x, y, z rows; 2 <= K <= 32 control points, whatever the context's
 * shape and dimension are; K > 32: OBTG_ERR_UNSUPPORTED): the search above with max_curv = 0 (tol = eps_rel U):
 *     k_max[M] = max kappa at t_max[M],    status[M].
 * w == 0 identically: 0 at t = 0.  A curve with a non-finite coefficient: NaN, OBTG_MD_OK.  Points with den <= 0 offer no
 * value; a curve on which none does ends on a cap with k_max = 0.
 * status is nullable.  M == 0 is OBTG_OK.  Two launches, timed under OBTG_K_ANG_RATE. */
int obtg_bern_space_curvature(obtg_ctx*, const double* c /*[M][3][K]*/, int M, int K, double eps_rel, int max_nodes,
                              double* k_max /*[M]*/, double* t_max /*[M]*/, int* status /*[M], nullable*/);
int obtg_bern_space_curvature_dev(obtg_ctx*, const double* d_c, int M, int K, double eps_rel, int max_nodes, double* d_k_max,
                                  double* d_t_max, int* d_status);

/* ---- keep-in regions: every listed vehicle stays inside its half-spaces, in 2-D and 3-D ----
 * A region is F half-spaces a_f . p <= b_f, H[F][d+1] = (a_f[0 .. d-1], b_f); a is not normalised (with |a| = 1 a row is a
 * distance).  An item is a (vehicle, face) pair of the list VF[P][2]; vehicles may have different faces, or none.  For vehicle v
 * with control points P[c][i] (c < d, i <= n):
 *     g(t) = b_f - a_f . c_v(t),    Bernstein coefficient i:  g_i = b_f - sum_c a_f[c] P[c][i]     (degree n; feasible iff g >= 0)
 * formed as fma(-a[0], P[0][i], b), then fma(-a[c], P[c][i], .) for c = 1 .. d-1 (csrc/bern_device.h keep_in_coeff) in every
 * kernel form.  Neither tf nor a time span enters: nothing here takes tf and there is no jac_tf.
 * obtg_ctx_set_keep_in: copies H and VF to the context (P = 0 clears the region).  OBTG_ERR_ARG for a vehicle index outside
 *     0 .. N-1, a face index outside 0 .. F-1, a context whose d is not 2 or 3, F < 1 or a null table with P > 0.
 * obtg_len_keep_in: P (n+R+1).
 * obtg_keep_in: out[B][P][n+R+1], the R = 0 coefficients elevated by the context's DEG_ELEV -- formed first, then elevated once
 *     per row: the bits of obtg_bern_elev(R) applied to the R = 0 row (R = 0: the coefficients themselves; a -0 is written +0).
 *     Any degree up to 31, above that OBTG_ERR_UNSUPPORTED.  These are exact linear constraints on the control points.
 * obtg_keep_in_true_min: out[B][P] = min over t in [0, 1] of g, the true margin.  DEG_ELEV does not enter.  out, t_star and
 *     status are the bits of obtg_bern_extrema(eps_abs = 0, want_max = 0) on obtg_keep_in's rows of a DEG_ELEV = 0 context.  An
 *     end coefficient that is the row's smallest is returned as is (t_star 0 or 1).  A row with a non-finite coefficient: val
 *     and t_star NaN, status OBTG_MD_OK.  Degrees with a specialised kernel (obtg_fast_kernels & 1) form the coefficients in
 *     registers, one launch; other degrees up to 31 go through a workspace of the R = 0 rows (two launches); above 31:
 *     OBTG_ERR_UNSUPPORTED.  t_star and status are nullable.
 * obtg_keep_in_true_min_jac: out, t_star, status are the bits of the value call with the same arguments, plus the envelope
 *     block of every row at its t_star with respect to the control points of the item's own vehicle:
 *         jac[B][P][d][n+1]:  jac[c][i] = -a_f[c] B_i^n(t_star)
 *     (csrc/bern_device.h keep_in_envelope_block; g is linear in the control points, so the block does not read them).  An end
 *     minimiser (t_star 0 or 1) leaves column 0 or n as the only non-zero one; a row with a non-finite coefficient gets a NaN
 *     block (status OBTG_MD_OK).  Every specialised count has a fused value-and-blocks kernel (one launch; all build without
 *     scratch); a context created under OBTG_TRUE_MIN_JAC_FUSED=0 forms the blocks in one more launch, as other degrees up to 31
 *     do after their value path (three launches).
 * Host and _dev calls give the same bits.  No region set, or a context whose d is not 2 or 3: OBTG_ERR_ARG before any launch.
 * Every launch is timed under OBTG_K_SPEED.  _dev: dY is device memory [B][N d][n+1]; dY = NULL inside an obtg_fd_view is not
 * built for this family and answers OBTG_ERR_ARG.  Not part of obtg_constraint_sweep_dev or of the structured step. */
int obtg_ctx_set_keep_in(obtg_ctx*, const double* H /*[F][d+1]*/, int F, const int* VF /*[P][2]*/, int P);
int obtg_len_keep_in(const obtg_ctx*);      /* P * (n+R+1)         */
int obtg_keep_in(obtg_ctx*, const double* Y, int B, double* out /*[B][P][n+R+1]*/);
int obtg_keep_in_dev(obtg_ctx*, const double* dY, int B, double* d_out);
int obtg_keep_in_true_min(obtg_ctx*, const double* Y, int B, double eps_rel, int max_nodes,
                          double* out /*[B][P]*/, double* t_star /*[B][P], nullable*/, int* status /*[B][P], nullable*/);
int obtg_keep_in_true_min_dev(obtg_ctx*, const double* dY, int B, double eps_rel, int max_nodes, double* d_out, double* d_t_star,
                              int* d_status);
int obtg_keep_in_true_min_jac(obtg_ctx*, const double* Y, int B, double eps_rel, int max_nodes,
                              double* out /*[B][P]*/, double* t_star /*[B][P], nullable*/, int* status /*[B][P], nullable*/,
                              double* jac /*[B][P][d][n+1]*/);
int obtg_keep_in_true_min_jac_dev(obtg_ctx*, const double* dY, int B, double eps_rel, int max_nodes, double* d_out, double* d_t_star,
                                  int* d_status, double* d_jac);

/* ---- proximity rows: a vehicle comes within, or stays within, a Euclidean radius of a point or of another vehicle ----
 * An item is (a, b, kind) of items[P][3] with (rho, tau0, tau1) of params[P][3]: a is a vehicle, b another vehicle (b < N) or
 * point b - N of points[Q][d], a table the family owns (it is not the context's point obstacles); kind is OBTG_PROX_WITHIN (0)
 * or OBTG_PROX_REACH (1); rho > 0 is a Euclidean radius; 0 <= tau0 < tau1 <= 1 is the window of the normalised parameter in
 * which the extremum is taken (a window in tau does not depend on tf: nothing here takes tf and there is no jac_tf).
 *     g(tau) = (d/2) (rho^2 - |c_a(tau) - c_b(tau)|^2),  tau in [tau0, tau1]       (degree 2n; >= 0 iff the distance is <= rho)
 * -- normSquare's (d/2) factor, as the separation rows carry it, here on rho^2 as well.
 *     OBTG_PROX_WITHIN: the row is the MINIMUM of g over the window: >= 0 iff the pair never leaves range;
 *     OBTG_PROX_REACH:  the row is the MAXIMUM of g over the window: >= 0 iff it comes within rho at some time.
 * Coefficients (csrc/bern_device.h proximity_coeffs): every coordinate row of a, and of b when b is a vehicle, is cut down to
 * the window in the order of obtg_bern_restrict on the span (0, 1) -- the right piece of a split at tau0 when tau0 > 0, then the
 * left piece of a split of THAT piece at (tau1 - tau0) / (1 - tau0) when tau1 < 1, every level (1 - z) p[i] + z p[i+1] in plain
 * double arithmetic (two products, one sum); the full window takes no split -- then the rounded difference, the product of
 * obtg_temporal_sep's R = 0 rows, and g_k = fma(-1, c_k, (0.5 d) (rho rho)).  A point is a constant curve and is not cut.  An item
 * with the full window is therefore fma(-1, ., (0.5 d)(rho rho)) of obtg_temporal_sep's R = 0 row at max_sep = 0 for the same pair.
 * obtg_ctx_set_proximity: copies the three tables to the context (P = 0 clears them).  OBTG_ERR_ARG for a outside 0 .. N-1, b
 *     outside 0 .. N+Q-1, a == b, a kind that is neither, rho that is not finite and > 0, a window that is not
 *     0 <= tau0 < tau1 <= 1 (NaN ends too), a context whose d is not 2 or 3, or a null table that is needed.
 * obtg_len_proximity: P, the rows per batch row.
 * obtg_proximity_poly: out[B][P][2n+1], g's coefficients, un-negated for both kinds.  Degrees with a specialised kernel
 *     (obtg_fast_kernels & 1) form them as the fused kernels do; other degrees up to 31 in the any-degree separation arithmetic
 *     of obtg_temporal_sep on those degrees; above 31: OBTG_ERR_UNSUPPORTED.  DEG_ELEV does not enter anywhere in the family.
 * obtg_proximity_true: val, bound, nodes, status are the bits of obtg_bern_extrema(eps_abs = 0, want_max = kind) on
 *     obtg_proximity_poly's rows -- val is the value ATTAINED at the returned parameter, bound closes the bracket on the other
 *     side (within: bound <= min g <= val; reach: val <= max g <= bound) -- and t_star = fma(t_w, tau1 - tau0, tau0) is the
 *     CURVE's parameter of that call's t, the window's parameter t_w.  A row with a non-finite coefficient: val, t_star and bound
 *     NaN, nodes 0, status OBTG_MD_OK, no search.  Specialised degrees: one launch, the coefficients never reach memory; other
 *     degrees up to 31: the rows into a workspace, then their search (two launches).  Every output but val is nullable.
 * obtg_proximity_true_jac: the same outputs with the same bits, plus the envelope block of every row at its t_star with respect
 *     to the control points of a, evaluated on the UNRESTRICTED control points:
 *         jac[B][P][d][n+1]:  jac[c][i] = -d B_i^n(t_star) (c_a - c_b)_c(t_star)          (both kinds)
 *     -- obtg_temporal_sep_true_min_jac's block with the sign turned, every element its exact negation (csrc/bern_device.h
 *     envelope_block), and its conventions: when b is a vehicle its block is the exact negation and is not stored; a point has no
 *     variable.  A NaN t_star gives a NaN block.  Every specialised count has a fused value-and-blocks kernel (one launch); a
 *     context created under OBTG_TRUE_MIN_JAC_FUSED=0 forms the blocks in one more launch, as other degrees do after their values.
 * Host and _dev calls give the same bits.  No items set, or a context whose d is not 2 or 3: OBTG_ERR_ARG before any launch.
 * Every launch is timed under OBTG_K_TEMPORAL_SEP.  _dev: dY is device memory [B][N d][n+1]; dY = NULL inside an obtg_fd_view is
 * not built for this family and answers OBTG_ERR_ARG.  Not part of obtg_constraint_sweep_dev or of the structured step. */
#define OBTG_PROX_WITHIN 0
#define OBTG_PROX_REACH 1
int obtg_ctx_set_proximity(obtg_ctx*, const int* items /*[P][3]*/, const double* params /*[P][3]*/, const double* points /*[Q][d]*/,
                           int P, int Q);
int obtg_len_proximity(const obtg_ctx*);    /* P                   */
int obtg_proximity_poly(obtg_ctx*, const double* Y, int B, double* out /*[B][P][2n+1]*/);
int obtg_proximity_poly_dev(obtg_ctx*, const double* dY, int B, double* d_out);
int obtg_proximity_true(obtg_ctx*, const double* Y, int B, double eps_rel, int max_nodes, double* val /*[B][P]*/,
                        double* t_star /*[B][P], nullable*/, double* bound /*[B][P], nullable*/, int* nodes /*[B][P], nullable*/,
                        int* status /*[B][P], nullable*/);
int obtg_proximity_true_dev(obtg_ctx*, const double* dY, int B, double eps_rel, int max_nodes, double* d_val, double* d_t_star,
                            double* d_bound, int* d_nodes, int* d_status);
int obtg_proximity_true_jac(obtg_ctx*, const double* Y, int B, double eps_rel, int max_nodes, double* val /*[B][P]*/,
                            double* t_star /*[B][P], nullable*/, double* bound /*[B][P], nullable*/, int* nodes /*[B][P], nullable*/,
                            int* status /*[B][P], nullable*/, double* jac /*[B][P][d][n+1]*/);
int obtg_proximity_true_jac_dev(obtg_ctx*, const double* dY, int B, double eps_rel, int max_nodes, double* d_val, double* d_t_star,
                                double* d_bound, int* d_nodes, int* d_status, double* d_jac);

/* ---- keep-out obstacles: every listed vehicle stays outside convex obstacles, in 2-D and 3-D ----
 * An obstacle is a convex set {p : a_f . p <= b_f, f = 1 .. F_o}: a run of rows (a_f[0 .. d-1], b_f) of H[F][d+1], obstacle o
 * owning rows obs_off[o] .. obs_off[o+1]-1.  a is not normalised (with |a| = 1 the rows are distances).  An item is a (vehicle,
 * obstacle) pair of the list VO[P][2].  For vehicle v with control points P[c][i] (c < d, i <= n) and obstacle o:
 *     g_f(t) = a_f . c_v(t) - b_f      Bernstein coefficient i:  a_f . P_i - b_f, formed as fma(a[0], P[0][i], -b), then
 *                                      fma(a[c], P[c][i], .): the exact negation of obtg_keep_in's coefficient
 *     G(t)   = max over the obstacle's faces of g_f(t)      (> 0 outside; inside: minus the penetration depth)
 *     row    = min over t in [0, 1] of G(t)  -  margin      (feasible iff >= 0)
 * G(t) <= dist(c(t), obstacle) outside -- equal where the nearest feature is a face, smaller near a corner -- so row >= 0
 * implies a true clearance >= margin: the row is CONSERVATIVE near corners.  G is negative inside, so a start that penetrates
 * still has a gradient that pushes out.  Neither tf nor a time span enters.
 * Search (csrc/keepout_kernels.hip), the conventions of obtg_bern_extrema: bisection at 1/2 by de Casteljau on the coordinate
 * rows; a sub-curve's bound is max_f min_i of its face coefficients, exact values of G at its ends and its mid point;
 * s = max |g_f,i| of the root, tol = eps_rel s; the incumbent is replaced on strict decrease only, a child is dropped when
 * incumbent - bound <= tol; depth-first, the smaller bound first; nodes counts sub-curves, the root being 1; OBTG_MD_NODE_CAP
 * when the next split would pass max_nodes, OBTG_MD_DEPTH_CAP at 32 waiting frames, both with a valid bracket [bound, out].  A
 * non-finite control point or face: NaN outputs (face -1, nodes 0), status OBTG_MD_OK.  A root that closes: out is an end
 * value, t_star 0 or 1, nodes 1.
 * Envelope block.  t* the minimiser, f1 = argmax_f g_f(t*) (the first of equals), values and slopes taken at c(t*), c'(t*):
 *   an end minimiser (t* 0 or 1) or a smooth interior minimum: one face, jac[c][i] = a_f1[c] B_i^n(t*);
 *   a kink: a second face f2 is CO-ACTIVE iff  g_f2'(t*) and g_f1'(t*) have opposite signs  and
 *           g_f1(t*) - g_f2(t*) <= 2 tol (1 + |g_f2'| / |g_f1'|);
 *       among several the one with the largest g_f(t*); g_f1'(t*) == 0 is a smooth minimum.  (The search's dyadic t* may sit
 *       tol / |slope| from the kink where the two faces cross; the rule is what G(t*) - min G <= tol leaves.)  Then
 *           lam1 = g_f2' / (g_f2' - g_f1'), lam2 = 1 - lam1 (both in [0, 1]),
 *           jac[c][i] = (lam1 a_f1[c] + lam2 a_f2[c]) B_i^n(t*).
 *   The block is linear in the control points of the item's own vehicle only; the basis comes from the recurrence of the other
 *   envelope blocks, every multiply-add an explicit fma.  An end minimiser leaves one non-zero column; a NaN row a NaN block.
 * obtg_ctx_set_keep_out: copies H, obs_off and VO to the context (P = 0 clears the tables) and CLEARS any motion that
 *     obtg_ctx_set_keep_out_motion left: new tables stand still.  OBTG_ERR_ARG for a vehicle index
 *     outside 0 .. N-1, an obstacle index outside 0 .. O-1, a context whose d is not 2 or 3, obs_off[0] != 0, offsets that do not
 *     ascend (an empty obstacle) or a null table with P > 0; OBTG_ERR_UNSUPPORTED for an obstacle of more than 16 faces.
 * obtg_len_keep_out: P.
 * obtg_keep_out_true_min: out[B][P] the rows; nullable: t_star[B][P]; face[B][P][2], indices into H of f1 and f2 (-1: no second
 *     face); lam[B][P] = lam1 (1 without a second face); bound[B][P], the certified lower bound (the smallest bound dropped)
 *     minus margin, bound <= true row <= out and out - bound <= tol when status is OBTG_MD_OK; nodes[B][P]; status[B][P].
 *     Degrees 1 .. 31 (above: OBTG_ERR_UNSUPPORTED), one kernel, one launch.
 * obtg_keep_out_true_min_jac: the same outputs, bit for bit (the same kernel; the blocks are one more output), plus
 *     jac[B][P][d][n+1].
 * obtg_bern_keep_out: the same search on M free curves c[M][dim][K] (dim 2 or 3, 2 <= K <= 32, whatever the context's shape
 *     is) against ONE obstacle, the F <= 16 faces of H (a host array in the _dev form too), margin 0: val[M], nullable
 *     t_star[M], status[M].
 * An item's outputs depend on its control points, its faces, margin, eps_rel and max_nodes alone.  Host and _dev calls give the
 * same bits.  No tables set, or a context whose d is not 2 or 3: OBTG_ERR_ARG before any launch.  Every launch is timed under
 * OBTG_K_SPEED.  _dev: dY is device memory [B][N d][n+1]; dY = NULL inside an obtg_fd_view is not built for this family and
 * answers OBTG_ERR_ARG.  Not part of obtg_constraint_sweep_dev or of the structured step. */
int obtg_ctx_set_keep_out(obtg_ctx*, const double* H /*[F][d+1]*/, const int* obs_off /*[O+1]*/, int O, const int* VO /*[P][2]*/, int P);
int obtg_len_keep_out(const obtg_ctx*);     /* P                   */
int obtg_keep_out_true_min(obtg_ctx*, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out /*[B][P]*/,
                           double* t_star /*[B][P], nullable*/, int* face /*[B][P][2], nullable*/, double* lam /*[B][P], nullable*/,
                           double* bound /*[B][P], nullable*/, int* nodes /*[B][P], nullable*/, int* status /*[B][P], nullable*/);
int obtg_keep_out_true_min_dev(obtg_ctx*, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                               double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes, int* d_status);
int obtg_keep_out_true_min_jac(obtg_ctx*, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                               double* t_star, int* face, double* lam, double* bound, int* nodes, int* status,
                               double* jac /*[B][P][d][n+1]*/);
int obtg_keep_out_true_min_jac_dev(obtg_ctx*, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                                   double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes, int* d_status,
                                   double* d_jac);
int obtg_bern_keep_out(obtg_ctx*, const double* c /*[M][dim][K]*/, int M, int dim, int K, const double* H /*[F][dim+1]*/, int F,
                       double eps_rel, int max_nodes, double* val /*[M]*/, double* t_star /*[M], nullable*/, int* status /*[M], nullable*/);
int obtg_bern_keep_out_dev(obtg_ctx*, const double* d_c, int M, int dim, int K, const double* H, int F, double eps_rel, int max_nodes,
                           double* d_val, double* d_t_star, int* d_status);

/* ---- Euclidean keep-out clearance: the signed Euclidean distance in place of the largest face value ----
 * The rows above measure an obstacle by G = max_f g_f, which is the distance only where the nearest feature is a face; beside
 * a corner it is smaller, so a margin keeps a round vehicle out of the obstacle inflated with SHARP corners.  These calls use
 * the signed Euclidean distance D (rounded corners).  They read the tables of obtg_ctx_set_keep_out; obstacles that stand still
 * only (a motion on the context: OBTG_ERR_UNSUPPORTED).  The faces-metric calls above are untouched and keep reading the raw H.
 * Host geometry (csrc/keepout_features.h; obtg_keep_out_features), once per table, on the first Euclidean call after
 * obtg_ctx_set_keep_out, plain double arithmetic in this order:
 *     normalisation  s = a[0] a[0], then s = fma(a[c], a[c], s); n = sqrt(s); a^[c] = a[c] / n, b^ = b / n.  A face with
 *                    |a| = 1 is left bit for bit; |a| = 0 or a non-finite entry gives a NaN normal.
 *     Gram entries   G_kl = a^_k . a^_l in coordinate order, the first product alone, then fma; the diagonal likewise.
 *     features       d = 2: a pair (i < j) with det = G_ii G_jj - G_ij G_ij > 1e-12 whose point admits every other face;
 *                    d = 3, edges: such a pair whose common line, clipped by every other face, is not empty (a single point
 *                    counts); d = 3, vertices: a triple (i < j < k) with det Gram > 1e-12 whose point admits every other face.
 *                    The point is A^T (Gram^-1 b^); face m admits p iff a^_m . p - b^_m <= 1e-9 (1 + |b^_m|): tolerant, so a
 *                    feature is included rather than left out.  The line's direction is a^_i x a^_j; with s = a^_m . v and
 *                    r = 1e-9 (1 + |b^_m|) - (a^_m . p - b^_m): |s| <= 1e-12 empties the line iff r < 0, s > 0 gives t <= r / s,
 *                    s < 0 gives t >= r / s.
 *     Gram^-1        pair: (G_jj / det, -G_ij / det, G_ii / det) = entries (00, 01, 11); triple: the symmetric cofactors over
 *                    det = fma(G_ik, C_02, fma(G_ij, C_01, G_ii C_00)), entries (00, 01, 02, 11, 12, 22).
 *     table order    every pair in lexicographic order, then every triple in lexicographic order.
 * More than 128 features on one obstacle: OBTG_ERR_UNSUPPORTED from the Euclidean calls (never from obtg_ctx_set_keep_out).
 * The quantity.  With g_f(p) = a^_f . p - b^_f (the coefficient arithmetic of the rows above, on the normalised faces):
 *     D(p) = max_f g_f(p)                                   when that is <= 0     (inside: minus the depth)
 *     D(p) = max over the candidates of their value         otherwise,
 * the candidates being the faces (value g_f, lambda = e_f) and the features S whose multipliers mu = Gram_S^-1 g_S are all >= 0
 * (value sqrt(g_S . mu), lambda = mu / value).  Every candidate is dual feasible (lambda >= 0, |A^T lambda| = 1), so every
 * candidate is a lower bound of the distance and the largest is the distance; no primal test is made.  A feature left out of
 * the table can only make a row smaller (conservative); a set that is no feature changes nothing.
 *     row = min over t in [0, 1] of D(c(t))  -  margin.
 * Device arithmetic at a point (csrc/keepout_device.h), every multiply-add an explicit fma:
 *     pair     mu0 = fma(i01, g1, i00 g0), mu1 = fma(i11, g1, i01 g0); q = fma(g1, mu1, g0 mu0)
 *     triple   mu0 = fma(i02, g2, fma(i01, g1, i00 g0)), mu1 = fma(i12, g2, fma(i11, g1, i01 g0)),
 *              mu2 = fma(i22, g2, fma(i12, g1, i02 g0)); q = fma(g2, mu2, fma(g1, mu1, g0 mu0))
 *     a feature counts iff every mu >= 0 and q > 0; its value is sqrt(q).
 *     Evaluation order and ties: the candidates are taken in the order faces 0 .. F-1, then features in table order; lane l of
 *     the item's wavefront looks at face l and features l and l + 64, the wavefront's largest value wins, the FIRST of equals
 *     in that order.  The winner's dual pair: a face's (u, beta) = (a^_f, b^_f); a feature's lambda_k = mu_k / value,
 *     u[c] = lambda_0 a^_0[c], then fma(lambda_k, a^_k[c], .) for k = 1, 2, and beta the same on b^.
 * Search: the rows' above, word for word -- s = max |g_f,i| of the root, tol = eps_rel s, strict-decrease incumbent,
 * depth-first with the smaller bound first, 32 waiting frames, nodes, both caps with a valid bracket, the NaN rule (a face with
 * |a| = 0 or a non-finite entry: NaN items, status OBTG_MD_OK) -- with two changes.  The exact values at the root's ends and at
 * every split point are D there (the feature evaluation runs only where max_f g_f > 0).  And a sub-curve's bound is
 *     max( max_f min_i g_f,i ,  min_i (u . P_i - beta) ),
 * (u, beta) the winner's dual pair at the split point both children share, formed as fma(u[0], P[0][i], -beta), then
 * fma(u[c], P[c][i], .); the root takes the pairs of both ends.  It holds because D(p) >= u . p - beta for every p and every
 * dual-feasible pair (inside too: lambda . g <= (sum lambda) max g <= max g, as sum lambda >= |A^T lambda| = 1 and max g <= 0).
 * Near the minimiser u is perpendicular to c', so the gap closes quadratically in the width; the face bound alone never closes
 * at a corner minimum.
 * A root that closes reports bound = min(its bound, out): a dual bound and the value it meets are rounded apart, and
 * bound <= out holds in every case.
 * Envelope block at t*: jac[c][i] = dir[c] B_i^n(t*).  c(t*) and c'(t*) come from the item's own control points as for the rows
 * above.  max_f g_f(c(t*)) > 0: dir = u of the winner there and faces = its set -- no co-activity rule, D is C^1 outside.
 * Otherwise dir = lam1 a^_f1 + lam2 a^_f2 and faces = (f1, f2, -1) by the co-activity rule above on the normalised faces.
 * obtg_keep_out_features: Hn[F][d+1] the normalised faces; idx[128][3] the features' faces ascending, -1 padded; ginv[128][6] a
 *     pair's (00, 01, 11, 0, 0, 0), a triple's six; *n the count.  Needs no context and no device.  OBTG_ERR_ARG: a null pointer,
 *     F < 1, d not 2 or 3; OBTG_ERR_UNSUPPORTED: F > 16, or more than 128 features (*n is the count found, the first 128 stored).
 * obtg_keep_out_euclid_true_min: the outputs and conventions of obtg_keep_out_true_min with faces[B][P][3] (the active set,
 *     indices into H, -1 padded) and dir[B][P][d] in place of face and lam; both nullable.  bound <= true row <= out and
 *     out - bound <= tol when status is OBTG_MD_OK.
 * obtg_keep_out_euclid_true_min_jac: the same outputs, bit for bit (the same kernel; the blocks are one more output), plus
 *     jac[B][P][d][n+1].
 * obtg_bern_keep_out_euclid: M free curves against ONE obstacle H[F][dim+1] (raw faces, a host array in both forms), margin 0.
 * One kernel body with the rows above (csrc/keepout_kernels.hip), one launch; host and _dev calls give the same bits; an obstacle
 * of one face with |a| = 1 gives the bits of obtg_keep_out_true_min in every output the two share.  Refusals, timing and the
 * obtg_fd_view rule are those of the rows above. */
int obtg_keep_out_features(const double* H /*[F][d+1]*/, int F, int d, double* Hn /*[F][d+1]*/, int* idx /*[128][3]*/,
                           double* ginv /*[128][6]*/, int* n);
int obtg_keep_out_euclid_true_min(obtg_ctx*, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out /*[B][P]*/,
                                  double* t_star /*[B][P], nullable*/, int* faces /*[B][P][3], nullable*/,
                                  double* dir /*[B][P][d], nullable*/, double* bound /*[B][P], nullable*/, int* nodes /*[B][P], nullable*/,
                                  int* status /*[B][P], nullable*/);
int obtg_keep_out_euclid_true_min_dev(obtg_ctx*, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                                      double* d_t_star, int* d_faces, double* d_dir, double* d_bound, int* d_nodes, int* d_status);
int obtg_keep_out_euclid_true_min_jac(obtg_ctx*, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                      double* t_star, int* faces, double* dir, double* bound, int* nodes, int* status,
                                      double* jac /*[B][P][d][n+1]*/);
int obtg_keep_out_euclid_true_min_jac_dev(obtg_ctx*, const double* dY, int B, double margin, double eps_rel, int max_nodes,
                                          double* d_out, double* d_t_star, int* d_faces, double* d_dir, double* d_bound, int* d_nodes,
                                          int* d_status, double* d_jac);
int obtg_bern_keep_out_euclid(obtg_ctx*, const double* c /*[M][dim][K]*/, int M, int dim, int K, const double* H /*[F][dim+1]*/, int F,
                              double eps_rel, int max_nodes, double* val /*[M]*/, double* t_star /*[M], nullable*/,
                              int* status /*[M], nullable*/);
int obtg_bern_keep_out_euclid_dev(obtg_ctx*, const double* d_c, int M, int dim, int K, const double* H, int F, double eps_rel,
                                  int max_nodes, double* d_val, double* d_t_star, int* d_status);

/* ---- moving keep-out obstacles: a convex obstacle that translates along a known path ----
 * Obstacle o of the keep-out tables keeps its faces and may carry a motion: a Bezier offset q_o(time) with control points
 * Q_o[d][m_o+1] on the ABSOLUTE span [0, T_o].  Its body at `time` is {p : a_f . (p - q_o(time)) <= b_f}: translation only.
 * Vehicles live on [0, tf], tf per batch row.  With s in [0, 1] and r = tf / T_o:
 *     E(s)   = q_o(s tf)        the motion restricted to [0, r] of its own parameter, raised to the vehicle's degree n
 *     D_i    = P_i - E_i        the relative control points, i <= n
 *     g_f(s) = a_f . D(s) - b_f,  G = max_f g_f,  row = min_s G(s) - margin:   the static row of the curve D.
 * An obstacle without a motion is the static obstacle: D = P bit for bit, tf does not enter, d row / d tf is an exact 0.
 * The arithmetic of D (csrc/keepout_device.h keep_out_motion_points), every multiply-add an explicit fma; it needs m_o <= n:
 *     ratio        r = tf / T_o, one division;
 *     restriction  de Casteljau at r, each level b = fma(r, up, (1 - r) * b) with 1 - r rounded once; point j of the left piece
 *                  is the first value after level j.  At r == 1 this is the identity, bit for bit (a zero may change sign);
 *     elevation    n - m_o single-degree steps, degree k -> k + 1: E_i = fma(w, E_(i-1), (1 - w) * E_i) with
 *                  w = (double)i / (k + 1); the ends (w = 0 and w = 1) are exact; at m_o == n there are zero steps;
 *     difference   D = P - E, one subtraction.
 * r > 1 (tf beyond the motion's span; a time-optimal solve may overshoot) is answered by the polynomial's continuation, the
 * same instructions: NO rounding bound is claimed there (de Casteljau outside [0, 1] is not a convex combination).
 * Non-finite input follows the static convention: a non-finite Q, T_o or tf, tf <= 0, or a ratio that is not finite and
 * positive: NaN outputs (rel and jac_tf too; face -1, nodes 0), status OBTG_MD_OK -- for the items of a moving obstacle.
 * Envelope Jacobian.  a^ = lam1 a_f1 + lam2 a_f2, faces and lam by the static rule on D(s*), D'(s*).  The block with respect to
 * the vehicle's control points is the static one, jac[c][i] = a^[c] B_i(s*).  New is the explicit
 *     d row / d tf = -(a^ . E'(s*)) s* / tf          (dE/d tf = s q_o'(s tf) = s E'(s) / tf),
 * E'(s*) = n (E1 - E0) of de Casteljau on E at s*, the dot product summed in coordinate order, then * s*, then / tf: jac_tf[B][P].
 * obtg_ctx_set_keep_out_motion: Q the obstacles' [d][m_o+1] blocks one after the other, q_off[O+1] in control points (an empty
 *     run: that obstacle stands still), T[O] (read for moving obstacles only).  O = 0 clears the motion.  OBTG_ERR_ARG: no
 *     keep-out tables set, an O other than the tables', offsets that do not start at 0 or descend, a T_o that is not finite and
 *     positive, a null table; OBTG_ERR_UNSUPPORTED: m_o > n.
 * obtg_keep_out_moving_true_min: the outputs and conventions of obtg_keep_out_true_min, tf[B] the rows' spans; rel (nullable)
 *     returns the relative control points D[B][P][d][n+1] the search ran on.  OBTG_ERR_ARG without a motion on the context.
 * obtg_keep_out_moving_true_min_jac: the same outputs, bit for bit, plus jac[B][P][d][n+1] and jac_tf[B][P].
 * obtg_bern_keep_out_moving: M free curves c[M][dim][K] against ONE obstacle H[F][dim+1] moving by Q[dim][Km], 1 <= Km <= K
 *     (above: OBTG_ERR_UNSUPPORTED); r[M] the ratio per curve (null: 1 for all) -- H and Q host arrays in both forms, r device
 *     memory in the _dev form.  margin 0: val[M], nullable t_star[M], status[M].
 * One kernel, one launch: the static search's body, whose root is read from D (csrc/keepout_kernels.hip).  Host and _dev calls
 * give the same bits; dY = NULL inside an obtg_fd_view answers OBTG_ERR_ARG; every launch is timed under OBTG_K_SPEED. */
int obtg_ctx_set_keep_out_motion(obtg_ctx*, const double* Q, const int* q_off /*[O+1]*/, const double* T /*[O]*/, int O);
int obtg_keep_out_moving_true_min(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double margin, double eps_rel,
                                  int max_nodes, double* out /*[B][P]*/, double* t_star, int* face, double* lam, double* bound,
                                  int* nodes, int* status, double* rel /*[B][P][d][n+1], nullable*/);
int obtg_keep_out_moving_true_min_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double margin, double eps_rel,
                                      int max_nodes, double* d_out, double* d_t_star, int* d_face, double* d_lam, double* d_bound,
                                      int* d_nodes, int* d_status, double* d_rel);
int obtg_keep_out_moving_true_min_jac(obtg_ctx*, const double* Y, const double* tf, int B, double margin, double eps_rel, int max_nodes,
                                      double* out, double* t_star, int* face, double* lam, double* bound, int* nodes, int* status,
                                      double* rel, double* jac /*[B][P][d][n+1]*/, double* jac_tf /*[B][P]*/);
int obtg_keep_out_moving_true_min_jac_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double margin, double eps_rel,
                                          int max_nodes, double* d_out, double* d_t_star, int* d_face, double* d_lam, double* d_bound,
                                          int* d_nodes, int* d_status, double* d_rel, double* d_jac, double* d_jac_tf);
int obtg_bern_keep_out_moving(obtg_ctx*, const double* c /*[M][dim][K]*/, int M, int dim, int K, const double* H /*[F][dim+1]*/, int F,
                              const double* Q /*[dim][Km]*/, int Km, const double* r /*[M], nullable: 1*/, double eps_rel, int max_nodes,
                              double* val /*[M]*/, double* t_star /*[M], nullable*/, int* status /*[M], nullable*/);
int obtg_bern_keep_out_moving_dev(obtg_ctx*, const double* d_c, int M, int dim, int K, const double* H, int F, const double* Q, int Km,
                                  const double* d_r, double eps_rel, int max_nodes, double* d_val, double* d_t_star, int* d_status);

/* ---- polytopic vehicle-to-vehicle separation: a pair's relative curve stays outside ONE convex region around the origin ----
 * The context holds one separation region R = {d : a_f . d <= b_f}, F faces (1 <= F <= 16), every b_f > 0: the origin is
 * strictly inside, so vehicles at the same place violate the row.  For batch row B the items are the pairs i < j of the N
 * vehicles in lexicographic order (np.triu_indices(N, 1); the order of obtg_temporal_sep_true_min), P = N (N - 1) / 2:
 *     D[c][k]  = Y[i*d + c][k] - Y[j*d + c][k]          one subtraction per control point: the relative curve c_i - c_j
 *     row(i,j) = min over t in [0, 1] of G(D(t)) - margin,
 * G = max_f (a_f . p - b_f) for the faces calls (the keep-out rows above) and the signed Euclidean distance on the normalised
 * faces for the _euclid calls ("Euclidean keep-out clearance" above): negative inside, as for obstacles.  The region does not
 * move in the pair's frame, so a row IS the static keep-out row of a vehicle whose control points are D against the region as
 * its one obstacle -- the same kernel body (csrc/keepout_kernels.hip), whose root reads D where the static form reads Y; every
 * output equals that static call's, bit for bit.  A region with R != -R makes a row depend on which vehicle of the pair comes
 * first (i, the one with the smaller index); ordered pairs are not built.  Vehicles only: point and curve obstacles do not enter.
 * Envelope block at the returned t_star, jac[B][P][d][n+1]: the block of the pair's FIRST vehicle, what the static calls give for
 * the curve D (faces: (lam1 a_f1 + lam2 a_f2)[c] B_k(t_star); Euclidean: dir[c] B_k(t_star)).  The second vehicle's block is
 * its exact negation and is not stored.  There is no explicit tf column: tf enters through dY/dtf alone.
 * obtg_ctx_set_pair_keep_out: H[F][d+1] = (a_f, b_f), copied; F = 0 clears.  Independent of obtg_ctx_set_keep_out and of a motion
 *     set on it.  OBTG_ERR_ARG: a context whose d is not 2 or 3, a null H, F < 0, a b_f that is not > 0 (a NaN b_f passes and gives
 *     NaN rows, as a NaN face does everywhere); OBTG_ERR_UNSUPPORTED: F > 16.
 * obtg_len_pair_keep_out: P while a region is set, else 0.
 * obtg_pair_keep_out_true_min: the outputs and conventions of obtg_keep_out_true_min (face indexes the region's faces), plus rel
 *     (nullable): the D[B][P][d][n+1] the search ran on, NaN for an item that is not finite.  A non-finite control point: NaN
 *     outputs for exactly the pairs that contain its vehicle (face -1, nodes 0), status OBTG_MD_OK.
 * obtg_pair_keep_out_true_min_jac: the same bits, plus jac.
 * obtg_pair_keep_out_euclid_true_min[_jac]: the outputs of obtg_keep_out_euclid_true_min[_jac] (faces[B][P][3], dir[B][P][d]),
 *     plus rel.  The normalised faces and the feature records are made on the first Euclidean call after the region is set; more
 *     than 128 features: OBTG_ERR_UNSUPPORTED, from these calls only.
 * Refusals, all before any launch: no region, d not 2 or 3, or an argument obtg_keep_out_true_min refuses: OBTG_ERR_ARG; degree
 * above 31: OBTG_ERR_UNSUPPORTED.  N = 1: P = 0, OBTG_OK, nothing written.  One launch, timed under OBTG_K_SPEED; host and _dev
 * calls give the same bits; _dev takes device pointers, and dY = NULL inside an obtg_fd_view answers OBTG_ERR_ARG. */
int obtg_ctx_set_pair_keep_out(obtg_ctx*, const double* H /*[F][d+1]*/, int F);
int obtg_len_pair_keep_out(const obtg_ctx*);
int obtg_pair_keep_out_true_min(obtg_ctx*, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out /*[B][P]*/,
                                double* t_star, int* face /*[B][P][2]*/, double* lam, double* bound, int* nodes, int* status,
                                double* rel /*[B][P][d][n+1], nullable*/);
int obtg_pair_keep_out_true_min_dev(obtg_ctx*, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                                    double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes, int* d_status,
                                    double* d_rel);
int obtg_pair_keep_out_true_min_jac(obtg_ctx*, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                    double* t_star, int* face, double* lam, double* bound, int* nodes, int* status, double* rel,
                                    double* jac /*[B][P][d][n+1]*/);
int obtg_pair_keep_out_true_min_jac_dev(obtg_ctx*, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                                        double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes, int* d_status,
                                        double* d_rel, double* d_jac);
int obtg_pair_keep_out_euclid_true_min(obtg_ctx*, const double* Y, int B, double margin, double eps_rel, int max_nodes,
                                       double* out /*[B][P]*/, double* t_star, int* faces /*[B][P][3]*/, double* dir /*[B][P][d]*/,
                                       double* bound, int* nodes, int* status, double* rel /*[B][P][d][n+1], nullable*/);
int obtg_pair_keep_out_euclid_true_min_dev(obtg_ctx*, const double* dY, int B, double margin, double eps_rel, int max_nodes,
                                           double* d_out, double* d_t_star, int* d_faces, double* d_dir, double* d_bound, int* d_nodes,
                                           int* d_status, double* d_rel);
int obtg_pair_keep_out_euclid_true_min_jac(obtg_ctx*, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                           double* t_star, int* faces, double* dir, double* bound, int* nodes, int* status, double* rel,
                                           double* jac /*[B][P][d][n+1]*/);
int obtg_pair_keep_out_euclid_true_min_jac_dev(obtg_ctx*, const double* dY, int B, double margin, double eps_rel, int max_nodes,
                                               double* d_out, double* d_t_star, int* d_faces, double* d_dir, double* d_bound,
                                               int* d_nodes, int* d_status, double* d_rel, double* d_jac);

/* ---- the acceleration bound: |d^2 c / dtime^2| <= bound for every vehicle, in 2-D, 3-D and any other dimension ----
 * For vehicle v with control points P[c][i] (c < d, i <= n) on a span T = tf[b]:
 *     q(t) = bound**2 - (d/2) |c''(t)|^2,    c''_c(t) = (n(n-1)/T^2) sum_{i<=n-2} B_i^(n-2)(t) (P[c][i+2] - 2 P[c][i+1] + P[c][i]).
 * normSquare's (d/2) factor and Python's bound**2 are kept, as for the speed rows.
 * obtg_accel: the 2n+R+1 Bernstein coefficients of q, out[B][N][2n+R+1], in the reference's sequence for the acceleration
 *     (optimization.py:503-519): diff() (the derivative, then elev(1)), diff() again, normSquare(), elev(R), then
 *     fma(-1, c, bound**2).  The second derivative's control points are formed by csrc/bern_device.h diff_elev1_at applied
 *     twice, every multiply-add an explicit fma: every kernel form gives the same source curve.  Degree 1: every row equals
 *     bound**2.  Argument checks, the specialised shapes and the any-degree route are obtg_speed's; _dev: dY may be NULL inside
 *     an obtg_fd_view.
 * obtg_accel_true_min: out[B][N] = min over t in [0, 1] of q: feasible iff >= 0, bound**2 - max over t of (d/2)|c''|^2.  DEG_ELEV
 *     does not enter and the context's R is not read.  The 2n+1 coefficients are the bits of obtg_accel's rows on a context with
 *     DEG_ELEV = 0, so out, t_star, status are the bits of obtg_bern_extrema(eps_abs = 0, want_max = 0) on those rows.  An end
 *     coefficient that is the row's smallest is returned as is (t_star 0 or 1).  A row with a non-finite coefficient: val and
 *     t_star NaN, status OBTG_MD_OK.  tf <= 0 is the caller's business.  Degrees with a specialised kernel (obtg_fast_kernels & 1)
 *     form the coefficients in registers, one launch; other degrees up to 31 go through a workspace of obtg_accel's R = 0 rows
 *     (two launches); above 31: OBTG_ERR_UNSUPPORTED.  t_star and status are nullable.
 * obtg_accel_true_min_jac: out, t_star, status are, bit for bit, those of obtg_accel_true_min with the same arguments, and the
 *     envelope (Danskin) block of every row at its t_star.  With u = B^(n-2)(t_star), entries out of range 0:
 *         C_i = (n(n-1)/T^2)(u_(i-2) - 2 u_(i-1) + u_i)
 *         jac[B][N][d][n+1]:  jac[c][i] = -d * c''_c(t_star) * C_i
 *         jac_tf[B][N] (nullable):  -4 (q(t_star) - bound**2) / T, q(t_star) - bound**2 = -(d/2)|c''(t_star)|^2 from the same u
 *     -- the partial derivatives of q AT THE RETURNED t_star with respect to the vehicle's own control points and to tf at fixed
 *     control points.  t_star = 0 leaves columns 0, 1, 2 as the only non-zero ones, t_star = 1 columns n-2, n-1, n; degree 1: a
 *     zero block.  A row with a non-finite coefficient gets a NaN block and a NaN jac_tf (status OBTG_MD_OK); with another
 *     status the block is still the derivative at the returned t_star.  Every multiply-add is an explicit fma
 *     (csrc/bern_device.h accel_envelope_block): a block depends on the vehicle's control points, tf and t_star alone, not on the
 *     entry point (host and _dev: same bits) or the kernel form.  Fused value-and-blocks kernels (one launch): degrees 3, 5, 7,
 *     8, 10, 15, 20 in 2-D and 3-D, every specialised count -- all build without scratch; a context created under
 *     OBTG_TRUE_MIN_JAC_FUSED=0 forms the blocks in one more launch from Y, tf and t_star on every shape, as other degrees up to
 *     31 do after their value path (three launches).  Degrees above 31: OBTG_ERR_UNSUPPORTED.
 * Every launch is timed under OBTG_K_SPEED.  _dev: dY may be NULL inside an obtg_fd_view; d_tf is device memory, [B]. */
int obtg_accel(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double bound, double* out /*[B][N][2n+R+1]*/);
int obtg_accel_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, double* d_out);
int obtg_accel_true_min(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double bound, double eps_rel, int max_nodes,
                        double* out /*[B][N]*/, double* t_star /*[B][N], nullable*/, int* status /*[B][N], nullable*/);
int obtg_accel_true_min_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, double eps_rel, int max_nodes,
                            double* d_out, double* d_t_star, int* d_status);
int obtg_accel_true_min_jac(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double bound, double eps_rel, int max_nodes,
                            double* out /*[B][N]*/, double* t_star /*[B][N], nullable*/, int* status /*[B][N], nullable*/,
                            double* jac /*[B][N][d][n+1]*/, double* jac_tf /*[B][N], nullable*/);
int obtg_accel_true_min_jac_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, double eps_rel, int max_nodes,
                                double* d_out, double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf);

/* ---- the jerk bound: |d^3 c / dtime^3| <= bound for every vehicle, in 2-D, 3-D and any other dimension ----
 * For vehicle v with control points P[c][i] (c < d, i <= n) on a span T = tf[b]:
 *     q(t) = bound**2 - (d/2) |c'''(t)|^2,
 *     c'''_c(t) = (n(n-1)(n-2)/T^3) sum_{i<=n-3} B_i^(n-3)(t) (P[c][i+3] - 3 P[c][i+2] + 3 P[c][i+1] - P[c][i]).
 * normSquare's (d/2) factor and Python's bound**2 are kept, as for the speed and acceleration rows.
 * obtg_jerk: the 2n+R+1 Bernstein coefficients of q, out[B][N][2n+R+1], in the reference's sequence for the jerk
 *     (optimization.py:522-539): diff() (the derivative, then elev(1)) three times, normSquare(), elev(R), then
 *     fma(-1, c, bound**2).  The third derivative's control points are formed by csrc/bern_device.h diff_elev1_at applied
 *     three times (diff3_elev1_rows), every multiply-add an explicit fma: every kernel form gives the same source curve.
 *     Degree 1: the second pass is exactly zero, every row equals bound**2 bit for bit.  Degree 2: the third derivative is
 *     zero, but three rounded passes need not cancel: the rows equal bound**2 up to that residue (the reference's own chain
 *     leaves one too).  Degree 3: the jerk is constant, the row constant in t up to rounding.  Argument checks, the specialised
 *     shapes and the any-degree route are obtg_speed's; _dev: dY may be NULL inside an obtg_fd_view.
 * obtg_jerk_true_min: out[B][N] = min over t in [0, 1] of q: feasible iff >= 0, bound**2 - max over t of (d/2)|c'''|^2.
 *     DEG_ELEV does not enter and the context's R is not read.  The 2n+1 coefficients are the bits of obtg_jerk's rows on a
 *     context with DEG_ELEV = 0, so out, t_star, status are the bits of obtg_bern_extrema(eps_abs = 0, want_max = 0) on those
 *     rows.  An end coefficient that is the row's smallest is returned as is (t_star 0 or 1).  Degree 3: t_star is anywhere in
 *     [0, 1]; degree 4: c''' is linear, the row concave, every minimum at an end.  A row with a non-finite coefficient: val
 *     and t_star NaN, status OBTG_MD_OK.  tf <= 0 is the caller's business.  Degrees with a specialised kernel
 *     (obtg_fast_kernels & 1) form the coefficients in registers, one launch; other degrees up to 31 go through a workspace
 *     of obtg_jerk's R = 0 rows (two launches); above 31: OBTG_ERR_UNSUPPORTED.  t_star and status are nullable.
 * obtg_jerk_true_min_jac: out, t_star, status are, bit for bit, those of obtg_jerk_true_min with the same arguments, and the
 *     envelope (Danskin) block of every row at its t_star.  With u = B^(n-3)(t_star), entries out of range 0:
 *         C_i = (n(n-1)(n-2)/T^3)(u_(i-3) - 3 u_(i-2) + 3 u_(i-1) - u_i)
 *         jac[B][N][d][n+1]:  jac[c][i] = -d * c'''_c(t_star) * C_i
 *         jac_tf[B][N] (nullable):  -6 (q(t_star) - bound**2) / T, q(t_star) - bound**2 = -(d/2)|c'''(t_star)|^2 from the same u
 *     -- the partial derivatives of q AT THE RETURNED t_star with respect to the vehicle's own control points and to tf at fixed
 *     control points.  t_star = 0 leaves columns 0 .. 3 as the only non-zero ones, t_star = 1 columns n-3 .. n; degrees 1 and
 *     2: a zero block; degree 3: the same block at every t.  A row with a non-finite coefficient gets a NaN block and a NaN
 *     jac_tf (status OBTG_MD_OK); with another status the block is still the derivative at the returned t_star.  Every
 *     multiply-add is an explicit fma (csrc/bern_device.h jerk_envelope_block): a block depends on the vehicle's control
 *     points, tf and t_star alone, not on the entry point (host and _dev: same bits) or the kernel form.  Fused
 *     value-and-blocks kernels (one launch): degrees 3, 5, 7, 8, 10, 15, 20 in 2-D and 3-D, every specialised count -- all
 *     build without scratch; a context created under OBTG_TRUE_MIN_JAC_FUSED=0 forms the blocks in one more launch from Y, tf
 *     and t_star on every shape, as other degrees up to 31 do after their value path (three launches).  Degrees above 31:
 *     OBTG_ERR_UNSUPPORTED.
 * Every launch is timed under OBTG_K_SPEED.  _dev: dY may be NULL inside an obtg_fd_view; d_tf is device memory, [B]. */
int obtg_jerk(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double bound, double* out /*[B][N][2n+R+1]*/);
int obtg_jerk_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, double* d_out);
int obtg_jerk_true_min(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double bound, double eps_rel, int max_nodes,
                       double* out /*[B][N]*/, double* t_star /*[B][N], nullable*/, int* status /*[B][N], nullable*/);
int obtg_jerk_true_min_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, double eps_rel, int max_nodes,
                           double* d_out, double* d_t_star, int* d_status);
int obtg_jerk_true_min_jac(obtg_ctx*, const double* Y, const double* tf /*[B]*/, int B, double bound, double eps_rel, int max_nodes,
                           double* out /*[B][N]*/, double* t_star /*[B][N], nullable*/, int* status /*[B][N], nullable*/,
                           double* jac /*[B][N][d][n+1]*/, double* jac_tf /*[B][N], nullable*/);
int obtg_jerk_true_min_jac_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double bound, double eps_rel, int max_nodes,
                               double* d_out, double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf);

/* ---- single-curve Bernstein algebra (the Bezier object's methods, batched over rows) ----
 * obtg_bern_elev:   Bezier.elev(R)      bezier.py:469-495   in[rows][n+1]   -> out[rows][n+R+1]
 * obtg_bern_diff:   Bezier.diff()       bezier.py:497-519   in[rows][n+1]   -> out[rows][n+1]  (T = tf-t0)
 * obtg_bern_mul:    Bezier.mul          bezier.py:376-432   a[rows][m+1], b[rows][n+1] -> out[rows][m+n+1]
 * obtg_bern_normsq: Bezier.normSquare() bezier.py:869-889   x[d][n+1]       -> out[2n+1]  ((d/2) quirk kept)
 * obtg_bern_split:  Bezier.split(tDiv)  bezier.py:533-572 -> deCasteljauSplit 985-1027   in[rows][n+1] ->
 *                   left[rows][n+1], right[rows][n+1] at z = (tDiv - t0)/(tf - t0); `right` is in the curve's own
 *                   orientation (the reference reverses deCasteljauSplit's second array, bezier.py:563)
 * obtg_bern_restrict: one curve's share of _temporalAlignment  bezier.py:903-941   in[rows][n+1] on span[rows][2] = (t0, tf)
 *                   -> out[rows][n+1] on target[rows][2] = (a, e): the right piece of a split at (a - t0)/(tf - t0) when
 *                   t0 < a, then the left piece of a split at (e - a)/(tf - a) when e < tf (two curves aligned in ONE call
 *                   instead of up to four obtg_bern_split calls).  OBTG_ERR_ARG unless t0 <= a < e <= tf in every row.
 * Limits.  A row -- input or output -- holds at most 1024 coefficients (n + R + 1, m + n + 1, 2n + 1, n + 1 <= 1024), and
 * obtg_bern_eval takes at most 125 control points (its per-lane working rows fill the 64 KB of LDS of one launch); beyond
 * either the call answers OBTG_ERR_UNSUPPORTED and launches nothing.  Elevation and the products form the unnormalised sum
 * sum_j a_j C(n,j) C(R,k-j) BEFORE dividing by C(n+R,k), so a result is finite only while max|a| C(n+R, (n+R)/2) stays
 * below DBL_MAX (products: max|a| max|b| C(m+n, (m+n)/2)): magnitudes below about 50 at 1024 coefficients, below about
 * 1e150 at 500. */
int obtg_bern_elev(obtg_ctx*, const double* in, int rows, int n, int R, double* out);
int obtg_bern_diff(obtg_ctx*, const double* in, int rows, int n, double T, double* out);
int obtg_bern_mul(obtg_ctx*, const double* a, const double* b, int rows, int m, int n, double* out);
int obtg_bern_normsq(obtg_ctx*, const double* x, int d, int n, double* out);
int obtg_bern_split(obtg_ctx*, const double* in, int rows, int n, double z, double* left, double* right);
int obtg_bern_restrict(obtg_ctx*, const double* in, int rows, int n, const double* span, const double* target, double* out);
/* Bezier.__call__ / Bezier.curve (bezier.py:184-199, 233-258) -> deCasteljauCurve (bezier.py:945-982): every row of
 * cpts[rows][n+1] at every tau[k]: out[rows][n_tau], T = (tau - t0) / (tf - t0), the de Casteljau triangle per sample. */
int obtg_bern_eval(obtg_ctx*, const double* cpts, int rows, int n, const double* tau, int n_tau, double t0, double tf, double* out);

/* ---- objectives (optimization.py:462-489 _euclideanObjective, 503-519 _minAccelObjective,
 * 522-539 _minJerkObjective): sums over vehicles of the elevated |d^k pos/dt^k|^2 control
 * points, k = 2 (accel) or 3 (jerk); tf[B] must hold ONE final time B times, as the reference has a single
 * model['tf'] for these objectives (a batch with differing tf is OBTG_ERR_ARG). */
int obtg_euclidean_obj(obtg_ctx*, const double* Y, int B, double* out /*[B]*/);
int obtg_accel_obj(obtg_ctx*, const double* Y, const double* tf, int B, double* out /*[B]*/);
int obtg_jerk_obj(obtg_ctx*, const double* Y, const double* tf, int B, double* out /*[B]*/);

/* ---- true arc length (arclen_kernels.hip) ------------------------------------------------------
 * The length of the curve itself, L = int_0^1 |c'(t)| dt, and its gradient -- NOT something the reference computes: its
 * `minGoal='euclidean'` (optimization.py:462-489) sums the control polygon, an upper bound of L that shrinks under degree
 * elevation and whose gradient is NaN where two neighbouring control points coincide.  This is the quantity that bound stands
 * in for, with a stated contract like obtg_bern_extrema's.  L depends on neither tf nor the span: there is no tf argument.
 * c[M][d][K]: M independent curves of K = n + 1 control points in d dimensions, 1 <= d <= 3 (else OBTG_ERR_ARG), degree
 * 1 <= n <= 31 (K < 2: OBTG_ERR_ARG; K > 32: OBTG_ERR_UNSUPPORTED); independent of the context's shape.
 * Rule: adaptive bisection with the 8-point Gauss-Legendre rule per panel.  A panel [a, a + w] has the estimate
 * G = (w / 2) sum_k omega_k |c'(a + w (1 + x_k) / 2)|; with S = the length of the curve's control polygon (what
 * obtg_euclidean_obj sums: a majorant of L known before the search) and tol = eps_rel * S it is accepted when
 * |G - (G_left + G_right)| <= tol * w.  Depth first, left to right; a and w are dyadic and so exact.
 *   len[M]      the sum of G_left + G_right over the accepted panels, in that order -- kept inside the bracket the length lies in,
 *               chord <= L <= S (chord = |P_n - P_0|, both as rounded on the device): a sum that passes an end, which the
 *               quadrature's error can do where the curve leaves no room (a straight line, a monotone curve in one dimension),
 *               is returned as that end, which is nearer to L; so len never exceeds what obtg_euclidean_obj sums;
 *   err[M]      the sum of |G - G_left - G_right| over them: with status OBTG_MD_OK err <= tol (the widths sum to 1), and the
 *               true error of len is far below it (the accepted estimate is the finer one);
 *   nodes[M]    panel estimates formed: 1 for [0, 1] and 2 per bisection (a straight line: 3 at any eps_rel);
 *   status[M]   OBTG_MD_OK; OBTG_MD_DEPTH_CAP: a panel of width 2^-48 still failed the test and was accepted as it was (a cusp
 *               off every dyadic point, under a tol near the floor); OBTG_MD_NODE_CAP: max_nodes estimates were used up and the
 *               panels still waiting were accepted with the estimate they had (they add nothing to err).  Both: DEPTH_CAP.
 *   grad[M][d][K]  nullable: the derivative of the returned len with respect to the control points, for the panel set the search
 *               ended on: grad[c][i] = sum over the accepted nodes t_k with weight q_k of
 *               q_k (c'_c(t_k) / |c'(t_k)|) n (B_(i-1)^(n-1)(t_k) - B_i^(n-1)(t_k)), B_(-1) = B_n = 0 -- what SLSQP needs: forward
 *               differences of len at a step of 1.5e-8 divide tol by that step.  Where len is an end of the bracket, grad is
 *               that end's gradient (S: the unit vectors of the two segments at a control point, none for a segment of length
 *               0; chord: its unit vector at the two end points).  A node with |c'| = 0 adds nothing: a constant
 *               curve has len 0 and an all-zero grad, not NaN.  Every entry is bounded by 2.  At a cusp the integrand of the
 *               gradient jumps where that of the length has a kink: its error there is a larger multiple of eps_rel than len's.
 * Floor of eps_rel: one estimate is 3 n + d + 9 rounded operations deep on a speed of up to n S, so below
 * 2 n (3 n + d + 9) 2^-53 rounding alone can fail the test; a smaller eps_rel (0 included) is raised to that floor.
 * A curve with a non-finite control point (or whose polygon overflows): len, err, grad NaN, nodes 0, status OBTG_MD_OK.
 * A curve's results depend on its control points, eps_rel and max_nodes alone: not on M, the other curves, its position or
 * the entry point; host and _dev give the same bits.  err, nodes, grad are nullable (and status in the _dev form); M == 0 is
 * OBTG_OK; max_nodes < 1 or eps_rel < 0 (or NaN): OBTG_ERR_ARG.  Timed under OBTG_K_ARC_LENGTH.
 *
 * obtg_arc_length_obj: the objective on the context's shape, out[b] = sum_v len[b][v] in vehicle order on the device, with
 * Y viewed as [B * N][d][n + 1]: the per-vehicle lengths and gradient blocks are the bits of obtg_bern_arc_length.
 * status[B] (nullable): the worst status among the row's vehicles; grad[B][N*d][n+1] (nullable): obtg_euclidean_grad's layout.
 * _dev: dY is a batch in device memory (not NULL: an obtg_fd_view does not serve these calls). */
int obtg_bern_arc_length(obtg_ctx*, const double* c /*[M][d][K]*/, int M, int d, int K, double eps_rel, int max_nodes,
                         double* len /*[M]*/, double* err /*[M], nullable*/, int* nodes /*[M], nullable*/,
                         int* status /*[M]*/, double* grad /*[M][d][K], nullable*/);
int obtg_bern_arc_length_dev(obtg_ctx*, const double* d_c, int M, int d, int K, double eps_rel, int max_nodes,
                             double* d_len, double* d_err, int* d_nodes, int* d_status, double* d_grad);
int obtg_arc_length_obj(obtg_ctx*, const double* Y, int B, double eps_rel, int max_nodes,
                        double* out /*[B]*/, int* status /*[B], nullable*/, double* grad /*[B][N*d][n+1], nullable*/);
int obtg_arc_length_obj_dev(obtg_ctx*, const double* dY, int B, double eps_rel, int max_nodes,
                            double* d_out, int* d_status, double* d_grad);

/* ---- exact derivatives (the `jac` SLSQP takes; no finite differences) ----------------------
 * With n = deg, d = dim, R = deg_elev, L = 2n+R+1, La = 4(n+R)+1, P = C(N+M, 2); every block is batched over the B rows
 * of Y like the value entry points, and the entries of a block are the partial derivatives with respect to the control
 * points Y[v*d + c][i] of ONE vehicle, laid out [d][n+1] (c major).
 * obtg_temporal_sep_jac: d/dP_a of obtg_temporal_sep's rows (optimization.py:311-346), out[B][P][L][d][n+1] for pair (a, b)
 *   in lexicographic order.  The b side is the exact negation of the a side and is not stored; when b is a point obstacle
 *   it has no variable, and a pair of two obstacles is all zeros.
 * obtg_speed_jac: d/dP_v of obtg_speed's rows (optimization.py:349-422, diff's trailing elev(1) included), out[B][N][L][d][n+1],
 *   the sign of is_max applied (bound^2 - v: negated); out_tf[B][N][L] (nullable) = d/dtf at fixed control points
 *   (the rows scale as tf^-2).
 * obtg_ang_rate_jac: dim 2, d/dP_v of obtg_ang_rate's rows (optimization.py:425-459, 578-611), out[B][N][La][2][n+1],
 *   out_tf[B][N][La] (nullable).  Numerator and denominator are differentiated at degree 4n and elevated by 4R -- elevation
 *   is exact, so these are the derivatives of the rows of every obtg_ctx_set_ang_rate_order.  A row whose quotient is not
 *   finite (a vehicle at rest at a control point of |v|^2) gets NaN derivatives.  OBTG_ERR_UNSUPPORTED for n > 15 or
 *   4R > 1000, and where the per-vehicle working set passes 64 KB of LDS (at n = 15: R > 177).
 * obtg_euclidean_grad: gradient of obtg_euclidean_obj (optimization.py:462-489), out[B][N*d][n+1]; a zero-length
 *   segment gives NaN at its two ends.
 * obtg_deriv_energy_grad: gradient of obtg_accel_obj (order 2, optimization.py:503-519) / obtg_jerk_obj (order 3,
 *   optimization.py:522-539), out[B][N*d][n+1], out_tf[B] (nullable) = d/dtf (the objective scales as tf^(-2 order)). */
int obtg_temporal_sep_jac(obtg_ctx*, const double* Y, int B, double* out);
int obtg_temporal_sep_jac_dev(obtg_ctx*, const double* dY, int B, double* d_out);
int obtg_speed_jac(obtg_ctx*, const double* Y, const double* tf, int B, int is_max, double* out, double* out_tf);
int obtg_speed_jac_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, int is_max, double* d_out, double* d_out_tf);
int obtg_ang_rate_jac(obtg_ctx*, const double* Y, const double* tf, int B, double* out, double* out_tf);
int obtg_ang_rate_jac_dev(obtg_ctx*, const double* dY, const double* d_tf, int B, double* d_out, double* d_out_tf);
int obtg_euclidean_grad(obtg_ctx*, const double* Y, int B, double* out);
int obtg_deriv_energy_grad(obtg_ctx*, const double* Y, const double* tf, int B, int order, double* out, double* out_tf);

/* ---- instrumentation -------------------------------------------------------------------
 * When enabled every kernel launch is bracketed by HIP events on the launch stream;
 * obtg_kernel_stats returns the accumulated device time and launch count per kernel id. */
enum {
    OBTG_K_TEMPORAL_SEP = 0, OBTG_K_SPEED = 1, OBTG_K_ANG_RATE = 2, OBTG_K_GJK = 3,
    OBTG_K_MIN_DIST = 4, OBTG_K_FD_BATCH = 5, OBTG_K_BERN = 6, OBTG_K_PAIR_SWEEP = 7, OBTG_K_JAC = 8, OBTG_K_COUNT = 9,
    /* ids added after revision 7 was cut (OBTG_K_COUNT is what that revision's callers size their arrays by, and stays) */
    OBTG_K_ARC_LENGTH = 9, OBTG_K_END = 10
};
/* on: 0 = off, 1 = every kernel, OBTG_PROFILE_ONLY(id) = only launches of that kernel id (two
 * events per launch drain the queue between kernels: 15 % of a 0.25 ms step when all three
 * launches of the step carry them, hence the selective form for timed regions). */
#define OBTG_PROFILE_ONLY_FLAG 0x100
#define OBTG_PROFILE_ONLY(kernel_id) (OBTG_PROFILE_ONLY_FLAG | (kernel_id))
int obtg_set_profiling(obtg_ctx*, int on);
/* sample: events on every `every`-th eligible launch of each kernel id (1 = all, the default) */
int obtg_set_profile_period(obtg_ctx*, int every);
int obtg_kernel_stats(obtg_ctx*, int kernel_id, double* total_ms, long long* launches);
int obtg_reset_kernel_stats(obtg_ctx*);
const char* obtg_kernel_name(int kernel_id);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* OBTG_H */
