// Internal declarations shared by the translation units of libobtg_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/obtg.h"

namespace obtg {

// ---- Specialised control-point counts (degree + 1).  The batch kernels are templates on the count; these lists are the
// ONLY place that says which counts are instantiated -- every dispatch below expands one of them, so a new degree is one
// entry here (round 5: 9 = the degree-8 drivers, Examples/DubinsCarTimeOptimal.py:72, DubinsCarExample2.py:83).
//   OBTG_NC_SEP : separation / speed rows (k_normsq_elev, k_tsep_fd, k_one_vs_many; 2-D and 3-D), planar hull sweep
//   OBTG_NC_DYN : angular rate (k_dynamics*), 3-D sweeps, the one-launch steps (k_pair_sweep*, k_step_fd_structured)
//   OBTG_NC_ELEV: DEG_ELEV > 0 separation + dynamics in one launch (k_sep_dynamics_elev) and the elevated structured step
#define OBTG_NC_ELEV(X) X(4) X(6) X(8) X(9) X(11)
#define OBTG_NC_DYN(X)  OBTG_NC_ELEV(X) X(16)
#define OBTG_NC_SEP(X)  OBTG_NC_DYN(X) X(21)
#define OBTG_NC_EQ_(N) || nc == N
//   OBTG_NC_ANG_LIST : the true angular-rate rows' fused kernels (k_ang_true_min; 2-D), the counts of OBTG_NC_SEP that build
//                      without scratch
#define OBTG_NC_ANG_LIST(X) OBTG_NC_DYN(X) X(21)
//   OBTG_NC_ACCEL_LIST : the true acceleration rows' fused value-and-blocks kernels (k_accel_true_min<.., true>; 2-D and 3-D),
//                      the counts of OBTG_NC_SEP that build without scratch; the others form their blocks
//                      in a launch of their own
#define OBTG_NC_ACCEL_LIST(X) OBTG_NC_DYN(X) X(21)
//   OBTG_NC_JERK_LIST : the true jerk rows' fused value-and-blocks kernels (k_jerk_true_min<.., true>; 2-D and 3-D), the counts
//                      of OBTG_NC_SEP that build without scratch; the others form their blocks in a launch
//                      of their own
#define OBTG_NC_JERK_LIST(X) OBTG_NC_DYN(X) X(21)
//   OBTG_NC_CURV_LIST : the curvature rows' in-register kernels (k_curv_true_min; 2-D), the counts of OBTG_NC_ANG_LIST that
//                      build without scratch; the others take the workspace route
#define OBTG_NC_CURV_LIST(X) OBTG_NC_DYN(X) X(21)
//   OBTG_NC_SCURV_LIST: the space-curvature rows' in-register kernels (k_scurv_true_min; 3-D), the counts that build without
//                      scratch with four registers per coefficient (21 does not); the others take the workspace route
#define OBTG_NC_SCURV_LIST(X) OBTG_NC_DYN(X)
//   OBTG_NC_PROX_LIST : the proximity rows' fused kernels (k_prox_true: values, values and blocks, the rows; 2-D and 3-D), the
//                      counts of OBTG_NC_SEP that build without scratch; the others take the workspace route
#define OBTG_NC_PROX_LIST(X) OBTG_NC_DYN(X) X(21)
static inline bool nc_in_sep(int nc)  { return false OBTG_NC_SEP(OBTG_NC_EQ_); }
static inline bool nc_in_dyn(int nc)  { return false OBTG_NC_DYN(OBTG_NC_EQ_); }
static inline bool nc_in_elev(int nc) { return false OBTG_NC_ELEV(OBTG_NC_EQ_); }

constexpr int kWave = 64;
constexpr int kMdMaxCurveK = 32;     // control points per curve of the branch & bound searches (gjk_kernels.hip: kMdMaxK), for the host's checks
constexpr int kNeedBatch = 1077;      // internal launcher result: "this kernel needs the finite-difference batch in memory"
constexpr int kMaxGenericLen = 1024;  // longest Bernstein coefficient vector of the generic kernels

// ---------------------------------------------------------------- host-side tables (tables.cpp)
double binom(int n, int k);                         // scipy.special.binom on integers (0 outside range)
std::vector<double> binom_row(int n);               // C(n, 0..n)
std::vector<double> folded_product_weights(int n, int dim);  // [2n+1][n+1], see bern_kernels.hip
std::vector<double> elev_table_frag(int L_in, int R);   // the same matrix as v_mfma_f64_16x16x4 B fragments: [NT][KS][64]
std::vector<double> elev_table_T_ld(int L_in, int R);   // dense, transposed, zero padded: [L_in+R][L_in] (bit-equal to the fragments)
struct DdTables { int wn, w2n, w22n, ratio, row4, sc4; };     // offsets (doubles) of angrate_dd_tables' parts
DdTables angrate_dd_tables(int n, int R, std::vector<double>& t);
std::vector<double> elev_conv_tables(int L_in, int R);  // scale | padded C(R,.) | 1/C(N+R,.)
std::vector<double> elev_conv_padded(int L_in, int R, int extra, bool normalise, bool with_inv);

// ---------------------------------------------------------------- device buffers
// Device buffer that grows.  A staging buffer of the host entry points (`io`) serves requests of up to kZeroCopyBytes
// from mapped pinned HOST memory instead: the kernel reads its few hundred bytes of control points and writes its
// results (up to one 64-vehicle row of separation rows, 339 KB) across PCIe itself, and a one-row SLSQP callback is memcpy + ONE launch + synchronize + memcpy instead
// of two DMA transfers around the launch (tools/latency_probe.py: 30 -> 15 us per call at Example1's size).
constexpr size_t kZeroCopyBytes = 512u << 10;
struct DevBuf {
    void* p = nullptr;          // the address kernels use for the current request
    size_t cap = 0;             // capacity behind p
    bool io = false;            // a staging buffer of the host entry points (set once, at context creation)
    bool on_host = false;       // p is the mapped host block
    void* dev = nullptr;        // device allocation (grows, never shrinks)
    size_t dev_cap = 0;
    void* host = nullptr;       // CPU address of the mapped block (kZeroCopyBytes), host_dev its device address
    void* host_dev = nullptr;
    bool host_failed = false;
    // returns OBTG_* code.  zero_copy: this request may be served from the mapped host block -- only for data a kernel
    // touches once (control points staged to LDS or registers, results written once)
    int reserve(size_t bytes, bool zero_copy = false);
    void release();
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct KernelStat {
    double ms = 0.0;
    long long launches = 0;
};

// obtg_ctx::ws_misc: every slot by name.  The first name of an index is what the batched pair searches of capi.cpp
// (obtg_gjk_pairs .. obtg_coll_check2poly) keep there; the names under it are the same buffer as the other calls use it.  A
// host call leaves the device idle, so nothing lives from one entry point to the next: only uses inside ONE call can collide.
// The rule the code relies on: an entry point holds (from its reservation to its last download) only names WITHOUT the L; a
// launcher takes only WS_L_* names, and only those whose index none of its calling entry points holds across the call.
// The chains that are two deep, by index:
//   obtg_temporal_sep_true_min[_jac], obtg_speed_true_min[_jac], obtg_ang_rate_true_min[_jac] hold 4 (WS_STATUS: true_min_host)
//     -> true_min_chain takes 6 (WS_L_TSTAR: only with blocks in a launch of their own for a _dev caller that wants no t_star;
//        the host call's is in ws_out) and 7 (WS_L_ROWS: degrees off the fast-kernel list) across the family's R = 0 rows
//        launcher, launch_bern_extrema and launch_true_min_envelope, which take none
//   obtg_temporal_sep_active holds 4 (WS_STATUS) -> launch_temporal_sep takes 7 (WS_L_ROWS: the any-degree selection)
//   host_deriv_obj           holds none -> launch_deriv_energy_obj takes 3, 6, 4 (launch_bern_diff and launch_speed take none)
//   obtg_bern_extrema        holds 3 (WS_INFO) -> launch_bern_extrema takes none
//   obtg_gjk_swarm           holds 3 (WS_INFO) -> launch_gjk_swarm takes 7 (WS_L_CHANGED) and, under OBTG_TIMELINE, 6
//   obtg_bern_arc_length     holds 3 (WS_INFO) -> launch_arc_length takes none
//   obtg_arc_length_obj      holds 4 (WS_STATUS) -> launch_arc_length_obj takes 7 (WS_L_ROWS: the vehicles' lengths and status)
//   obtg_curvature_true_min[_jac] are true_min_host / true_min_chain calls like the first line's (the workspace rows are num and den)
//   obtg_proximity_true[_jac] hold 4 (WS_STATUS: nodes | status, proximity_true_host) -> proximity_chain takes 6 and 7 as true_min_chain does
//   obtg_bern_curvature      holds 4 (WS_STATUS) -> bern_curvature_chain takes 7 (WS_L_ROWS: the curves' num and den rows)
enum WsSlot {
    WS_POLY_OFF = 0,      // int[n_poly + 1]: polygon offsets
    WS_CURVE_OFF = 0,     //   int[n_curves + 1]: control-point offsets of obtg_min_dist_mixed's curves
    WS_ARG_A = 0,         //   first small operand beside ws_in / ws_in2: one_span (obtg_one_vs_many_min_spans[_dev]), pert_row (obtg_temporal_sep_fd), span (obtg_bern_restrict)
    WS_PAIR_A = 1,        // int[n_pairs]: first operand of every pair
    WS_ARG_B = 1,         //   second small operand: many_span, pert_col, target (the same three calls)
    WS_PAIR_B = 2,        // int[n_pairs]: second operand
    WS_INFO = 3,          // int[4 n_pairs]: counters and status of a curve search; flag | n_support or iters | status of a GJK call; nodes | status of obtg_bern_extrema
    WS_L_DIFF_A = 3,      //   launch_deriv_energy_obj: derivative passes, even ones
    WS_TRACE = 4,         // obtg_gjk_pairs: the support trace
    WS_STATUS = 4,        //   int per value: the row indices of obtg_temporal_sep_active, the status of the true-minimum row families (true_min_host)
    WS_L_SPEED = 4,       //   launch_deriv_energy_obj: the speed-style rows before their sum
    WS_STACK = 5,         // frame stacks (the frontiers of the robust searches)
    WS_OUT_TF = 5,        //   the d/dtf output of obtg_speed_jac, obtg_ang_rate_jac, obtg_deriv_energy_grad
    WS_QUEUE = 6,         // work-queue counter, and behind it obtg_min_dist's pair order
    WS_L_DIFF_B = 6,      //   launch_deriv_energy_obj: derivative passes, odd ones
    WS_L_TSTAR = 6,       //   true_min_chain: t_star between the value launches and the envelope launch, when the caller wants none
    WS_L_TIMELINE = 6,    //   TimelineDump (gjk_kernels.hip; the one-launch sweeps, which no holder of WS_QUEUE calls)
    WS_L_ROWS = 7,        // whole rows under a reduction: launch_temporal_sep's any-degree selection, true_min_chain's R = 0 rows,
                          //   launch_arc_length_obj's per-vehicle lengths and status
    WS_L_CHANGED = 7,     //   launch_gjk_swarm's de-duplicated sweep: which objects differ from row 0
    WS_COUNT = 8,
};

}  // namespace obtg

struct obtg_ctx {
    int device = 0;
    int n_cus = 256;          // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    int n_veh = 0, dim = 0, deg = 0, R = 0, n_obs = 0;
    int n_obj = 0, n_pairs = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string last_error;

    // resident tables
    obtg::DevBuf d_pairs;     // int2[n_pairs]  (i, j) lexicographic, i < j < n_obj
    obtg::DevBuf d_obs;       // double[n_obs][dim]
    obtg::DevBuf d_w2;        // folded product weights for (deg, dim)
    obtg::DevBuf d_Tt;        // elevation (2*deg -> 2*deg+R) as convolution tables (elev_conv_tables)
    obtg::DevBuf d_Td;        // the same elevation as a dense transposed matrix (elev_table_T_ld): rows for the lane-per-item chains
    obtg::DevBuf d_Tf;        // ... and as matrix-instruction B fragments (elev_table_frag): the batch kernels
    obtg::DevBuf d_ang_w2n, d_ang_w22n, d_ang_wn;  // angular-rate fast path weights
    obtg::DevBuf d_ang_rows;  // the true angular-rate rows' separable product weights: C(n, .)[n+1], 1 / C(2n, .)[2n+1] (dim 2 and 3, n <= 31)
    obtg::DevBuf d_curv_tab;  // obtg_bern_curvature: the same table for the degree of the last call's curves (curv_tab_n)
    int curv_tab_n = -1;
    obtg::DevBuf d_ang_T4;    // angular rate, R > 0: elevation 4*deg -> 4*(deg+R) as a scaled convolution (elev_conv_padded)
    obtg::DevBuf d_ang_cv2;   // the same for the speed rows, 2*deg -> 2*deg+R, with the 1/C(2n+R, k) row
    bool ang_elevate_first = false;   // true: the reference's order (elevate, then products at degree n+R; generic kernel)
    bool ang_exact = false;           // obtg_ctx_set_ang_rate_order(2): the default order, then the rows of near-stop vehicles again in
                                      // double-double (k_angrate_dd); tables and the flag list below, made on first use
    obtg::DevBuf d_ang_dd, d_ang_flags;
    // exact Jacobians (jac_kernels.hip): G = elevation o folded product for (deg, R), its row sums, and for dim 2 the angular
    // rate's product / elevation weights from offset jac_off_ang (-1: not this shape); made on first use, per R
    obtg::DevBuf d_jac;
    int jac_R = -1;
    long long jac_off_ang = -1;
    obtg::DdTables ang_dd_off{};
    int ang_dd_R = -1;
    // obtg_ctx_set_second_speed_bound: every dynamics pass that writes speed rows also writes the other bound's rows
    struct { double bound = 0.0; int is_max = 0; double* d_out = nullptr; } speed2;
    // obtg_ctx_set_keep_in: the region's half-spaces and the (vehicle, face) items of the keep-in rows; keep_P == 0: none set
    obtg::DevBuf d_keep_H;    // double[keep_F][dim + 1]: (a, b) of a . p <= b
    obtg::DevBuf d_keep_VF;   // int2[keep_P]
    int keep_F = 0, keep_P = 0;
    // obtg_ctx_set_keep_out: the obstacles' faces, the face ranges of the obstacles and the (vehicle, obstacle) items of the
    // keep-out rows; ko_P == 0: none set
    obtg::DevBuf d_ko_H;      // double[ko_F][dim + 1]: (a, b) of a . p <= b
    obtg::DevBuf d_ko_off;    // int[ko_O + 1]
    obtg::DevBuf d_ko_VO;     // int2[ko_P]
    int ko_F = 0, ko_O = 0, ko_P = 0;
    // the Euclidean metric (obtg_keep_out_euclid_*): host copies of H and obs_off, kept by obtg_ctx_set_keep_out, and what the
    // first Euclidean call after it makes of them (csrc/keepout_features.h): the normalised faces and the feature records
    // beside H on the device.  ko_eu_state 0: not made yet; 1: made; any other value: the code every Euclidean call answers
    std::vector<double> h_ko_H;
    std::vector<int> h_ko_off;
    obtg::DevBuf d_ko_Hn;     // double[ko_F][dim + 1]
    obtg::DevBuf d_ko_feat;   // double[features][7]: Gram^-1 (6) | the faces, a byte each
    obtg::DevBuf d_ko_foff;   // int[ko_O + 1]
    int ko_eu_state = 0;
    // obtg_ctx_set_keep_out_motion: the obstacles' offset curves; ko_motion false: none set (every obstacle stands still)
    obtg::DevBuf d_ko_Q;      // double: the [dim][m_o + 1] blocks, one after the other
    obtg::DevBuf d_ko_qoff;   // int[ko_O + 1], in control points
    obtg::DevBuf d_ko_T;      // double[ko_O]
    bool ko_motion = false;
    // obtg_ctx_set_pair_keep_out: the ONE separation region of the vehicle pairs and the pairs' (i, j) in lexicographic order;
    // pk_F == 0: none set.  The Euclidean tables as above: h_pk_H the host copy, pk_eu_state 0 / 1 / the code; pk_NF the records
    obtg::DevBuf d_pk_H;      // double[pk_F][dim + 1]
    obtg::DevBuf d_pk_IJ;     // int2[n_veh (n_veh - 1) / 2]
    obtg::DevBuf d_pk_Hn;     // double[pk_F][dim + 1]
    obtg::DevBuf d_pk_feat;   // double[pk_NF][7]
    std::vector<double> h_pk_H;
    int pk_F = 0, pk_NF = 0, pk_eu_state = 0;
    // obtg_ctx_set_proximity: the items (a, b, kind) and (rho, tau0, tau1) of the proximity rows and the family's own points;
    // prox_P == 0: none set
    obtg::DevBuf d_prox_items;   // int[prox_P][3]
    obtg::DevBuf d_prox_par;     // double[prox_P][3]
    obtg::DevBuf d_prox_pts;     // double[prox_Q][dim]
    int prox_P = 0, prox_Q = 0;
    std::vector<int> h_pairs; // host copy of the pair table (2 ints per pair)
    std::vector<int> h_tiles; // row-window tiles of the current (pair_begin, pair_count)
    obtg::DevBuf d_tiles;
    int tiles_begin = -1, tiles_count = -1;
    std::vector<double> h_binrows;
    obtg::DevBuf d_binrows;   // concatenated binomial rows for the generic kernels
    std::vector<int> binrow_off;   // offset of row C(n, .) inside d_binrows, -1 if absent
    int tables_R = -1;

    // swarm GJK state
    obtg::DevBuf d_poly_pts;  // SoA per polygon: x[K], y[K], z[K]
    obtg::DevBuf d_poly_off;  // int[n_poly+1]
    int n_poly = 0, n_poly_pts = 0, max_poly_K = 0;
    bool polys_planar = true;   // every registered polygon vertex has z == 0
    bool fd_dedup = false;      // reuse row 0's GJK results for bit-identical hull pairs
    bool true_min_jac_fused = true;   // OBTG_TRUE_MIN_JAC_FUSED=0: obtg_temporal_sep_true_min_jac, obtg_speed_true_min_jac and obtg_ang_rate_true_min_jac take the two-launch form on every shape
    bool fd_view_structured = true;   // obtg_ctx_set_fd_view_structured: the one-call sweep of a view takes the structured step where it applies
    obtg::DevBuf d_hp_a, d_hp_b;  // hull pair list
    obtg::DevBuf d_vp_off, d_vp_idx;   // per vehicle: the positions of the hull pairs that contain it (CSR; structured FD step)
    // Structured FD step, rows handed out at run time (gjk_kernels.hip StructuredParams::tickets): two banks of
    // struct_ticket_stride counters, one per separation group and then one per hull-pair chunk.  Both are zero at creation;
    // a launch draws from bank struct_ticket_bank and zeroes the other, which the next launch draws from -- the bank
    // changes only once a launch is on the stream, so a call that failed before that leaves the next one a zero bank.
    // struct_ticket_layout: (groups, chunks) of the last launch; another layout zeroes both banks first.
    obtg::DevBuf d_struct_tickets;
    int struct_ticket_bank = 0, struct_ticket_stride = 0, struct_ticket_layout[2] = { 0, 0 };
    std::vector<int> h_hp_a, h_hp_b;   // host copy (tile-major chunking of large rows)
    obtg::DevBuf d_tile_chunk_off, d_tile_order, d_tile_pslots, d_tile_cobj_off, d_tile_cobjs, d_tile_ij;
    bool tile_ts_ok = false;  // every chunk's tile origin is recorded and the hull pair list holds every vehicle pair: the tiled
                              // sweep can write the temporal-separation rows of its tiles (one-launch pair sweep of large rows)
    int tile_a = 8;           // tile height the chunks were cut for
    bool tile_valid = false;
    int tile_n_chunks = 0, tile_max_objs = 0, tile_max_pairs = 0;
    int n_hull_pairs = 0;
    bool hull_pairs_set = false;  // obtg_ctx_set_hull_pairs since the last obtg_ctx_set_polygons
    obtg::DevBuf d_gjk_len[2];   // per-pair support-scan counts of the last planar sweep (scheduling history)
    bool gjk_history = true;
    int gjk_len_cur = 0, gjk_len_rows = 0;   // buffer holding the latest counts, and how many rows of them

    // Virtual finite-difference batch (obtg_*_fd_dev): rows are formed on the fly from ONE row of control points,
    // row b >= 1 = Y0 with its (b-1)-th free control point advanced by h (exactly obtg_fd_batch_dev's rows).
    // `fd` is set for the duration of ONE launcher call; launchers whose kernel cannot form the rows return
    // obtg::kNeedBatch before launching anything and the caller materialises the batch (once per view) instead.
    struct FdView { const double* Y0 = nullptr; double h = 0.0; int fixed = 0; int row0 = 0; } fd;       // row0: batch row of local row 0
    struct { const double* Y0 = nullptr; double h = 0.0; int fixed = 0; int B = 0; int row0 = 0; bool materialised = false; } view;   // obtg_fd_view_begin[_rows] .. _end
    obtg::DevBuf ws_fd;                   // the view's batch, written only when some kernel needs it

    // scratch for host-buffer entry points
    // (ws_misc: every slot has a name and an owner rule, obtg::WsSlot above)
    obtg::DevBuf ws_in, ws_in2, ws_out, ws_misc[obtg::WS_COUNT];
    // obtg_min_dist: node counts of the previous evaluation of the SAME pair list (signature = count + hash of the lists):
    // the next evaluation hands its pairs to the worker waves in descending order of them (k_min_dist_wave)
    // (up to four lists, least recently used dropped: a driver alternates the constraint's list with its Jacobian's longer one)
    struct MdHist { unsigned long long sig; std::vector<int> nodes; };
    std::vector<MdHist> md_hist;
    void* ring = nullptr;                 // pinned staging ring for pageable caller buffers (capi.cpp h2d / d2h)
    hipEvent_t ring_ev[4] = {};
    bool ring_pending[4] = {};            // slot's event recorded and not waited for yet
    int ring_next = 0;                    // next slot of the rotation

    // instrumentation
    bool profiling = false;
    int profile_period = 1;               // events on every n-th eligible launch of a kernel id
    long long profile_seen[OBTG_K_END] = {};
    unsigned profile_mask = ~0u;          // kernel ids that get events while profiling
    std::vector<hipEvent_t> event_pool;   // recycled events
    obtg::KernelStat stats[OBTG_K_END];
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending_events;
};

namespace obtg {

int set_error(obtg_ctx* c, hipError_t e, const char* where);
#define OBTG_HIP(c, call)                                                   \
    do {                                                                    \
        hipError_t e__ = (call);                                            \
        if (e__ != hipSuccess) return ::obtg::set_error((c), e__, #call);   \
    } while (0)

// bracket a launch with events when profiling.  ext = true: the events are NOT recorded on the stream; the launch itself
// carries them (launch_timed -> hipExtLaunchKernelGGL: the dispatch's own start / stop timestamps, no barrier packets
// around the kernel, so events on every launch do not stretch the step).
struct ScopedKernelTimer {
    obtg_ctx* c;
    int id;
    bool ext;
    hipEvent_t a = nullptr, b = nullptr;
    ScopedKernelTimer(obtg_ctx* c_, int id_, bool ext_ = false);
    ~ScopedKernelTimer();
};
void flush_pending_events(obtg_ctx* c);

int ensure_tables(obtg_ctx* c);
int binrow_offset(obtg_ctx* c, int n);  // ensures row C(n,.) is resident; returns offset (doubles)

// ---------------------------------------------------------------- launchers (bern_kernels.hip)
// comm.cpp: this rank's block of the per-pair minima (contiguous balanced partition of the lexicographic pair list), ONE
// RCCL all-gather on the context's stream, rows [B][P] on every rank
int comm_gather_pair_minima(::obtg_comm* m, obtg_ctx* c, const double* dY, int B, double max_sep, double* d_min_all);
int launch_temporal_sep(obtg_ctx* c, const double* dY, int B, double max_sep, int pair_begin,
                        int pair_count, bool min_only, double* d_out, int sel_k = 0, int* d_sel_idx = nullptr);
struct NsParams;
// What launch_gjk_swarm may fold into its 3-D sweep launch (k_pair_sweep_3d): the row's temporal-separation block and,
// when d_out_speed is set, its speed rows.  did_* report what the launch took over.
struct SweepFold {
    double max_sep = 0.0;
    double* d_out_sep = nullptr;
    const double* d_tf = nullptr;
    double speed_bound = 0.0;
    int speed_is_max = 1;
    double* d_out_speed = nullptr;
    double max_rate = 0.0;          // planar rows: with d_out_ang the speed / angular-rate groups may join the sweep's grid
    double* d_out_ang = nullptr;
    bool did_sep = false, did_speed = false, did_dynamics = false;
};
int plan_temporal_sep(obtg_ctx* c, const double* dY, int B, int pair_begin, int pair_count, double* d_out, NsParams& p);
size_t temporal_sep_lds_bytes(const obtg_ctx* c, NsParams& p, size_t budget);
// speed (optional): the speed rows of the same batch, folded into the launch where a kernel does that (3-D sweeps);
// speed->did_speed tells the caller whether they still have to be launched
int launch_pair_sweep(obtg_ctx* c, const double* dY, int B, double max_sep, double* d_out_sep, int max_iter,
                      int md_cap, int* d_flag, double* d_p1, double* d_p2, double* d_dist, int* d_nsup, int* d_status,
                      SweepFold* speed = nullptr);
int launch_step_fd_structured(obtg_ctx* c, int B, double max_sep, double* d_out_sep, int max_iter, int md_cap, int* d_flag,
                              double* d_p1, double* d_p2, double* d_dist, int* d_nsup, int* d_status, SweepFold* speed);
int launch_temporal_sep_fd(obtg_ctx* c, const double* dY0, int n_pert, const int* d_prow, const int* d_pcol,
                           const double* d_pval, double max_sep, double* d_out, int min_only = 0, int fd_row0 = 0,
                           int fd_fixed = 0, double fd_h = 0.0);
int launch_one_vs_many_min(obtg_ctx* c, const double* d_one, int B, const double* d_many, int K, double max_sep, double* d_out);
int launch_one_vs_many_min_spans(obtg_ctx* c, const double* d_one, const double* d_one_span, int B, const double* d_many,
                                 const double* d_many_span, int K, double max_sep, double no_overlap, double* d_out);
int launch_bern_restrict(obtg_ctx* c, const double* d_in, int rows, int n, const double* d_span, const double* d_target, double* d_out);
int launch_speed(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, int is_max,      // deriv 2: the acceleration rows, 3: the jerk rows
                 double* d_out, int deriv = 1);
void speed_sign_offset(double bound, int is_max, double& sign, double& offset);    // the output transform of the speed rows
int launch_ang_rate(obtg_ctx* c, const double* dY, const double* d_tf, int B, double max_rate,
                    double* d_out);
// DEG_ELEV > 0, planar: separation rows + speed / angular-rate rows in one launch; OBTG_ERR_UNSUPPORTED = not this shape
int launch_sep_dynamics_elev(obtg_ctx* c, const double* dY, int B, double max_sep, double* d_out_sep, const SweepFold& f);
int launch_dynamics(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, int is_max,
                    double max_rate, double* d_out_speed, double* d_out_ang);
int launch_fd_batch(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int B, double* dY, int row0 = 0);   // rows row0 .. row0 + B - 1 of the batch
struct AngParams;
void second_speed_rows(const obtg_ctx* c, AngParams& p);    // the second speed bound's output and offset of a dynamics pass, when one is set
bool dynamics_fd_on_the_fly(const obtg_ctx* c, bool want_ang);
int ang_rate_order_in_effect(obtg_ctx* c);
bool bernstein_fd_on_the_fly(const obtg_ctx* c);      // the separate temporal-separation / speed kernels form a view's rows themselves
// What the sweep launchers of gjk_kernels.hip will do, asked before anything is launched.  Each is a question put to the plan
// its launcher executes (pair_sweep_plan for launch_pair_sweep, step_fd_structured_plan for launch_step_fd_structured): no
// condition is written a second time here or in capi.cpp.
bool pair_sweep_is_one_launch(const obtg_ctx* c);           // launch_pair_sweep of a large batch is the one-launch planar sweep (which forms a view's rows itself); touches nothing
bool constraint_sweep_is_one_launch(obtg_ctx* c, int B);    // launch_pair_sweep of B rows, every dynamics output wanted, is ONE launch (one-launch planar or tiled, dynamics
                                                            // groups folded in); may build what that launch needs (tables, the tiled form's chunk tables)
int sweep_shape_query(obtg_ctx* c, int B, int which, bool want_dyn, int out[8]);      // obtg_sweep_shape: the plans' form and grid; launches nothing
bool step_fd_structured_supported(obtg_ctx* c);             // launch_step_fd_structured has a kernel for this context (given all outputs); launches nothing
int launch_bern_elev(obtg_ctx* c, const double* d_in, int rows, int n, int R, double* d_out);
int launch_bern_diff(obtg_ctx* c, const double* d_in, int rows, int n, double T, double* d_out);
int launch_bern_split(obtg_ctx* c, const double* d_in, int rows, int n, double z, double* d_left, double* d_right);
int launch_bern_eval(obtg_ctx* c, const double* d_cpts, int rows, int n, const double* d_tau, int n_tau, double t0, double tf,
                     double* d_out);
int launch_bern_mul(obtg_ctx* c, const double* d_a, const double* d_b, int rows, int m, int n,
                    double* d_out);
int launch_bern_normsq(obtg_ctx* c, const double* d_x, int d, int n, double* d_out);
int launch_euclidean_obj(obtg_ctx* c, const double* dY, int B, double* d_out);
int launch_deriv_energy_obj(obtg_ctx* c, const double* dY, const double* d_tf, double tf0, int B, int order, double* d_out);

// ---------------------------------------------------------------- launchers (jac_kernels.hip): exact derivatives, layouts in obtg.h
int launch_temporal_sep_jac(obtg_ctx* c, const double* dY, int B, double* d_out);
int launch_speed_jac(obtg_ctx* c, const double* dY, const double* d_tf, int B, int is_max, double* d_out, double* d_out_tf);
int launch_ang_rate_jac(obtg_ctx* c, const double* dY, const double* d_tf, int B, double* d_out, double* d_out_tf);
int launch_euclidean_grad(obtg_ctx* c, const double* dY, int B, double* d_out);
int launch_deriv_energy_grad(obtg_ctx* c, const double* dY, const double* d_tf, int B, int order, double* d_out, double* d_out_tf);

// ---------------------------------------------------------------- launchers (gjk_kernels.hip)
int launch_gjk_pairs(obtg_ctx* c, const double* d_soa, const int* d_off, const int* d_pa,
                     const int* d_pb, int n_pairs, int max_iter, int md_cap, int* d_flag,
                     double* d_p1, double* d_p2, double* d_dist, short* d_trace, int trace_cap,
                     int* d_nsup, int* d_status, bool planar);
int launch_gjk_swarm(obtg_ctx* c, const double* dY, int B, int max_iter, int md_cap, int* d_flag,
                     double* d_p1, double* d_p2, double* d_dist, int* d_nsup, int* d_status, SweepFold* fold = nullptr);
int launch_min_dist(obtg_ctx* c, const double* d_curves, int K, const int* d_pa, const int* d_pb,
                    int n_pairs, double eps, int max_iter, int md_cap, int max_depth, int max_nodes,
                    double* d_stack, double* d_res, int* d_info, const int* d_order = nullptr, int* d_queue = nullptr,
                    bool planar = false);      // planar: every control point of every curve has z == 0 (the caller has looked)
// curves of different degree: curve i is [3][K_i] at d_cpts + 3 * d_off[i]; kt_max: the largest KA + KB among the pairs
int launch_min_dist_mixed(obtg_ctx* c, const double* d_cpts, const int* d_off, int kt_max, const int* d_pa, const int* d_pb,
                          int n_pairs, double eps, int max_iter, int md_cap, int max_depth, int max_nodes, double* d_stack,
                          double* d_res, int* d_info, const int* d_order, int* d_queue, bool planar);
int launch_min_dist_robust(obtg_ctx* c, const double* d_curves, int K, const int* d_pa, const int* d_pb, int n_pairs,
                           double eps, int max_nodes, int max_level, int cap, double* d_frontier, double* d_res, int* d_info);
int launch_min_dist2poly(obtg_ctx* c, const double* d_curves, int K, const double* d_soa,
                         const int* d_off, const int* d_pc, const int* d_pp, int n_pairs, double eps,
                         int max_iter, int md_cap, int max_depth, int max_nodes, double* d_stack,
                         double* d_res, int* d_info, int max_poly_K, bool planar = false);     // planar: curves AND polygons have z == 0 throughout
int launch_gjk_true_pairs(obtg_ctx* c, const double* d_soa, const int* d_off, const int* d_pa, const int* d_pb, int n_pairs,
                          double eps, int max_iter, int* d_flag, double* d_p1, double* d_p2, double* d_dist, double* d_lower,
                          int* d_iters, int* d_status);
int launch_min_dist2poly_robust(obtg_ctx* c, const double* d_curves, int K, const double* d_soa, const int* d_off,
                                const int* d_pc, const int* d_pp, int n_pairs, double eps, int max_nodes, int max_level,
                                int cap, int max_poly_K, double* d_frontier, double* d_res, int* d_info);
// x**2 as Python forms it for the constraint offsets (optimization.py:343, 384, 422, 459: maxSep**2, minSpeed**2, maxSpeed**2,
// maxAngRate**2 on Python floats): the host libm's pow(x, 2.0), which is not always x * x (tables.cpp)
double square_as_python(double x);
double cube_as_python(double x);       // x**3 likewise (bezier.py:1468: eps**3)
size_t min_dist_stack_doubles(const obtg_ctx* c, int K, int max_depth, int n_pairs, bool planar);   // whole launch, the form launch_min_dist runs
size_t min_dist_mixed_stack_doubles(const obtg_ctx* c, int kt_max, int max_depth, int n_pairs);   // whole launch, as launch_min_dist_mixed lays it out
size_t min_dist2poly_stack_doubles(int K, int max_depth, int n_pairs, int max_poly_K, bool planar);   // whole launch, the form launch_min_dist2poly runs
int min_dist_workers(const obtg_ctx* c, int n_pairs, size_t lds_per_wave, int waves_per_simd);   // worker waves of the queue forms

// ---------------------------------------------------------------- launchers (coll_kernels.hip): _collCheckBez2Bez / _collCheckBez2Poly
bool coll_check_supported(int K, int max_poly_K);      // at most 16 control points per curve and 16 vertices per polygon
size_t coll_check_stack_doubles(const obtg_ctx* c, int K, int n_pairs, bool poly, bool planar);      // whole launch: a frame stack per worker wave of the grid that `planar` launches
int launch_coll_check(obtg_ctx* c, const double* d_curves, int K, const int* d_pa, const int* d_pb, int n_pairs, double eps,
                      int max_iter, int md_cap, int max_nodes, double* d_stack, double* d_res, int* d_info, int* d_queue,
                      bool planar);      // planar: every control point of every curve has z == +0 (the caller has looked)
int launch_coll_check2poly(obtg_ctx* c, const double* d_curves, int K, const double* d_soa, const int* d_off, const int* d_pc,
                           const int* d_pp, int n_pairs, int max_iter, int md_cap, int max_nodes, double* d_stack, double* d_res,
                           int* d_info, int* d_queue, int max_poly_K, bool planar);      // planar: curves AND polygons

// ---------------------------------------------------------------- launchers (extrema_kernels.hip): true Bernstein extrema
bool bern_extrema_supported(int K);                    // 1 <= K <= 64: a row is a row of lanes
int launch_bern_extrema(obtg_ctx* c, const double* d_c, long M, int K, int want_max, double eps_rel, double eps_abs,
                        int max_nodes, double* d_val, double* d_t, double* d_bound, int* d_nodes, int* d_status,
                        int kernel_id = OBTG_K_BERN);     // every output but d_val nullable
// A true-minimum row family (obtg_temporal_sep_true_min[_jac], obtg_speed_true_min[_jac], obtg_ang_rate_true_min[_jac], obtg_accel_true_min[_jac], obtg_jerk_true_min[_jac]) as the host path sees it: what one
// call of the family contributes beyond the arguments every family has.  On the device the family is a struct of
// extrema_kernels.hip (TsepRows, SpeedRows, AngRows, AccelRows, JerkRows), found by `kind`.
enum RowKind { ROWS_TSEP, ROWS_SPEED, ROWS_ANG, ROWS_ACCEL, ROWS_JERK, ROWS_CURV, ROWS_SCURV, ROWS_KEEP_IN };
struct RowFamily {
    RowKind kind;
    int items;                  // per batch row: n_pairs | n_veh | 2 n_veh
    int kernel_id;              // every launch of the call is timed under it
    double sign, offset;        // the output transform of its rows
    const double* d_tf;         // [B], device; null where the rows have no time span
    // its full rows at R = 0 from the any-degree kernel, [B][items][row_len], whatever the context's DEG_ELEV is: the launch
    // a context with R = 0 makes, bit for bit; the context is not touched
    int (*rows_r0)(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double* d_out);
    double w = 0.0;             // ROWS_ANG: the bound on |angular rate| (it enters the coefficients, not the output transform);
                                // ROWS_CURV: max_curv
    // the search of the workspace rows rows_r0 wrote; null: launch_bern_extrema, one row per item.  ROWS_CURV: a vehicle's two
    // rows are num and den and serve both of its items, so the workspace has as many rows as the batch has items
    int (*search)(obtg_ctx* c, const RowFamily& f, const double* d_rows, long items, double eps_rel, int max_nodes, double* d_out,
                  double* d_t, int* d_status) = nullptr;
    int ws_rows = 1;            // workspace rows per item (ROWS_SCURV: 4 -- wx, wy, wz, den)
    int row_len = 0;            // coefficients of a row at R = 0 -- what a workspace row holds and what the search sees; 0: 2 deg + 1
                                // (ROWS_KEEP_IN: deg + 1, the polynomial is linear in the curve)
};
static inline int row_len(const RowFamily& f, int deg) { return f.row_len ? f.row_len : 2 * deg + 1; }
RowFamily tsep_row_family(const obtg_ctx* c, double max_sep);                                         // bern_kernels.hip
RowFamily speed_row_family(const obtg_ctx* c, const double* d_tf, double bound, int is_max);
RowFamily accel_row_family(const obtg_ctx* c, const double* d_tf, double bound);                      // q = bound^2 - (d/2)|c''|^2
RowFamily jerk_row_family(const obtg_ctx* c, const double* d_tf, double bound);                       // q = bound^2 - (d/2)|c'''|^2
RowFamily ang_row_family(const obtg_ctx* c, const double* d_tf, double max_rate);                     // extrema_kernels.hip
// The keep-in family (ROWS_KEEP_IN): the context's region (obtg_ctx_set_keep_in), one item per listed (vehicle, face), rows of
// deg + 1 coefficients, no time span; dim 2 or 3.  launch_keep_in_rows: obtg_keep_in's rows out[B][P][deg + R + 1], the R = 0
// coefficients elevated once per row (R = 0: the family's rows_r0), degree up to 31
RowFamily keep_in_row_family(const obtg_ctx* c);                                                      // bern_kernels.hip
int launch_keep_in_rows(obtg_ctx* c, const RowFamily& f, const double* dY, int B, int R, double* d_out);
// The keep-out rows (keepout_kernels.hip): min over t of the max over an obstacle's faces of a_f . c(t) - b_f, per item, in
// every form the family has -- ONE launcher over one argument struct; the host path on top of it is DESIGN.md 4.29.
// The outputs of a call as one named set: device pointers for the launcher, host pointers for the entry points (capi.cpp's
// column table walks it).  Every one but val is nullable; rel, jac and jac_tf null: the kernel skips those stores, the other
// outputs are the same bits either way.
struct KeepOutOutputs {
    double* val;            // [M]
    double* t;              // [M]
    int* face;              // [M][2]: the faces metric's active faces ...
    double* lam;            // [M]:    ... and the first one's weight
    int* faces3;            // [M][3]: the Euclidean metric's active set, -1 padded ...
    double* dir;            // [M][dim]: ... and the unit direction; they stand in for face and lam, which are then not written
    double* bound;          // [M]
    int* nodes;             // [M]
    int* status;            // [M]
    double* rel;            // [M][dim][K]: the relative control points (moving, pair)
    double* jac;            // [M][dim][K]
    double* jac_tf;         // [M] (moving)
};
// Items: with tables (VO_or_IJ set), item (b, k) of M = B P is batch row b of Y[B][n_veh dim][K] against entry k of the table --
// (vehicle, obstacle), obstacle o owning faces off[o] .. off[o + 1] - 1 of H (at most 16, the callers' check), or with `pair`
// the vehicles (i, j) against the ONE region H[F_all][dim + 1], 1 <= F_all <= 16.  Free curves (VO_or_IJ null): curve m of
// Y[M][dim][K] against faces 0 .. F_all - 1.  dim 2 or 3, 2 <= K <= 32.
//   euclid: H holds the NORMALISED faces, feat[.][7] the feature records, feat_off[O + 1] their ranges (pairs and free curves:
//           feat_off null, records 0 .. NF_all - 1; at most 128 records per obstacle);
//   moving: Q the obstacles' [dim][m_o + 1] blocks one after the other, q_off[O + 1] in control points (an empty run: the
//           obstacle stands still), T[O], tf[B]; free curves: Q[dim][Km] (Km <= K is the callers' check), r[M] or null (1).
// M <= 0 answers OBTG_OK; a shape out of range, or moving together with euclid or pair, OBTG_ERR_UNSUPPORTED.
struct KeepOutLaunch {
    int dim, K;
    long M;
    int n_veh, P, F_all;
    bool moving, euclid, pair;
    const double* Y;
    const double* H;
    const int* off;
    const int* VO_or_IJ;
    const double* feat;
    const int* feat_off;
    int NF_all;
    const double* Q;
    const int* q_off;
    const double* T;
    const double* tf;
    const double* r;
    int Km;
    double margin, eps_rel;
    int max_nodes;
    KeepOutOutputs out;
};
int launch_keep_out(obtg_ctx* c, const KeepOutLaunch& a);
// the angular-rate family's polynomials [B][n_veh][2][2 deg + 1] (obtg_ang_rate_poly; its rows_r0): dim 2, degree 1 .. 31
int launch_ang_rows(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double* d_out);
// The two curvature families, kind = ROWS_CURV (dim 2; two items, the sides, per vehicle; workspace rows num, den) or ROWS_SCURV
// (dim 3; one item per vehicle; workspace rows wx, wy, wz, den): degree 1 .. 31, no time span.  Their search is their own
// (extrema_kernels.hip curv_wave_search over the policies PlanarCurv and SpaceCurv3).
RowFamily curvature_row_family(const obtg_ctx* c, RowKind kind, double max_curv);
int launch_curvature_rows(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double* d_out);      // obtg_[space_]curvature_poly; their rows_r0
// free curves (obtg_bern_[space_]curvature): d_curves[n][dim][nc], d_tab = C(nc-1, .)[nc] | 1 / C(2 nc - 2, .)[2 nc - 1]; rows
// out[n][2 or 4][2 nc - 1]; the search of 2 n or n items -- free_curve: max_curv = 0 and the extrema themselves are written,
// planar k_max, t_max to d_val, d_t and k_min, t_min to d_val1, d_t1 ([n] each), space the maximum to d_val, d_t (d_val1, d_t1 null)
bool curvature_supported(int nc);                       // 2 <= nc <= 32
struct CurvShape { int np, sides, dim; };               // of a kind: polynomials per curve (den last), items per curve, coordinates
CurvShape curvature_shape(RowKind kind);
int launch_curv_rows(obtg_ctx* c, RowKind kind, const double* d_curves, const double* d_tab, long n_curves, int nc, double* d_out,
                     int kernel_id);
int launch_curv_search(obtg_ctx* c, RowKind kind, const double* d_rows, long items, int nc, double max_curv, int free_curve,
                       double eps_rel, int max_nodes, double* d_val, double* d_t, double* d_val1, double* d_t1, int* d_status,
                       int kernel_id);
// the fused form for the fast-kernel list's shapes, one launch; OBTG_ERR_UNSUPPORTED: go through the family's R = 0 rows.
// d_jac: with the envelope blocks [B][items][dim][deg+1]; d_jac_tf (nullable, speed): their d/dtf [B][items]
int launch_true_min(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double eps_rel, int max_nodes, double* d_out,
                    double* d_t, int* d_status, double* d_jac = nullptr, double* d_jac_tf = nullptr);
// the blocks alone from Y (tf) and the t_star of a value launch: any degree up to 31 (else OBTG_ERR_UNSUPPORTED)
// d_val: the rows' values of the value launch (ROWS_CURV reads them: a row that is its bound has a zero block)
int launch_true_min_envelope(obtg_ctx* c, const RowFamily& f, const double* dY, int B, const double* d_t, double* d_jac,
                             double* d_jac_tf, const double* d_val = nullptr);

// The proximity family (obtg_ctx_set_proximity's items; dim 2 or 3): its outputs [B][P], all but val nullable
struct ProxOut { double* val; double* t; double* bound; int* nodes; int* status; };
bool proximity_fused(const obtg_ctx* c);       // the shape has kernels that form the coefficients in registers (OBTG_NC_PROX_LIST)
// obtg_proximity_poly: g's coefficients out[B][P][2 deg + 1], degree up to 31 -- the fused kernels' own on their counts, the
// any-degree separation arithmetic on the others
int launch_proximity_rows(obtg_ctx* c, const double* dY, int B, double* d_out);
// one launch on the fused counts (d_jac: with the blocks [B][P][dim][deg+1]); OBTG_ERR_UNSUPPORTED: go through the rows
int launch_proximity_true(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, const ProxOut& o, double* d_jac);
// the search of launch_proximity_rows' rows: obtg_bern_extrema with want_max and the window per item
int launch_proximity_search(obtg_ctx* c, const double* d_rows, int B, double eps_rel, int max_nodes, const ProxOut& o);
// the blocks alone from Y and the t_star of a value launch
int launch_proximity_envelope(obtg_ctx* c, const double* dY, int B, const double* d_t, double* d_jac);

// ---------------------------------------------------------------- launchers (arclen_kernels.hip): true arc length
bool arc_length_supported(int dim, int K);             // 1 <= dim <= 3, 2 <= K <= 32
// M curves c[M][dim][K]; an eps_rel below the floor is raised to it; every output but d_len nullable, d_grad [M][dim][K]
int launch_arc_length(obtg_ctx* c, const double* d_c, long M, int dim, int K, double eps_rel, int max_nodes, double* d_len,
                      double* d_err, int* d_nodes, int* d_status, double* d_grad);
// the objective: the curves of dY[B] as the context shapes them, their lengths summed per row in vehicle order (takes
// WS_L_ROWS); d_status[B] and d_grad[B][n_veh * dim][deg + 1] nullable
int launch_arc_length_obj(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, double* d_out, int* d_status,
                          double* d_grad);

}  // namespace obtg
