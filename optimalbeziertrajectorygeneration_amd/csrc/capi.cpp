// C ABI of libobtg_hip.so (include/obtg.h): context, tables, host-buffer entry points.
// Compiled with hipcc (host code + HIP runtime API); the kernels live in bern_kernels.hip, gjk_kernels.hip,
// coll_kernels.hip, extrema_kernels.hip and jac_kernels.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "obtg_internal.h"
#include "keepout_features.h"

namespace obtg {

int DevBuf::reserve(size_t bytes, bool zero_copy)
{
    if (io && zero_copy && bytes <= kZeroCopyBytes && !host_failed) {
        if (!host) {
            if (hipHostMalloc(&host, kZeroCopyBytes, hipHostMallocMapped) != hipSuccess ||
                hipHostGetDevicePointer(&host_dev, host, 0) != hipSuccess) {
                (void)hipGetLastError();
                if (host) (void)hipHostFree(host);
                host = nullptr; host_dev = nullptr; host_failed = true;
            }
        }
        if (host) { p = host_dev; cap = kZeroCopyBytes; on_host = true; return OBTG_OK; }
    }
    on_host = false;
    if (bytes <= dev_cap && dev) { p = dev; cap = dev_cap; return OBTG_OK; }
    if (bytes == 0) bytes = 8;
    if (dev) { (void)hipFree(dev); dev = nullptr; dev_cap = 0; }
    p = nullptr; cap = 0;
    // grow geometrically to keep repeated host-entry calls from reallocating
    size_t want = bytes + bytes / 4;
    if (hipMalloc(&dev, want) != hipSuccess) {
        (void)hipGetLastError();
        if (hipMalloc(&dev, bytes) != hipSuccess) { dev = nullptr; return OBTG_ERR_OOM; }
        want = bytes;
    }
    dev_cap = want;
    p = dev; cap = dev_cap;
    return OBTG_OK;
}

void DevBuf::release()
{
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = nullptr; dev_cap = 0; host = nullptr; host_dev = nullptr;
    p = nullptr; cap = 0; on_host = false;
}

int set_error(obtg_ctx* c, hipError_t e, const char* where)
{
    if (c) {
        c->last_error = std::string(hipGetErrorString(e)) + " at " + where;
    }
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? OBTG_ERR_OOM : OBTG_ERR_DEVICE;
}

ScopedKernelTimer::ScopedKernelTimer(obtg_ctx* c_, int id_, bool ext_) : c(c_), id(id_), ext(ext_)
{
    if (!c->profiling || !((c->profile_mask >> id) & 1u)) return;
    if (c->profile_period > 1 && (c->profile_seen[id]++ % c->profile_period) != 0) return;
    auto take = [&](hipEvent_t& e) {
        if (!c->event_pool.empty()) { e = c->event_pool.back(); c->event_pool.pop_back(); return true; }
        return hipEventCreate(&e) == hipSuccess;
    };
    if (!take(a) || !take(b)) { a = b = nullptr; return; }
    if (!ext) (void)hipEventRecord(a, c->stream);
}

ScopedKernelTimer::~ScopedKernelTimer()
{
    if (!a || !b) return;
    if (!ext) (void)hipEventRecord(b, c->stream);
    c->pending_events.push_back({ id, { a, b } });
}

void flush_pending_events(obtg_ctx* c)
{
    for (auto& pe : c->pending_events) {
        float ms = 0.f;
        if (hipEventSynchronize(pe.second.second) == hipSuccess &&
            hipEventElapsedTime(&ms, pe.second.first, pe.second.second) == hipSuccess) {
            c->stats[pe.first].ms += ms;
            c->stats[pe.first].launches += 1;
        }
        c->event_pool.push_back(pe.second.first);
        c->event_pool.push_back(pe.second.second);
    }
    c->pending_events.clear();
}

static int upload(obtg_ctx* c, DevBuf& buf, const void* src, size_t bytes)
{
    int rc = buf.reserve(bytes);
    if (rc) return rc;
    if (bytes) OBTG_HIP(c, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    // the source is usually a temporary: complete the copy before returning
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    return OBTG_OK;
}

// plain (unfolded) equal-degree product weights w(k,j), layout [2n+1][n+1]
static std::vector<double> plain_product_weights(int n)
{
    int L = 2 * n + 1, nc = n + 1;
    std::vector<double> W((size_t)L * nc, 0.0);
    for (int k = 0; k < L; ++k) {
        double den = binom(2 * n, k);
        for (int j = (k - n > 0 ? k - n : 0); j <= (n < k ? n : k); ++j)
            W[(size_t)k * nc + j] = binom(n, j) * binom(n, k - j) / den;
    }
    // behind them, for the separable form of the speed / angular-rate arithmetic (bern_device.h ang_raw_*): C(n, .), 1 / C(2n, .)
    for (int j = 0; j < nc; ++j) W.push_back(binom(n, j));
    for (int k = 0; k < L; ++k) W.push_back(1.0 / binom(2 * n, k));
    return W;
}

// the true angular-rate rows' product weights in their separable form (bern_device.h ang_row_coeff): C(n, .), 1 / C(2n, .)
static std::vector<double> ang_rows_table(int n)
{
    std::vector<double> W;
    for (int j = 0; j <= n; ++j) W.push_back(binom(n, j));
    for (int k = 0; k <= 2 * n; ++k) W.push_back(1.0 / binom(2 * n, k));
    return W;
}

int ensure_tables(obtg_ctx* c)
{
    if (c->tables_R == c->R) return OBTG_OK;
    (void)hipSetDevice(c->device);                 // (obtg_ctx_set_deg_elev comes here from whatever device the caller was on)
    const int n = c->deg, L = 2 * n + 1;
    if (c->tables_R < 0) {
        auto W2 = folded_product_weights(n, c->dim);
        int rc = upload(c, c->d_w2, W2.data(), W2.size() * sizeof(double));
        if (rc) return rc;
        if (c->dim == 2 && n <= 15) {
            auto a = folded_product_weights(n, 2);        // factor dim/2 = 1
            auto b = folded_product_weights(2 * n, 2);
            auto w = plain_product_weights(n);
            if ((rc = upload(c, c->d_ang_w2n, a.data(), a.size() * sizeof(double)))) return rc;
            if ((rc = upload(c, c->d_ang_w22n, b.data(), b.size() * sizeof(double)))) return rc;
            if ((rc = upload(c, c->d_ang_wn, w.data(), w.size() * sizeof(double)))) return rc;
        }
        if ((c->dim == 2 || c->dim == 3) && n >= 1 && n <= 31) {       // (dim 3: the space-curvature rows)
            auto t = ang_rows_table(n);
            if ((rc = upload(c, c->d_ang_rows, t.data(), t.size() * sizeof(double)))) return rc;
        }
    }
    // the elevation tables belong to ONE R: a context that moves to R = 0 or beyond 512 must not keep the previous R's
    // (the launchers' `d_Tf.p == nullptr` guards mean "no table for this R")
    c->d_Tt.release();
    c->d_Td.release();
    c->d_Tf.release();
    if (c->R > 0 && c->R <= 512) {
        auto Tt = elev_conv_tables(L, c->R);
        int rc = upload(c, c->d_Tt, Tt.data(), Tt.size() * sizeof(double));
        if (rc) return rc;
        auto Td = elev_table_T_ld(L, c->R);
        if ((rc = upload(c, c->d_Td, Td.data(), Td.size() * sizeof(double)))) return rc;
        auto Tf = elev_table_frag(L, c->R);
        if ((rc = upload(c, c->d_Tf, Tf.data(), Tf.size() * sizeof(double)))) return rc;
    }
    c->d_ang_T4.release();
    c->d_ang_cv2.release();
    if (c->R > 0 && c->dim == 2 && n <= 15 && 4 * c->R <= 1000) {   // C(4R, .) and C(2n+R, .) finite in binary64
        auto cv4 = elev_conv_padded(4 * n + 1, 4 * c->R, 8, true, false);
        auto cv2 = elev_conv_padded(2 * n + 1, c->R, 8, false, true);
        int rc = upload(c, c->d_ang_T4, cv4.data(), cv4.size() * sizeof(double));
        if (rc) return rc;
        if ((rc = upload(c, c->d_ang_cv2, cv2.data(), cv2.size() * sizeof(double)))) return rc;
    }
    c->tables_R = c->R;
    return OBTG_OK;
}

int binrow_offset(obtg_ctx* c, int n)
{
    if (n < 0) return OBTG_ERR_ARG;
    if (n > 1029) return OBTG_ERR_UNSUPPORTED;   // C(n, n/2) must be finite in binary64
    if ((int)c->binrow_off.size() <= n) c->binrow_off.resize(n + 1, -1);
    if (c->binrow_off[n] >= 0) return c->binrow_off[n];
    auto row = binom_row(n);
    const int off = (int)c->h_binrows.size();
    c->h_binrows.insert(c->h_binrows.end(), row.begin(), row.end());
    // re-upload the whole (small) table; in-flight kernels keep reading the old allocation's
    // contents only if it is not freed, so drain the stream first
    if (hipStreamSynchronize(c->stream) != hipSuccess) return OBTG_ERR_DEVICE;
    int rc = upload(c, c->d_binrows, c->h_binrows.data(), c->h_binrows.size() * sizeof(double));
    if (rc) return rc;
    c->binrow_off[n] = off;
    return off;
}

static bool check_ctx(const obtg_ctx* c) { return c != nullptr; }

}  // namespace obtg

using namespace obtg;

extern "C" {

const char* obtg_strerror(int code)
{
    switch (code) {
        case OBTG_OK: return "ok";
        case OBTG_ERR_ARG: return "invalid argument";
        case OBTG_ERR_DEVICE: return "HIP runtime error";
        case OBTG_ERR_NO_DEVICE: return "no usable gfx950 device";
        case OBTG_ERR_OOM: return "out of memory";
        case OBTG_ERR_UNSUPPORTED: return "degree / size not supported by the kernels";
        default: return "unknown error";
    }
}

const char* obtg_last_error(const obtg_ctx* c) { return c ? c->last_error.c_str() : ""; }

int obtg_abi_version(void) { return OBTG_ABI_VERSION; }

int obtg_fast_kernels(int dim, int deg)
{
    const int nc = deg + 1;
    int mask = 0;
    if ((dim == 2 || dim == 3) && nc_in_sep(nc)) mask |= 1;
    if (nc_in_dyn(nc)) mask |= 2;
    if (dim == 2 && nc_in_elev(nc)) mask |= 4;
    return mask;
}

int obtg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

const char* obtg_abi_symbols(void)
{
    static const char syms[] =
        "obtg_strerror\0obtg_last_error\0obtg_abi_version\0obtg_source_hash\0obtg_libm_pow_matches\0obtg_fast_kernels\0obtg_device_count\0obtg_abi_symbols\0obtg_host_alloc\0obtg_host_free\0"
        "obtg_ctx_create\0obtg_ctx_destroy\0obtg_ctx_set_stream\0obtg_ctx_use_own_stream\0obtg_ctx_set_deg_elev\0obtg_ctx_set_ang_rate_order\0obtg_ctx_ang_rate_order_in_effect\0obtg_ctx_set_second_speed_bound\0obtg_sync\0"
        "obtg_len_temporal_sep\0obtg_len_speed\0obtg_len_ang_rate\0obtg_num_pairs\0"
        "obtg_temporal_sep\0obtg_speed\0obtg_ang_rate\0obtg_temporal_sep_min\0obtg_temporal_sep_min_range\0obtg_temporal_sep_active\0obtg_temporal_sep_active_dev\0obtg_temporal_sep_min_gather_dev\0obtg_temporal_sep_fd_min_rows_dev\0"
        "obtg_comm_unique_id\0obtg_comm_create\0obtg_comm_destroy\0obtg_comm_size\0obtg_comm_rank\0obtg_comm_last_error\0obtg_comm_all_gather_dev\0obtg_pair_block\0obtg_unpack_pair_blocks_dev\0"
        "obtg_temporal_sep_fd\0obtg_temporal_sep_fd_dev\0obtg_one_vs_many_min\0obtg_one_vs_many_min_dev\0obtg_one_vs_many_min_spans\0obtg_one_vs_many_min_spans_dev\0"
        "obtg_temporal_sep_dev\0obtg_temporal_sep_min_dev\0obtg_speed_dev\0obtg_ang_rate_dev\0obtg_dynamics_dev\0"
        "obtg_fd_batch_dev\0obtg_fd_view_begin\0obtg_fd_view_begin_rows\0obtg_fd_view_end\0obtg_fd_forms_on_the_fly\0obtg_pair_sweep_fd_dev\0obtg_dynamics_fd_dev\0obtg_gjk_pairs\0obtg_ctx_set_polygons\0obtg_ctx_set_hull_pairs\0"
        "obtg_ctx_set_fd_dedup\0obtg_ctx_set_fd_view_structured\0obtg_ctx_set_gjk_history\0obtg_sweep_shape\0obtg_pair_sweep_dev\0obtg_constraint_sweep_dev\0obtg_constraint_sweep_fd_structured_dev\0obtg_constraint_sweep_fd_structured_rows_dev\0obtg_gjk_swarm_dev\0obtg_gjk_swarm\0obtg_min_dist\0obtg_min_dist_mixed\0obtg_min_dist_robust\0obtg_min_dist2poly\0obtg_min_dist2poly_robust\0obtg_gjk_true_pairs\0obtg_coll_check\0obtg_coll_check2poly\0"
        "obtg_bern_extrema\0obtg_bern_extrema_dev\0obtg_temporal_sep_true_min\0obtg_temporal_sep_true_min_dev\0obtg_temporal_sep_true_min_jac\0obtg_temporal_sep_true_min_jac_dev\0"
        "obtg_speed_true_min\0obtg_speed_true_min_dev\0obtg_speed_true_min_jac\0obtg_speed_true_min_jac_dev\0"
        "obtg_accel\0obtg_accel_dev\0obtg_accel_true_min\0obtg_accel_true_min_dev\0obtg_accel_true_min_jac\0obtg_accel_true_min_jac_dev\0"
        "obtg_jerk\0obtg_jerk_dev\0obtg_jerk_true_min\0obtg_jerk_true_min_dev\0obtg_jerk_true_min_jac\0obtg_jerk_true_min_jac_dev\0"
        "obtg_ang_rate_poly\0obtg_ang_rate_poly_dev\0obtg_ang_rate_true_min\0obtg_ang_rate_true_min_dev\0obtg_ang_rate_true_min_jac\0obtg_ang_rate_true_min_jac_dev\0"
        "obtg_curvature_poly\0obtg_curvature_poly_dev\0obtg_curvature_true_min\0obtg_curvature_true_min_dev\0obtg_curvature_true_min_jac\0obtg_curvature_true_min_jac_dev\0obtg_bern_curvature\0obtg_bern_curvature_dev\0"
        "obtg_space_curvature_poly\0obtg_space_curvature_poly_dev\0obtg_space_curvature_true_min\0obtg_space_curvature_true_min_dev\0obtg_space_curvature_true_min_jac\0obtg_space_curvature_true_min_jac_dev\0obtg_bern_space_curvature\0obtg_bern_space_curvature_dev\0"
        "obtg_ctx_set_keep_in\0obtg_len_keep_in\0obtg_keep_in\0obtg_keep_in_dev\0obtg_keep_in_true_min\0obtg_keep_in_true_min_dev\0obtg_keep_in_true_min_jac\0obtg_keep_in_true_min_jac_dev\0"
        "obtg_ctx_set_keep_out\0obtg_len_keep_out\0obtg_keep_out_true_min\0obtg_keep_out_true_min_dev\0obtg_keep_out_true_min_jac\0obtg_keep_out_true_min_jac_dev\0obtg_bern_keep_out\0obtg_bern_keep_out_dev\0"
        "obtg_ctx_set_keep_out_motion\0obtg_keep_out_moving_true_min\0obtg_keep_out_moving_true_min_dev\0obtg_keep_out_moving_true_min_jac\0obtg_keep_out_moving_true_min_jac_dev\0obtg_bern_keep_out_moving\0obtg_bern_keep_out_moving_dev\0"
        "obtg_keep_out_features\0obtg_keep_out_euclid_true_min\0obtg_keep_out_euclid_true_min_dev\0obtg_keep_out_euclid_true_min_jac\0obtg_keep_out_euclid_true_min_jac_dev\0obtg_bern_keep_out_euclid\0obtg_bern_keep_out_euclid_dev\0"
        "obtg_ctx_set_pair_keep_out\0obtg_len_pair_keep_out\0obtg_pair_keep_out_true_min\0obtg_pair_keep_out_true_min_dev\0obtg_pair_keep_out_true_min_jac\0obtg_pair_keep_out_true_min_jac_dev\0"
        "obtg_pair_keep_out_euclid_true_min\0obtg_pair_keep_out_euclid_true_min_dev\0obtg_pair_keep_out_euclid_true_min_jac\0obtg_pair_keep_out_euclid_true_min_jac_dev\0"
        "obtg_ctx_set_proximity\0obtg_len_proximity\0obtg_proximity_poly\0obtg_proximity_poly_dev\0obtg_proximity_true\0obtg_proximity_true_dev\0obtg_proximity_true_jac\0obtg_proximity_true_jac_dev\0"
        "obtg_bern_elev\0obtg_bern_diff\0obtg_bern_mul\0obtg_bern_normsq\0obtg_bern_split\0obtg_bern_restrict\0obtg_bern_eval\0"
        "obtg_euclidean_obj\0obtg_accel_obj\0obtg_jerk_obj\0"
        "obtg_bern_arc_length\0obtg_bern_arc_length_dev\0obtg_arc_length_obj\0obtg_arc_length_obj_dev\0"
        "obtg_temporal_sep_jac\0obtg_temporal_sep_jac_dev\0obtg_speed_jac\0obtg_speed_jac_dev\0obtg_ang_rate_jac\0obtg_ang_rate_jac_dev\0obtg_euclidean_grad\0obtg_deriv_energy_grad\0"
        "obtg_set_profiling\0obtg_set_profile_period\0obtg_kernel_stats\0obtg_reset_kernel_stats\0obtg_kernel_name\0";
    return syms;
}

int obtg_ctx_create(obtg_ctx** out, int n_veh, int dim, int deg, int deg_elev, int n_point_obs,
                    const double* point_obs, int device)
{
    if (!out) return OBTG_ERR_ARG;
    *out = nullptr;
    if (n_veh < 1 || dim < 1 || dim > 3 || deg < 1 || deg_elev < 0 || n_point_obs < 0) return OBTG_ERR_ARG;
    if (n_point_obs > 0 && !point_obs) return OBTG_ERR_ARG;
    int ndev = obtg_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev) return OBTG_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); return OBTG_ERR_NO_DEVICE; }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return OBTG_ERR_NO_DEVICE;  // code objects are gfx950 only
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return OBTG_ERR_NO_DEVICE; }
    obtg_ctx* c = new (std::nothrow) obtg_ctx();
    if (!c) return OBTG_ERR_OOM;
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->device = device; c->n_veh = n_veh; c->dim = dim; c->deg = deg; c->R = deg_elev;
    c->n_obs = n_point_obs; c->n_obj = n_veh + n_point_obs;
    c->n_pairs = c->n_obj * (c->n_obj - 1) / 2;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError(); delete c; return OBTG_ERR_DEVICE;
    }
    c->stream = c->own_stream;
    // OBTG_ZERO_COPY=0 keeps every staging buffer in device memory (the path for large batches)
    { const char* e = getenv("OBTG_ZERO_COPY"); const bool zc = !(e && e[0] == '0'); c->ws_in.io = c->ws_in2.io = c->ws_out.io = zc; }
    // OBTG_FD_VIEW_STRUCTURED=0: contexts start with the structured routing of a view's one-call sweep off (obtg_ctx_set_fd_view_structured)
    { const char* e = getenv("OBTG_FD_VIEW_STRUCTURED"); c->fd_view_structured = !(e && e[0] == '0'); }
    // OBTG_TRUE_MIN_JAC_FUSED=0: obtg_temporal_sep_true_min_jac, obtg_speed_true_min_jac and obtg_ang_rate_true_min_jac form their blocks in a launch of their own on every shape
    { const char* e = getenv("OBTG_TRUE_MIN_JAC_FUSED"); c->true_min_jac_fused = !(e && e[0] == '0'); }
    int rc = OBTG_OK;
    c->h_pairs.resize((size_t)2 * c->n_pairs);
    {
        size_t p = 0;
        for (int i = 0; i < c->n_obj - 1; ++i)
            for (int j = i + 1; j < c->n_obj; ++j) { c->h_pairs[p++] = i; c->h_pairs[p++] = j; }
    }
    rc = upload(c, c->d_pairs, c->h_pairs.data(), c->h_pairs.size() * sizeof(int));
    if (!rc) rc = upload(c, c->d_obs, point_obs, sizeof(double) * (size_t)n_point_obs * dim);
    if (!rc) rc = ensure_tables(c);
    if (!rc) {
        // the structured FD step's ticket counters (obtg_ctx::d_struct_tickets): both banks zero
        c->struct_ticket_stride = std::max(256, (c->n_pairs + 63) / 64 + 64);
        const size_t bytes = sizeof(int) * 2 * (size_t)c->struct_ticket_stride;
        rc = c->d_struct_tickets.reserve(bytes);
        if (!rc && hipMemset(c->d_struct_tickets.p, 0, bytes) != hipSuccess) { (void)hipGetLastError(); rc = OBTG_ERR_DEVICE; }
    }
    if (rc) { obtg_ctx_destroy(c); return rc; }
    *out = c;
    return OBTG_OK;
}

void obtg_ctx_destroy(obtg_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    flush_pending_events(c);
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    DevBuf* bufs[] = { &c->d_pairs, &c->d_obs, &c->d_w2, &c->d_Tt, &c->d_Td, &c->d_Tf, &c->d_ang_dd, &c->d_ang_flags, &c->d_vp_off, &c->d_vp_idx, &c->d_ang_w2n, &c->d_ang_w22n, &c->d_ang_wn, &c->d_ang_rows, &c->d_curv_tab, &c->d_ang_T4, &c->d_ang_cv2, &c->d_jac,
                       &c->d_binrows, &c->d_tiles, &c->d_poly_pts, &c->d_poly_off, &c->d_hp_a, &c->d_hp_b, &c->d_tile_chunk_off, &c->d_tile_order, &c->d_tile_pslots,
                       &c->d_tile_cobj_off, &c->d_tile_cobjs, &c->d_tile_ij, &c->d_struct_tickets, &c->d_keep_H, &c->d_keep_VF, &c->d_ko_H, &c->d_ko_off, &c->d_ko_VO, &c->d_ko_Q, &c->d_ko_qoff, &c->d_ko_T, &c->d_pk_H, &c->d_pk_IJ, &c->d_pk_Hn, &c->d_pk_feat, &c->d_prox_items, &c->d_prox_par, &c->d_prox_pts, &c->ws_in,
                       &c->ws_in2, &c->ws_out, &c->ws_fd };
    for (DevBuf* b : bufs) b->release();
    for (auto& b : c->ws_misc) b.release();
    for (auto& b : c->d_gjk_len) b.release();
    if (c->ring) {
        (void)hipHostFree(c->ring);
        for (hipEvent_t e : c->ring_ev) if (e) (void)hipEventDestroy(e);
    }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int obtg_ctx_set_stream(obtg_ctx* c, void* hip_stream)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->stream = static_cast<hipStream_t>(hip_stream);        // as given: NULL is the null stream
    return OBTG_OK;
}

int obtg_ctx_use_own_stream(obtg_ctx* c)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->stream = c->own_stream;
    return OBTG_OK;
}

int obtg_ctx_set_deg_elev(obtg_ctx* c, int deg_elev)
{
    if (!check_ctx(c) || deg_elev < 0) return OBTG_ERR_ARG;
    if (deg_elev == c->R) return OBTG_OK;
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->R = deg_elev;
    return ensure_tables(c);
}

int obtg_host_alloc(size_t bytes, void** out)
{
    if (!out) return OBTG_ERR_ARG;
    *out = nullptr;
    if (bytes == 0) bytes = 8;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return OBTG_ERR_OOM; }
    return OBTG_OK;
}

int obtg_host_free(void* p)
{
    if (!p) return OBTG_OK;
    if (hipHostFree(p) != hipSuccess) { (void)hipGetLastError(); return OBTG_ERR_ARG; }
    return OBTG_OK;
}

int obtg_ctx_set_ang_rate_order(obtg_ctx* c, int elevate_first)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    if (elevate_first < 0 || elevate_first > 2) return OBTG_ERR_ARG;
    c->ang_elevate_first = elevate_first == 1;
    c->ang_exact = elevate_first == 2;
    return OBTG_OK;
}

int obtg_ctx_ang_rate_order_in_effect(obtg_ctx* c)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    return ang_rate_order_in_effect(c);
}

int obtg_ctx_set_second_speed_bound(obtg_ctx* c, double bound, int is_max, double* d_out)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    c->speed2.bound = bound; c->speed2.is_max = is_max != 0; c->speed2.d_out = d_out;
    return OBTG_OK;
}

int obtg_sync(obtg_ctx* c)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    flush_pending_events(c);
    return OBTG_OK;
}

int obtg_len_temporal_sep(const obtg_ctx* c) { return c ? c->n_pairs * (2 * c->deg + c->R + 1) : 0; }
int obtg_len_speed(const obtg_ctx* c) { return c ? c->n_veh * (2 * c->deg + c->R + 1) : 0; }
int obtg_len_ang_rate(const obtg_ctx* c) { return c ? c->n_veh * (4 * (c->deg + c->R) + 1) : 0; }
int obtg_num_pairs(const obtg_ctx* c) { return c ? c->n_pairs : 0; }

// ------------------------------------------------------------------ virtual finite-difference batch
// dY == NULL in a `_dev` sweep means "the batch of the open view" (obtg_fd_view_begin): the launcher gets the view's
// single row with c->fd set; kernels that form the rows while staging them use it, the others answer kNeedBatch and
// the batch is written to a context buffer -- once per view -- and handed over instead.
static int fd_materialise(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int B, int row0);

extern "C++" {
// can_fd: can EVERY kernel of this call form the view's rows itself?  Decided before anything is launched, so that a
// call of several launches never runs its first ones twice (a launcher answering kNeedBatch after an earlier launch of
// the same call had gone out used to make the whole call run again on the materialised batch: right results, twice
// the work, two flips of the sweep's trip-count history).
// launch_dynamics is one launch on the specialised shapes; otherwise a speed launch and / or a generic angular-rate one
static bool dynamics_can_fd(const obtg_ctx* c, bool want_speed, bool want_ang)
{
    if (dynamics_fd_on_the_fly(c, want_ang)) return true;
    return !want_ang && want_speed && bernstein_fd_on_the_fly(c);
}
// launch_pair_sweep: one launch, or a gjkNew sweep (forms the rows itself unless it de-duplicates) + the separate
// temporal-separation kernel
static bool pair_sweep_can_fd(const obtg_ctx* c)
{
    return pair_sweep_is_one_launch(c) || (!c->fd_dedup && bernstein_fd_on_the_fly(c));
}

template <class Launch>
static int with_batch(obtg_ctx* c, const double* dY, int B, bool can_fd, Launch launch)
{
    if (dY) return launch(dY);
    if (!c->view.Y0 || B != c->view.B) return OBTG_ERR_ARG;
    int rc = kNeedBatch;
    if (!c->view.materialised && can_fd) {
        c->fd.Y0 = c->view.Y0; c->fd.h = c->view.h; c->fd.fixed = c->view.fixed; c->fd.row0 = c->view.row0;
        rc = launch(c->view.Y0);
        c->fd.Y0 = nullptr; c->fd.row0 = 0;
    }
    if (rc != kNeedBatch) return rc;
    if (!c->view.materialised) {
        if ((rc = fd_materialise(c, c->view.Y0, c->view.fixed, c->view.h, c->view.B, c->view.row0))) return rc;
        c->view.materialised = true;
    }
    return launch(c->ws_fd.as<double>());
}
}  // extern "C++"

static int fd_args_ok(const obtg_ctx* c, int n_fixed_cols, int row_begin, int B)
{
    const int rows = c->n_veh * c->dim, nc = c->deg + 1;
    if (n_fixed_cols < 0 || nc - 2 * n_fixed_cols <= 0 || row_begin < 0) return OBTG_ERR_ARG;
    if (B < 1 || row_begin + B > rows * (nc - 2 * n_fixed_cols) + 1) return OBTG_ERR_ARG;
    return OBTG_OK;
}

int obtg_fd_view_begin_rows(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int row_begin, int B)
{
    if (!check_ctx(c) || !dY0) return OBTG_ERR_ARG;
    if (int rc = fd_args_ok(c, n_fixed_cols, row_begin, B)) return rc;
    c->view.Y0 = dY0; c->view.h = h; c->view.fixed = n_fixed_cols; c->view.B = B; c->view.row0 = row_begin; c->view.materialised = false;
    return OBTG_OK;
}

int obtg_fd_view_begin(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int B)
{
    return obtg_fd_view_begin_rows(c, dY0, n_fixed_cols, h, 0, B);
}

int obtg_fd_view_end(obtg_ctx* c)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    c->view.Y0 = nullptr; c->view.B = 0; c->view.row0 = 0; c->view.materialised = false;
    return OBTG_OK;
}

// ------------------------------------------------------------------ device-pointer sweeps
int obtg_temporal_sep_dev(obtg_ctx* c, const double* dY, int B, double max_sep, int pair_begin,
                          int pair_count, double* d_out)
{
    if (!check_ctx(c) || !d_out || B < 0) return OBTG_ERR_ARG;
    if (pair_begin < 0 || pair_count < 0 || pair_begin + pair_count > c->n_pairs) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) {
        return launch_temporal_sep(c, src, B, max_sep, pair_begin, pair_count, false, d_out); });
}

int obtg_temporal_sep_min_dev(obtg_ctx* c, const double* dY, int B, double max_sep, int pair_begin,
                              int pair_count, double* d_out)
{
    if (!check_ctx(c) || !d_out || B < 0) return OBTG_ERR_ARG;
    if (pair_begin < 0 || pair_count < 0 || pair_begin + pair_count > c->n_pairs) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) {
        return launch_temporal_sep(c, src, B, max_sep, pair_begin, pair_count, true, d_out); });
}

int obtg_temporal_sep_active_dev(obtg_ctx* c, const double* dY, int B, double max_sep, int k, int pair_begin,
                                 int pair_count, double* d_out_val, int* d_out_idx)
{
    if (!check_ctx(c) || !d_out_val || B < 0 || k < 1 || k > 4 || k > 2 * c->deg + c->R + 1) return OBTG_ERR_ARG;
    if (pair_begin < 0 || pair_count < 0 || pair_begin + pair_count > c->n_pairs) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) {
        return launch_temporal_sep(c, src, B, max_sep, pair_begin, pair_count, true, d_out_val, k, d_out_idx); });
}

int obtg_temporal_sep_fd_min_rows_dev(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int row_begin, int n_rows,
                                      double max_sep, double* d_out)
{
    if (!check_ctx(c) || !dY0 || !d_out || n_rows < 0 || row_begin < 1) return OBTG_ERR_ARG;
    if (int rc = fd_args_ok(c, n_fixed_cols, row_begin, n_rows > 0 ? n_rows : 1)) return rc;
    if (n_rows == 0 || c->n_obj < 2) return OBTG_OK;
    (void)hipSetDevice(c->device);
    return launch_temporal_sep_fd(c, dY0, n_rows, nullptr, nullptr, nullptr, max_sep, d_out, 1, row_begin, n_fixed_cols, h);
}

int obtg_temporal_sep_min_gather_dev(obtg_ctx* c, obtg_comm* m, const double* dY, int B, double max_sep, double* d_min_all)
{
    if (!check_ctx(c) || !m || !d_min_all || B < 0) return OBTG_ERR_ARG;
    if (B == 0 || c->n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) { return comm_gather_pair_minima(m, c, src, B, max_sep, d_min_all); });
}

int obtg_speed_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, int is_max,
                   double* d_out)
{
    if (!check_ctx(c) || !d_tf || !d_out || B < 0) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) { return launch_speed(c, src, d_tf, B, bound, is_max, d_out); });
}

int obtg_accel_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, double* d_out)
{
    if (!check_ctx(c) || !d_tf || !d_out || B < 0) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) { return launch_speed(c, src, d_tf, B, bound, 1, d_out, 2); });
}

int obtg_jerk_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, double* d_out)
{
    if (!check_ctx(c) || !d_tf || !d_out || B < 0) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) { return launch_speed(c, src, d_tf, B, bound, 1, d_out, 3); });
}

int obtg_ang_rate_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double max_rate, double* d_out)
{
    if (!check_ctx(c) || !d_tf || !d_out || B < 0) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) { return launch_ang_rate(c, src, d_tf, B, max_rate, d_out); });
}

int obtg_dynamics_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double speed_bound,
                      int speed_is_max, double max_rate, double* d_out_speed, double* d_out_ang)
{
    if (!check_ctx(c) || !d_tf || B < 0 || (!d_out_speed && !d_out_ang)) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, dynamics_can_fd(c, d_out_speed != nullptr, d_out_ang != nullptr), [&](const double* src) {
        return launch_dynamics(c, src, d_tf, B, speed_bound, speed_is_max, max_rate, d_out_speed, d_out_ang); });
}

static int fd_materialise(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int B, int row0)
{
    int rc = c->ws_fd.reserve(sizeof(double) * (size_t)B * c->n_veh * c->dim * (c->deg + 1));
    if (rc) return rc;
    return launch_fd_batch(c, dY0, n_fixed_cols, h, B, c->ws_fd.as<double>(), row0);
}

int obtg_fd_forms_on_the_fly(const obtg_ctx* c)
{
    if (!c) return 0;
    return (pair_sweep_is_one_launch(c) ? 1 : 0) | ((c->dim == 2 && dynamics_fd_on_the_fly(c, true)) ? 2 : 0);
}

// one-call forms: a view around a single sweep
int obtg_pair_sweep_fd_dev(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int B, double max_sep,
                           double* d_out_sep, int max_iter, int md_cap, int* d_flag, double* d_p1, double* d_p2,
                           double* d_dist, int* d_nsup, int* d_status)
{
    int rc = obtg_fd_view_begin(c, dY0, n_fixed_cols, h, B);
    if (rc) return rc;
    rc = obtg_pair_sweep_dev(c, nullptr, B, max_sep, d_out_sep, max_iter, md_cap, d_flag, d_p1, d_p2, d_dist, d_nsup, d_status);
    (void)obtg_fd_view_end(c);
    return rc;
}

int obtg_dynamics_fd_dev(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, const double* d_tf, int B,
                         double speed_bound, int speed_is_max, double max_rate, double* d_out_speed, double* d_out_ang)
{
    int rc = obtg_fd_view_begin(c, dY0, n_fixed_cols, h, B);
    if (rc) return rc;
    rc = obtg_dynamics_dev(c, nullptr, d_tf, B, speed_bound, speed_is_max, max_rate, d_out_speed, d_out_ang);
    (void)obtg_fd_view_end(c);
    return rc;
}

int obtg_fd_batch_dev(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int B, double* dY)
{
    if (!check_ctx(c) || !dY0 || !dY || B < 1 || n_fixed_cols < 0) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return launch_fd_batch(c, dY0, n_fixed_cols, h, B, dY);
}

// ------------------------------------------------------------------ host-buffer sweeps
// Host <-> device copies of the host-buffer entry points.  A caller's NumPy array is pageable memory; handing it
// to hipMemcpyAsync makes the runtime bounce it through its own staging at ~10 GB/s (measured: 427 MB D2H in
// 41 ms).  Instead: (a) buffers the caller allocated with obtg_host_alloc (pinned) are DMA targets as they are;
// (b) pageable buffers go through the context's pinned ring in chunks, the DMA of chunk i+1 running while the host
// copies chunk i out of (into) the ring.
constexpr size_t kRingChunk = 4u << 20;     // bytes per ring slot
constexpr int kRingSlots = 4;
constexpr size_t kRingMin = 256u << 10;     // smaller copies: one pageable hipMemcpyAsync is as fast

static bool is_pinned(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

static int ensure_ring(obtg_ctx* c)
{
    if (c->ring) return OBTG_OK;
    if (hipHostMalloc(&c->ring, kRingChunk * kRingSlots, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); c->ring = nullptr; return OBTG_ERR_OOM;
    }
    for (int i = 0; i < kRingSlots; ++i)
        if (hipEventCreateWithFlags(&c->ring_ev[i], hipEventDisableTiming) != hipSuccess) {
            // partial failure: leave no half-built ring behind (the next call would take it for a complete one)
            (void)hipGetLastError();
            for (int j = 0; j < i; ++j) { (void)hipEventDestroy(c->ring_ev[j]); c->ring_ev[j] = nullptr; }
            c->ring_ev[i] = nullptr;
            (void)hipHostFree(c->ring);
            c->ring = nullptr;
            return OBTG_ERR_DEVICE;
        }
    return OBTG_OK;
}

// wait until the DMA that last used ring slot `sl` is done (the CPU is about to touch the slot)
static int ring_slot_ready(obtg_ctx* c, int sl)
{
    if (c->ring_pending[sl]) {
        OBTG_HIP(c, hipEventSynchronize(c->ring_ev[sl]));
        c->ring_pending[sl] = false;
    }
    return OBTG_OK;
}

// zero_copy: inputs of up to kZeroCopyIn bytes may stay in mapped host memory (the kernel fetches them across PCIe:
// a one-row call of 64 vehicles, 11 KB read by several workgroups, is already slower that way than one DMA transfer)
constexpr size_t kZeroCopyIn = 8u << 10;
static int h2d(obtg_ctx* c, DevBuf& b, const void* src, size_t bytes, bool zero_copy = false)
{
    int rc = b.reserve(bytes, zero_copy && bytes <= kZeroCopyIn);
    if (rc) return rc;
    if (b.on_host) {        // mapped host block: the device is idle between host entry points, nothing can be reading it
        std::memcpy(b.host, src, bytes);
        return OBTG_OK;
    }
    if (bytes < kRingMin || is_pinned(src) || ensure_ring(c) != OBTG_OK) {
        OBTG_HIP(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return OBTG_OK;
    }
    char* ring = static_cast<char*>(c->ring);
    for (size_t off = 0; off < bytes; off += kRingChunk) {
        const int sl = c->ring_next;
        c->ring_next = (c->ring_next + 1) % kRingSlots;
        const size_t nb = std::min(kRingChunk, bytes - off);
        if ((rc = ring_slot_ready(c, sl))) return rc;
        std::memcpy(ring + sl * kRingChunk, static_cast<const char*>(src) + off, nb);
        OBTG_HIP(c, hipMemcpyAsync(static_cast<char*>(b.p) + off, ring + sl * kRingChunk, nb, hipMemcpyHostToDevice, c->stream));
        OBTG_HIP(c, hipEventRecord(c->ring_ev[sl], c->stream));
        c->ring_pending[sl] = true;
    }
    return OBTG_OK;
}

// device -> host, complete on return for THIS array (the stream may still hold other work)
// the CPU address of `src` when it lies in the mapped host block of a staging buffer, else nullptr
static const void* mapped_alias(const obtg_ctx* c, const void* src)
{
    for (const DevBuf* b : { &c->ws_in, &c->ws_in2, &c->ws_out }) {
        if (!b->host) continue;
        const char* lo = static_cast<const char*>(b->host_dev);
        const char* q = static_cast<const char*>(src);
        if (q >= lo && q < lo + kZeroCopyBytes) return static_cast<const char*>(b->host) + (q - lo);
    }
    return nullptr;
}

static int d2h_copy(obtg_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return OBTG_OK;
    if (const void* h = mapped_alias(c, src)) {     // the kernel wrote host memory itself: wait for it, then a plain copy
        OBTG_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(dst, h, bytes);
        return OBTG_OK;
    }
    if (bytes < kRingMin || is_pinned(dst) || ensure_ring(c) != OBTG_OK) {
        OBTG_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
        return OBTG_OK;
    }
    char* ring = static_cast<char*>(c->ring);
    const size_t n_chunks = (bytes + kRingChunk - 1) / kRingChunk;
    int slot_of[kRingSlots];
    int rc;
    auto issue = [&](size_t i) -> int {
        const size_t off = i * kRingChunk, nb = std::min(kRingChunk, bytes - off);
        const int sl = c->ring_next;
        c->ring_next = (c->ring_next + 1) % kRingSlots;
        slot_of[i % kRingSlots] = sl;
        // a pending H2D out of this slot precedes us on the same stream: DMA order is safe, only CPU access waits
        OBTG_HIP(c, hipMemcpyAsync(ring + sl * kRingChunk, static_cast<const char*>(src) + off, nb, hipMemcpyDeviceToHost, c->stream));
        OBTG_HIP(c, hipEventRecord(c->ring_ev[sl], c->stream));
        c->ring_pending[sl] = true;
        return OBTG_OK;
    };
    size_t issued = 0;
    for (; issued < n_chunks && issued < (size_t)kRingSlots; ++issued) if ((rc = issue(issued))) return rc;
    for (size_t i = 0; i < n_chunks; ++i) {
        const int sl = slot_of[i % kRingSlots];
        if ((rc = ring_slot_ready(c, sl))) return rc;
        const size_t off = i * kRingChunk, nb = std::min(kRingChunk, bytes - off);
        std::memcpy(static_cast<char*>(dst) + off, ring + sl * kRingChunk, nb);
        if (issued < n_chunks) { if ((rc = issue(issued))) return rc; ++issued; }   // the slot just emptied is next in the rotation
    }
    return OBTG_OK;
}

// the last output of a host entry point: copy, then leave the device idle
static int d2h(obtg_ctx* c, void* dst, const void* src, size_t bytes)
{
    int rc = d2h_copy(c, dst, src, bytes);
    if (rc) return rc;
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    for (bool& f : c->ring_pending) f = false;
    flush_pending_events(c);
    return OBTG_OK;
}

static size_t ysize(const obtg_ctx* c) { return (size_t)c->n_veh * c->dim * (c->deg + 1); }

// ------------------------------------------------------------------ the Bernstein-family host entry points
// The one host path of obtg_temporal_sep[_min[_range]|_active|_fd|_jac|_true_min[_jac]], obtg_one_vs_many_min[_spans],
// obtg_speed[_jac|_true_min[_jac]], obtg_ang_rate[_jac|_poly|_true_min[_jac]], obtg_bern_*, the objectives and their gradients.  Every one of them is: its argument
// checks, a HostCall, its operands by name (in), its outputs by name (out), its launcher (run), the download -- optional
// outputs first (fetch, skipped for a null pointer), the mandatory one last (finish: the call's ONE synchronise).  The slots
// of ws_misc are obtg::WsSlot, and so is the rule for who may hold which.  The next entry point of the family starts as a
// copy of obtg_speed (one output) or obtg_bern_extrema (optional outputs); the true-minimum row families have a path of
// their own on top of this one (true_min_host, below).
// What the entry points do NOT share, because a caller or a timing could tell -- each keeps the answer it has given since it
// was added:
//  - zero copy (mapped host memory; the one-row SLSQP callbacks): Y, tf and the result of obtg_temporal_sep[_min[_range]],
//    obtg_speed, obtg_ang_rate and the objectives, Y of _active and _true_min[_jac], Y and tf of
//    obtg_speed_true_min[_jac], obtg_ang_rate_true_min[_jac] and obtg_ang_rate_poly, `one` and the result of
//    obtg_one_vs_many_min[_spans]; NOT the outputs of _active / _true_min*, and nothing of the _jac / _grad calls, of
//    obtg_temporal_sep_fd, obtg_bern_extrema or obtg_bern_*;
//  - an empty call with null pointers is OBTG_OK in obtg_one_vs_many_min[_spans] (B or K == 0), obtg_temporal_sep_fd (no
//    perturbations, or fewer than two objects) and obtg_bern_extrema (M == 0); every other call rejects a null mandatory
//    pointer first, and a context without pairs answers OBTG_OK only after that;
//  - obtg_bern_extrema requires status, obtg_temporal_sep_true_min[_jac], obtg_speed_true_min[_jac] and
//    obtg_ang_rate_true_min[_jac] take it as optional;
//  - obtg_bern_normsq has no empty case (d >= 1); obtg_bern_restrict looks at every span before rows == 0 answers OBTG_OK;
//  - obtg_ang_rate answers dim != 2 after its pointer checks, obtg_ang_rate_jac before them;
//  - the _dev twins of the _jac calls answer OBTG_OK for B == 0 before the pointer checks, the host calls after them.
extern "C++" {
template <class T> static T* slot(obtg_ctx* c, WsSlot s) { return c->ws_misc[s].as<T>(); }

// One host-buffer call: remembers the first failure, after which every later step is skipped.  Counts are elements of T.
struct HostCall {
    obtg_ctx* c;
    int rc = OBTG_OK;
    explicit HostCall(obtg_ctx* c_) : c(c_) { (void)hipSetDevice(c->device); }
    template <class T> const T* in(DevBuf& b, const T* src, size_t count, bool zero_copy = false) { if (!rc) rc = h2d(c, b, src, sizeof(T) * count, zero_copy); return b.as<T>(); }
    template <class T> T* out(DevBuf& b, size_t count, bool zero_copy = false) { if (!rc) rc = b.reserve(sizeof(T) * count, zero_copy); return b.as<T>(); }
    template <class Launch> void run(Launch launch) { if (!rc) rc = launch(); }
    template <class T> void fetch(T* dst, const T* src, size_t count) { if (!rc && dst) rc = d2h_copy(c, dst, src, sizeof(T) * count); }     // optional output
    template <class T> int finish(T* dst, const T* src, size_t count) { return rc ? rc : d2h(c, dst, src, sizeof(T) * count); }             // the ONE synchronise
};
}  // extern "C++"

static int host_sep(obtg_ctx* c, const double* Y, int B, double max_sep, bool min_only, double* out,
                    int pair_begin = 0, int pair_count = -1)
{
    if (!check_ctx(c) || !Y || !out || B < 0) return OBTG_ERR_ARG;
    if (pair_count < 0) pair_count = c->n_pairs - pair_begin;
    if (pair_begin < 0 || pair_begin + pair_count > c->n_pairs) return OBTG_ERR_ARG;
    if (B == 0 || pair_count == 0) return OBTG_OK;
    const size_t n = (min_only ? (size_t)pair_count : (size_t)pair_count * (2 * c->deg + c->R + 1)) * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    double* d_out = h.out<double>(c->ws_out, n, true);
    h.run([&] { return launch_temporal_sep(c, dY, B, max_sep, pair_begin, pair_count, min_only, d_out); });
    return h.finish(out, d_out, n);
}

int obtg_temporal_sep_active(obtg_ctx* c, const double* Y, int B, double max_sep, int k, double* out_val, int* out_idx)
{
    if (!check_ctx(c) || !Y || !out_val || B < 0 || k < 1 || k > 4 || k > 2 * c->deg + c->R + 1) return OBTG_ERR_ARG;
    if (B == 0 || c->n_pairs == 0) return OBTG_OK;
    const size_t n = (size_t)c->n_pairs * k * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    double* d_val = h.out<double>(c->ws_out, n);
    int* d_idx = h.out<int>(c->ws_misc[WS_STATUS], n);
    h.run([&] { return launch_temporal_sep(c, dY, B, max_sep, 0, c->n_pairs, true, d_val, k, d_idx); });
    h.fetch(out_idx, d_idx, n);
    return h.finish(out_val, d_val, n);
}

int obtg_temporal_sep_min_range(obtg_ctx* c, const double* Y, int B, double max_sep, int pair_begin,
                                int pair_count, double* out)
{
    if (pair_count < 0) return OBTG_ERR_ARG;
    return host_sep(c, Y, B, max_sep, true, out, pair_begin, pair_count);
}

int obtg_temporal_sep(obtg_ctx* c, const double* Y, int B, double max_sep, double* out) { return host_sep(c, Y, B, max_sep, false, out); }
int obtg_temporal_sep_min(obtg_ctx* c, const double* Y, int B, double max_sep, double* out) { return host_sep(c, Y, B, max_sep, true, out); }

// Bezier.sub on curves with different [t0, tf] (bezier.py:347-374 -> _temporalAlignment 903-941), then the same minimum
static bool spans_ok(const double* s, int n)
{
    for (int i = 0; i < n; ++i) if (!(s[2 * i] < s[2 * i + 1])) return false;       // (NaN ends are refused too)
    return true;
}

// A check shared by a host entry point and its _dev twin answers an OBTG_ERR_* code, OBTG_OK ("go on") or kNothingToDo: the
// call is valid and empty, the entry point returns done(that) = OBTG_OK
constexpr int kNothingToDo = 1;
static int done(int chk) { return chk == kNothingToDo ? OBTG_OK : chk; }

// Examples/SequentialSwarm.py:43-70: one curve against K others, per-pair minimum of the elevated control points
static int one_vs_many_args(const obtg_ctx* c, const double* one, int B, const double* many, int K, const double* out,
                            bool with_spans = false, const double* one_span = nullptr, const double* many_span = nullptr)
{
    if (!check_ctx(c) || B < 0 || K < 0) return OBTG_ERR_ARG;
    if (B == 0 || K == 0) return kNothingToDo;
    if (!one || !many || !out) return OBTG_ERR_ARG;
    if (with_spans && (!one_span || !many_span || !spans_ok(one_span, B) || !spans_ok(many_span, K))) return OBTG_ERR_ARG;
    return OBTG_OK;
}

int obtg_one_vs_many_min_dev(obtg_ctx* c, const double* d_one, int B, const double* d_many, int K, double max_sep, double* d_out)
{
    if (int chk = one_vs_many_args(c, d_one, B, d_many, K, d_out)) return done(chk);
    (void)hipSetDevice(c->device);
    return launch_one_vs_many_min(c, d_one, B, d_many, K, max_sep, d_out);
}

int obtg_one_vs_many_min(obtg_ctx* c, const double* one, int B, const double* many, int K, double max_sep, double* out)
{
    if (int chk = one_vs_many_args(c, one, B, many, K, out)) return done(chk);
    const size_t curve = (size_t)c->dim * (c->deg + 1), n = (size_t)B * K;
    HostCall h(c);
    const double* d_one = h.in(c->ws_in, one, curve * B, true);
    // the planned trajectories grow by one curve per vehicle: the staging buffer grows with them, nothing else does
    const double* d_many = h.in(c->ws_in2, many, curve * K);
    double* d_out = h.out<double>(c->ws_out, n, true);
    h.run([&] { return launch_one_vs_many_min(c, d_one, B, d_many, K, max_sep, d_out); });
    return h.finish(out, d_out, n);
}

int obtg_one_vs_many_min_spans_dev(obtg_ctx* c, const double* d_one, const double* one_span, int B, const double* d_many,
                                   const double* many_span, int K, double max_sep, double no_overlap, double* d_out)
{
    if (int chk = one_vs_many_args(c, d_one, B, d_many, K, d_out, true, one_span, many_span)) return done(chk);
    HostCall h(c);
    const double* d_one_span = h.in(c->ws_misc[WS_ARG_A], one_span, 2 * (size_t)B);
    const double* d_many_span = h.in(c->ws_misc[WS_ARG_B], many_span, 2 * (size_t)K);
    if (h.rc) return h.rc;
    OBTG_HIP(c, hipStreamSynchronize(c->stream));       // the caller's span arrays are free on return; the launch is asynchronous
    return launch_one_vs_many_min_spans(c, d_one, d_one_span, B, d_many, d_many_span, K, max_sep, no_overlap, d_out);
}

int obtg_one_vs_many_min_spans(obtg_ctx* c, const double* one, const double* one_span, int B, const double* many,
                               const double* many_span, int K, double max_sep, double no_overlap, double* out)
{
    if (int chk = one_vs_many_args(c, one, B, many, K, out, true, one_span, many_span)) return done(chk);
    const size_t curve = (size_t)c->dim * (c->deg + 1), n = (size_t)B * K;
    HostCall h(c);
    const double* d_one = h.in(c->ws_in, one, curve * B, true);
    const double* d_many = h.in(c->ws_in2, many, curve * K);
    const double* d_one_span = h.in(c->ws_misc[WS_ARG_A], one_span, 2 * (size_t)B);
    const double* d_many_span = h.in(c->ws_misc[WS_ARG_B], many_span, 2 * (size_t)K);
    double* d_out = h.out<double>(c->ws_out, n, true);
    h.run([&] { return launch_one_vs_many_min_spans(c, d_one, d_one_span, B, d_many, d_many_span, K, max_sep, no_overlap, d_out); });
    return h.finish(out, d_out, n);
}

// host_arrays: the perturbation lists are host memory, so their entries can be checked too
static int temporal_sep_fd_args(const obtg_ctx* c, const double* Y0, int n_pert, const int* pert_row, const int* pert_col,
                                const double* pert_val, const double* out_blk, bool host_arrays)
{
    if (!check_ctx(c) || n_pert < 0) return OBTG_ERR_ARG;
    if (n_pert == 0 || c->n_obj < 2) return kNothingToDo;
    if (!Y0 || !pert_row || !pert_col || !pert_val || !out_blk) return OBTG_ERR_ARG;
    for (int t = 0; host_arrays && t < n_pert; ++t)
        if (pert_row[t] < 0 || pert_row[t] >= c->n_veh * c->dim || pert_col[t] < 0 || pert_col[t] > c->deg) return OBTG_ERR_ARG;
    return OBTG_OK;
}

int obtg_temporal_sep_fd(obtg_ctx* c, const double* Y0, int n_pert, const int* pert_row, const int* pert_col,
                         const double* pert_val, double max_sep, double* out_blk)
{
    if (int chk = temporal_sep_fd_args(c, Y0, n_pert, pert_row, pert_col, pert_val, out_blk, true)) return done(chk);
    const size_t n = (size_t)(c->n_obj - 1) * (2 * c->deg + c->R + 1) * n_pert;
    HostCall h(c);
    const double* dY0 = h.in(c->ws_in, Y0, ysize(c));
    const int* d_row = h.in(c->ws_misc[WS_ARG_A], pert_row, (size_t)n_pert);
    const int* d_col = h.in(c->ws_misc[WS_ARG_B], pert_col, (size_t)n_pert);
    const double* d_val = h.in(c->ws_in2, pert_val, (size_t)n_pert);
    double* d_out = h.out<double>(c->ws_out, n);
    h.run([&] { return launch_temporal_sep_fd(c, dY0, n_pert, d_row, d_col, d_val, max_sep, d_out); });
    return h.finish(out_blk, d_out, n);
}

int obtg_temporal_sep_fd_dev(obtg_ctx* c, const double* dY0, int n_pert, const int* d_pert_row,
                             const int* d_pert_col, const double* d_pert_val, double max_sep, double* d_out_blk)
{
    if (int chk = temporal_sep_fd_args(c, dY0, n_pert, d_pert_row, d_pert_col, d_pert_val, d_out_blk, false)) return done(chk);
    (void)hipSetDevice(c->device);
    return launch_temporal_sep_fd(c, dY0, n_pert, d_pert_row, d_pert_col, d_pert_val, max_sep, d_out_blk);
}

int obtg_speed(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, int is_max, double* out)
{
    if (!check_ctx(c) || !Y || !tf || !out || B < 0) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)obtg_len_speed(c) * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    const double* d_tf = h.in(c->ws_in2, tf, (size_t)B, true);
    double* d_out = h.out<double>(c->ws_out, n, true);
    h.run([&] { return launch_speed(c, dY, d_tf, B, bound, is_max, d_out); });
    return h.finish(out, d_out, n);
}

// obtg_speed with the source curve one derivative further (the rows have the speed rows' length)
int obtg_accel(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, double* out)
{
    if (!check_ctx(c) || !Y || !tf || !out || B < 0) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)obtg_len_speed(c) * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    const double* d_tf = h.in(c->ws_in2, tf, (size_t)B, true);
    double* d_out = h.out<double>(c->ws_out, n, true);
    h.run([&] { return launch_speed(c, dY, d_tf, B, bound, 1, d_out, 2); });
    return h.finish(out, d_out, n);
}

// obtg_accel with the source curve one derivative further still
int obtg_jerk(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, double* out)
{
    if (!check_ctx(c) || !Y || !tf || !out || B < 0) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)obtg_len_speed(c) * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    const double* d_tf = h.in(c->ws_in2, tf, (size_t)B, true);
    double* d_out = h.out<double>(c->ws_out, n, true);
    h.run([&] { return launch_speed(c, dY, d_tf, B, bound, 1, d_out, 3); });
    return h.finish(out, d_out, n);
}

int obtg_ang_rate(obtg_ctx* c, const double* Y, const double* tf, int B, double max_rate, double* out)
{
    if (!check_ctx(c) || !Y || !tf || !out || B < 0) return OBTG_ERR_ARG;
    if (c->dim != 2) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)obtg_len_ang_rate(c) * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    const double* d_tf = h.in(c->ws_in2, tf, (size_t)B, true);
    double* d_out = h.out<double>(c->ws_out, n, true);
    h.run([&] { return launch_ang_rate(c, dY, d_tf, B, max_rate, d_out); });
    return h.finish(out, d_out, n);
}

// ------------------------------------------------------------------ GJK
// AoS pts[n][3] + offsets -> SoA per polygon (x[K] y[K] z[K])
static std::vector<double> to_soa(const double* pts, const int* off, int n_poly)
{
    std::vector<double> s((size_t)3 * off[n_poly]);
    for (int a = 0; a < n_poly; ++a) {
        const int o = off[a], K = off[a + 1] - o;
        for (int k = 0; k < K; ++k)
            for (int cdim = 0; cdim < 3; ++cdim) s[(size_t)3 * o + (size_t)cdim * K + k] = pts[(size_t)3 * (o + k) + cdim];
    }
    return s;
}

static int check_polys(const int* off, int n_poly, int n_pts)
{
    if (!off || n_poly < 0) return OBTG_ERR_ARG;
    if (off[0] != 0 || off[n_poly] != n_pts) return OBTG_ERR_ARG;
    for (int a = 0; a < n_poly; ++a) if (off[a + 1] - off[a] < 1) return OBTG_ERR_ARG;
    return OBTG_OK;
}

// ------------------------------------------------------------------ batched searches over a pair list
// The one host path of obtg_gjk_pairs, obtg_gjk_true_pairs, obtg_min_dist[_robust], obtg_min_dist2poly[_robust] and
// obtg_coll_check[2poly].  Every one of them is: its argument checks (check_polys, check_pairs), upload_operands, the
// reservation of its outputs (reserve_search / reserve_gjk), its launcher, the download (download_search / download_gjk).
// The workspace slots are obtg::WsSlot.  The next search entry point starts as a copy of obtg_min_dist_robust (curves
// only) or obtg_min_dist2poly_robust (curves and polygons): nothing but checks, these helpers and a launcher.
// What the entry points do NOT share, because a caller could tell the difference -- each keeps the answer it has given since
// it was added:
//  - the obtg_gjk_* and obtg_min_dist* calls reject null pair / result pointers whatever n_pairs is, the obtg_coll_check*
//    calls only when n_pairs > 0;
//  - obtg_coll_check* answer OBTG_ERR_UNSUPPORTED (more than 16 points) before an empty pair list answers OBTG_OK; in the
//    others that answer is the launcher's, so an empty list is OBTG_OK whatever K is;
//  - obtg_gjk_pairs (as obtg_ctx_set_polygons) counts z == -0.0 as planar; the curve searches ask for +0, because a -0
//    would show in a returned closest point.
extern "C++" {
static int check_pairs(const int* a, int na, const int* b, int nb, int n_pairs)
{
    for (int k = 0; k < n_pairs; ++k)
        if (a[k] < 0 || a[k] >= na || b[k] < 0 || b[k] >= nb) return OBTG_ERR_ARG;
    return OBTG_OK;
}

// every z of curves[n_curves][3][K] is +0 (2-D curves arrive padded with a zero z row, bezier.py:1294-1308): then the planar
// gjkNew machine runs (the same bits)
static bool curves_planar(const double* curves, int n_curves, int K)
{
    for (int i = 0; i < n_curves; ++i) {
        const double* z = curves + ((size_t)i * 3 + 2) * K;
        for (int j = 0; j < K; ++j) if (z[j] != 0.0 || std::signbit(z[j])) return false;
    }
    return true;
}

// every z of pts[n_pts][3] is zero; plus_zero_only: and none of them is -0
static bool polys_planar(const double* pts, int n_pts, bool plus_zero_only)
{
    for (int k = 0; k < n_pts; ++k) {
        const double z = pts[3 * (size_t)k + 2];
        if (z != 0.0 || (plus_zero_only && std::signbit(z))) return false;
    }
    return true;
}

// every one of a[n] is finite.  The planar gjkNew machine (gjk_device.h) keeps the terms of the reference's 3-D arithmetic that
// survive z == 0: those it drops are +-0 for finite x and y only (0 * inf and 0 * nan are NaN in the reference's cross and dot
// products).  The collision checks return the reference's value on non-finite input, so they send it to the 3-D machine.
static bool all_finite(const double* a, size_t n)
{
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
    return true;
}

static int max_poly_size(const int* off, int n_poly)
{
    int max_K = 0;
    for (int a = 0; a < n_poly; ++a) max_K = std::max(max_K, off[a + 1] - off[a]);
    return max_K;
}

// the polygons of one call as the kernels read them; lives until the entry point returns (the uploads are asynchronous)
struct PolySoa {
    const int* off;
    int n_poly, max_K;
    std::vector<double> soa;
    PolySoa(const double* pts, const int* off_, int n_poly_)
        : off(off_), n_poly(n_poly_), max_K(max_poly_size(off_, n_poly_)), soa(to_soa(pts, off_, n_poly_)) {}
};

// curves (nullptr: none) -> ws_in; polygons (nullptr: none) -> ws_in2, or ws_in where there are no curves, and their
// offsets -> WS_POLY_OFF; the pair lists -> WS_PAIR_A, WS_PAIR_B
static int upload_operands(obtg_ctx* c, const double* curves, int n_curves, int K, const PolySoa* polys, const int* pair_a,
                           const int* pair_b, int n_pairs)
{
    int rc;
    if (curves && (rc = h2d(c, c->ws_in, curves, sizeof(double) * 3 * (size_t)K * n_curves))) return rc;
    if (polys) {
        if ((rc = h2d(c, curves ? c->ws_in2 : c->ws_in, polys->soa.data(), polys->soa.size() * sizeof(double)))) return rc;
        if ((rc = h2d(c, c->ws_misc[WS_POLY_OFF], polys->off, sizeof(int) * (polys->n_poly + 1)))) return rc;
    }
    if ((rc = h2d(c, c->ws_misc[WS_PAIR_A], pair_a, sizeof(int) * n_pairs))) return rc;
    return h2d(c, c->ws_misc[WS_PAIR_B], pair_b, sizeof(int) * n_pairs);
}

// device side of a curve search's outputs: its frame stacks, res[width][n_pairs] in ws_out, info[4 n_pairs]
static int reserve_search(obtg_ctx* c, size_t stack_doubles, int width, int n_pairs)
{
    int rc = c->ws_misc[WS_STACK].reserve(sizeof(double) * stack_doubles);
    if (rc) return rc;
    if ((rc = c->ws_out.reserve(sizeof(double) * width * (size_t)n_pairs))) return rc;
    return c->ws_misc[WS_INFO].reserve(sizeof(int) * 4 * (size_t)n_pairs);
}

// results of a curve search: info, then res (the copy that synchronises); info and status are optional
static int download_search(obtg_ctx* c, int n_pairs, int width, double* res, int* info, int* status)
{
    std::vector<int> hinfo((size_t)4 * n_pairs);
    int rc = d2h_copy(c, hinfo.data(), c->ws_misc[WS_INFO].p, sizeof(int) * 4 * n_pairs);
    if (rc) return rc;
    if ((rc = d2h(c, res, c->ws_out.p, sizeof(double) * width * n_pairs))) return rc;
    if (info) std::memcpy(info, hinfo.data(), sizeof(int) * 4 * n_pairs);
    if (status) for (int k = 0; k < n_pairs; ++k) status[k] = hinfo[4 * k + 3];
    return OBTG_OK;
}

// device side of a GJK call's outputs (obtg_gjk_swarm's too): flag | aux (n_support or iters) | status in WS_INFO;
// p1 | p2 | dist (| lower: `doubles` = 8) in ws_out
struct GjkOut { int *flag, *aux, *status; double *p1, *p2, *dist; };
static int reserve_gjk(obtg_ctx* c, size_t n, int doubles, GjkOut& o)
{
    int rc = c->ws_misc[WS_INFO].reserve(sizeof(int) * 3 * n);
    if (rc) return rc;
    if ((rc = c->ws_out.reserve(sizeof(double) * doubles * n))) return rc;
    o.flag = slot<int>(c, WS_INFO); o.aux = o.flag + n; o.status = o.aux + n;
    o.p1 = c->ws_out.as<double>(); o.p2 = o.p1 + 3 * n; o.dist = o.p2 + 3 * n;
    return OBTG_OK;
}

// every output the GJK calls share but dist, which each copies last (the copy that synchronises); aux and status are optional
static int download_gjk(obtg_ctx* c, const GjkOut& o, size_t n, int* flag, int* aux, int* status, double* p1, double* p2)
{
    int rc = d2h_copy(c, flag, o.flag, sizeof(int) * n);
    if (rc) return rc;
    if (aux && (rc = d2h_copy(c, aux, o.aux, sizeof(int) * n))) return rc;
    if (status && (rc = d2h_copy(c, status, o.status, sizeof(int) * n))) return rc;
    if ((rc = d2h_copy(c, p1, o.p1, sizeof(double) * 3 * n))) return rc;
    return d2h_copy(c, p2, o.p2, sizeof(double) * 3 * n);
}
}  // extern "C++"

int obtg_gjk_pairs(obtg_ctx* c, const double* pts, int n_pts, const int* poly_off, int n_poly,
                   const int* pair_a, const int* pair_b, int n_pairs, int max_iter, int md_cap, int* flag,
                   double* p1, double* p2, double* dist, short* support_trace, int trace_cap,
                   int* n_support, int* status)
{
    if (!check_ctx(c) || !pts || !pair_a || !pair_b || !flag || !p1 || !p2 || !dist) return OBTG_ERR_ARG;
    if (n_pairs < 0 || max_iter < 1 || md_cap < 1 || trace_cap < 0) return OBTG_ERR_ARG;
    int rc = check_polys(poly_off, n_poly, n_pts);
    if (rc) return rc;
    if ((rc = check_pairs(pair_a, n_poly, pair_b, n_poly, n_pairs))) return rc;
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    const PolySoa polys(pts, poly_off, n_poly);
    if ((rc = upload_operands(c, nullptr, 0, 0, &polys, pair_a, pair_b, n_pairs))) return rc;
    GjkOut o;
    if ((rc = reserve_gjk(c, n_pairs, 7, o))) return rc;
    short* d_trace = nullptr;
    const size_t trace_bytes = sizeof(short) * 2 * (size_t)trace_cap * n_pairs;
    if (support_trace && trace_cap > 0) {
        if ((rc = c->ws_misc[WS_TRACE].reserve(trace_bytes))) return rc;
        d_trace = slot<short>(c, WS_TRACE);
        OBTG_HIP(c, hipMemsetAsync(d_trace, 0, trace_bytes, c->stream));
    }
    rc = launch_gjk_pairs(c, c->ws_in.as<double>(), slot<int>(c, WS_POLY_OFF), slot<int>(c, WS_PAIR_A), slot<int>(c, WS_PAIR_B),
                          n_pairs, max_iter, md_cap, o.flag, o.p1, o.p2, o.dist, d_trace, trace_cap, o.aux, o.status,
                          polys_planar(pts, n_pts, false));
    if (rc) return rc;
    if ((rc = download_gjk(c, o, n_pairs, flag, n_support, status, p1, p2))) return rc;
    if (d_trace) OBTG_HIP(c, hipMemcpyAsync(support_trace, d_trace, trace_bytes, hipMemcpyDeviceToHost, c->stream));
    return d2h(c, dist, o.dist, sizeof(double) * n_pairs);
}

int obtg_gjk_true_pairs(obtg_ctx* c, const double* pts, int n_pts, const int* poly_off, int n_poly, const int* pair_a,
                        const int* pair_b, int n_pairs, double eps, int max_iter, int* flag, double* p1, double* p2,
                        double* dist, double* lower, int* iters, int* status)
{
    if (!check_ctx(c) || !pts || !pair_a || !pair_b || !flag || !p1 || !p2 || !dist) return OBTG_ERR_ARG;
    if (n_pairs < 0 || max_iter < 1 || !(eps > 0)) return OBTG_ERR_ARG;
    int rc = check_polys(poly_off, n_poly, n_pts);
    if (rc) return rc;
    if ((rc = check_pairs(pair_a, n_poly, pair_b, n_poly, n_pairs))) return rc;
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    const PolySoa polys(pts, poly_off, n_poly);
    if ((rc = upload_operands(c, nullptr, 0, 0, &polys, pair_a, pair_b, n_pairs))) return rc;
    GjkOut o;
    if ((rc = reserve_gjk(c, n_pairs, 8, o))) return rc;
    double* d_lower = o.dist + n_pairs;
    rc = launch_gjk_true_pairs(c, c->ws_in.as<double>(), slot<int>(c, WS_POLY_OFF), slot<int>(c, WS_PAIR_A),
                               slot<int>(c, WS_PAIR_B), n_pairs, eps, max_iter, o.flag, o.p1, o.p2, o.dist, d_lower, o.aux,
                               o.status);
    if (rc) return rc;
    if ((rc = download_gjk(c, o, n_pairs, flag, iters, status, p1, p2))) return rc;
    if (lower && (rc = d2h_copy(c, lower, d_lower, sizeof(double) * n_pairs))) return rc;
    return d2h(c, dist, o.dist, sizeof(double) * n_pairs);
}

int obtg_ctx_set_polygons(obtg_ctx* c, const double* pts, int n_pts, const int* poly_off, int n_poly)
{
    if (!check_ctx(c) || n_poly < 0 || n_pts < 0) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    if (n_poly == 0) {
        c->n_poly = 0; c->n_poly_pts = 0; c->polys_planar = true; c->max_poly_K = 0;
        c->n_hull_pairs = 0; c->hull_pairs_set = false; c->tile_valid = false; c->gjk_len_rows = 0;
        int zero = 0;
        return upload(c, c->d_poly_off, &zero, sizeof(int));
    }
    if (!pts) return OBTG_ERR_ARG;
    int rc = check_polys(poly_off, n_poly, n_pts);
    if (rc) return rc;
    auto soa = to_soa(pts, poly_off, n_poly);
    if ((rc = upload(c, c->d_poly_pts, soa.data(), soa.size() * sizeof(double)))) return rc;
    if ((rc = upload(c, c->d_poly_off, poly_off, sizeof(int) * (n_poly + 1)))) return rc;
    c->n_poly = n_poly; c->n_poly_pts = n_pts;
    c->polys_planar = polys_planar(pts, n_pts, false);
    c->max_poly_K = max_poly_size(poly_off, n_poly);
    c->n_hull_pairs = 0;   // object ids may have changed meaning
    c->hull_pairs_set = false;
    c->tile_valid = false;
    c->gjk_len_rows = 0;
    return OBTG_OK;
}

int obtg_ctx_set_hull_pairs(obtg_ctx* c, const int* pair_a, const int* pair_b, int n_pairs)
{
    if (!check_ctx(c) || n_pairs < 0 || (n_pairs && (!pair_a || !pair_b))) return OBTG_ERR_ARG;
    const int n_objs = c->n_veh + c->n_poly;
    for (int k = 0; k < n_pairs; ++k)
        if (pair_a[k] < 0 || pair_a[k] >= n_objs || pair_b[k] < 0 || pair_b[k] >= n_objs) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    int rc = upload(c, c->d_hp_a, pair_a, sizeof(int) * (size_t)n_pairs);
    if (rc) return rc;
    if ((rc = upload(c, c->d_hp_b, pair_b, sizeof(int) * (size_t)n_pairs))) return rc;
    c->n_hull_pairs = n_pairs;
    c->hull_pairs_set = false;             // (true again once EVERY table of the list is on the device: a failed upload below
                                           //  must not leave the previous list's per-vehicle index marked valid)
    c->h_hp_a.assign(pair_a, pair_a + n_pairs);
    c->h_hp_b.assign(pair_b, pair_b + n_pairs);
    {   // which pairs contain vehicle v (list order): what a finite-difference row that moves v has to re-evaluate
        std::vector<int> off(c->n_veh + 1, 0), idx;
        for (int k = 0; k < n_pairs; ++k) {
            if (pair_a[k] < c->n_veh) ++off[pair_a[k] + 1];
            if (pair_b[k] < c->n_veh && pair_b[k] != pair_a[k]) ++off[pair_b[k] + 1];
        }
        for (int v = 0; v < c->n_veh; ++v) off[v + 1] += off[v];
        idx.resize((size_t)off[c->n_veh] + 1);
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int k = 0; k < n_pairs; ++k) {
            if (pair_a[k] < c->n_veh) idx[fill[pair_a[k]]++] = k;
            if (pair_b[k] < c->n_veh && pair_b[k] != pair_a[k]) idx[fill[pair_b[k]]++] = k;
        }
        if ((rc = upload(c, c->d_vp_off, off.data(), sizeof(int) * off.size()))) return rc;
        if ((rc = upload(c, c->d_vp_idx, idx.data(), sizeof(int) * idx.size()))) return rc;
    }
    c->tile_valid = false;
    c->gjk_len_rows = 0;
    if (c->d_poly_off.p == nullptr) {
        int zero = 0;
        if ((rc = upload(c, c->d_poly_off, &zero, sizeof(int)))) return rc;
    }
    if (c->d_poly_pts.p == nullptr && (rc = c->d_poly_pts.reserve(8))) return rc;
    c->hull_pairs_set = true;
    return OBTG_OK;
}

int obtg_ctx_set_fd_dedup(obtg_ctx* c, int on)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    c->fd_dedup = on != 0;
    return OBTG_OK;
}

int obtg_ctx_set_fd_view_structured(obtg_ctx* c, int on)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    c->fd_view_structured = on != 0;
    return OBTG_OK;
}

int obtg_sweep_shape(obtg_ctx* c, int B, int which, int want_dyn, int* out)
{
    if (!check_ctx(c) || !out || B < 1 || (which != 0 && which != 1)) return OBTG_ERR_ARG;
    if (!c->hull_pairs_set || c->n_hull_pairs <= 0) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return sweep_shape_query(c, B, which, want_dyn != 0, out);
}

int obtg_pair_sweep_dev(obtg_ctx* c, const double* dY, int B, double max_sep, double* d_out_sep, int max_iter,
                        int md_cap, int* d_flag, double* d_p1, double* d_p2, double* d_dist, int* d_nsup,
                        int* d_status)
{
    if (!check_ctx(c) || !d_out_sep || !d_flag || !d_p1 || !d_p2 || !d_dist || B < 0 || max_iter < 1 ||
        md_cap < 1) return OBTG_ERR_ARG;
    if (!c->hull_pairs_set) return OBTG_ERR_ARG;   // no pair list registered (or invalidated by obtg_ctx_set_polygons)
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, pair_sweep_can_fd(c), [&](const double* src) {
        return launch_pair_sweep(c, src, B, max_sep, d_out_sep, max_iter, md_cap, d_flag, d_p1, d_p2, d_dist, d_nsup, d_status); });
}

int obtg_constraint_sweep_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double max_sep, double* d_out_sep,
                              double speed_bound, int speed_is_max, double max_rate, double* d_out_speed,
                              double* d_out_ang, int max_iter, int md_cap, int* d_flag, double* d_p1, double* d_p2,
                              double* d_dist, int* d_nsup, int* d_status)
{
    if (!check_ctx(c) || !d_tf || !d_out_sep || !d_out_speed || !d_flag || !d_p1 || !d_p2 || !d_dist || B < 0 ||
        max_iter < 1 || md_cap < 1) return OBTG_ERR_ARG;
    if (!c->hull_pairs_set) return OBTG_ERR_ARG;
    if (d_out_ang && c->dim != 2) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    // The whole batch of an open view, every family wanted: its rows are row 0 with one control point of one vehicle
    // advanced, and the structured step (k_step_fd_structured) fills the same arrays with the same bits without evaluating
    // row 0's pairs and vehicles again for every row.  Decided before anything is launched: only shapes the structured
    // kernel covers, and only where the brute-force form is itself ONE launch (DEG_ELEV > 0 keeps its two launches); any
    // other shape takes the path below with no launch spent and the sweep's trip-count history untouched.
    if (!dY && c->view.Y0 && B == c->view.B && B > 0 && !c->view.materialised && d_out_ang && c->fd_view_structured &&
        constraint_sweep_is_one_launch(c, B) && step_fd_structured_supported(c)) {
        SweepFold sp;
        sp.d_tf = d_tf; sp.speed_bound = speed_bound; sp.speed_is_max = speed_is_max;
        sp.d_out_speed = d_out_speed; sp.d_out_ang = d_out_ang; sp.max_rate = max_rate;
        c->fd.Y0 = c->view.Y0; c->fd.h = c->view.h; c->fd.fixed = c->view.fixed; c->fd.row0 = c->view.row0;
        const int rc = launch_step_fd_structured(c, B, max_sep, d_out_sep, max_iter, md_cap, d_flag, d_p1, d_p2, d_dist, d_nsup, d_status, &sp);
        c->fd.Y0 = nullptr; c->fd.row0 = 0;
        if (rc != OBTG_ERR_UNSUPPORTED) return rc;     // (the launcher answers that before it launches: the brute-force sweep below)
    }
    return with_batch(c, dY, B, pair_sweep_can_fd(c) && dynamics_can_fd(c, true, d_out_ang != nullptr), [&](const double* src) {
        SweepFold sp;
        sp.d_tf = d_tf; sp.speed_bound = speed_bound; sp.speed_is_max = speed_is_max;
        sp.d_out_speed = d_out_speed; sp.d_out_ang = d_out_ang; sp.max_rate = max_rate;
        int rc = launch_pair_sweep(c, src, B, max_sep, d_out_sep, max_iter, md_cap, d_flag, d_p1, d_p2, d_dist, d_nsup, d_status, &sp);
        if (rc) return rc;
        if (sp.did_dynamics || (sp.did_speed && !d_out_ang)) return (int)OBTG_OK;
        return launch_dynamics(c, src, d_tf, B, speed_bound, speed_is_max, max_rate, d_out_speed, d_out_ang);
    });
}

int obtg_constraint_sweep_fd_structured_rows_dev(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, int row_begin,
                                                 const double* d_tf, int B, double max_sep, double* d_out_sep, double speed_bound,
                                                 int speed_is_max, double max_rate, double* d_out_speed, double* d_out_ang,
                                                 int max_iter, int md_cap, int* d_flag, double* d_p1, double* d_p2, double* d_dist,
                                                 int* d_nsup, int* d_status)
{
    if (!check_ctx(c) || !dY0 || !d_tf || !d_out_sep || !d_out_speed || !d_out_ang || !d_flag || !d_p1 || !d_p2 || !d_dist ||
        B < 1 || row_begin < 0 || max_iter < 1 || md_cap < 1) return OBTG_ERR_ARG;
    if (!c->hull_pairs_set || c->dim != 2) return OBTG_ERR_ARG;
    if (c->view.Y0) return OBTG_ERR_ARG;       // a view of the caller's is open: this call is a view of its own and would replace and close it
    int rc = obtg_fd_view_begin_rows(c, dY0, n_fixed_cols, h, row_begin, B);
    if (rc) return rc;
    (void)hipSetDevice(c->device);
    SweepFold sp;
    sp.d_tf = d_tf; sp.speed_bound = speed_bound; sp.speed_is_max = speed_is_max;
    sp.d_out_speed = d_out_speed; sp.d_out_ang = d_out_ang; sp.max_rate = max_rate;
    c->fd.Y0 = c->view.Y0; c->fd.h = c->view.h; c->fd.fixed = c->view.fixed; c->fd.row0 = c->view.row0;
    rc = launch_step_fd_structured(c, B, max_sep, d_out_sep, max_iter, md_cap, d_flag, d_p1, d_p2, d_dist, d_nsup, d_status, &sp);
    c->fd.Y0 = nullptr; c->fd.row0 = 0;
    (void)obtg_fd_view_end(c);
    return rc;
}

int obtg_constraint_sweep_fd_structured_dev(obtg_ctx* c, const double* dY0, int n_fixed_cols, double h, const double* d_tf, int B,
                                            double max_sep, double* d_out_sep, double speed_bound, int speed_is_max, double max_rate,
                                            double* d_out_speed, double* d_out_ang, int max_iter, int md_cap, int* d_flag,
                                            double* d_p1, double* d_p2, double* d_dist, int* d_nsup, int* d_status)
{
    return obtg_constraint_sweep_fd_structured_rows_dev(c, dY0, n_fixed_cols, h, 0, d_tf, B, max_sep, d_out_sep, speed_bound, speed_is_max,
                                                        max_rate, d_out_speed, d_out_ang, max_iter, md_cap, d_flag, d_p1, d_p2, d_dist,
                                                        d_nsup, d_status);
}

int obtg_ctx_set_gjk_history(obtg_ctx* c, int on)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    c->gjk_history = on != 0;
    c->gjk_len_rows = 0;
    return OBTG_OK;
}

int obtg_gjk_swarm_dev(obtg_ctx* c, const double* dY, int B, int max_iter, int md_cap, int* d_flag,
                       double* d_p1, double* d_p2, double* d_dist, int* d_nsup, int* d_status)
{
    if (!check_ctx(c) || !d_flag || !d_p1 || !d_p2 || !d_dist || B < 0) return OBTG_ERR_ARG;
    if (max_iter < 1 || md_cap < 1) return OBTG_ERR_ARG;
    if (c->dim < 2) return OBTG_ERR_ARG;   // bezier.py:847-851: curves must be 2-D or 3-D
    if (!c->hull_pairs_set) return OBTG_ERR_ARG;   // no pair list registered (or invalidated by obtg_ctx_set_polygons)
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, true, [&](const double* src) {
        return launch_gjk_swarm(c, src, B, max_iter, md_cap, d_flag, d_p1, d_p2, d_dist, d_nsup, d_status); });
}

int obtg_gjk_swarm(obtg_ctx* c, const double* Y, int B, int max_iter, int md_cap, int* flag, double* p1,
                   double* p2, double* dist, int* nsup, int* status)
{
    if (!check_ctx(c) || !Y || !flag || !p1 || !p2 || !dist || B < 0) return OBTG_ERR_ARG;
    if (max_iter < 1 || md_cap < 1) return OBTG_ERR_ARG;
    if (c->dim < 2 || !c->hull_pairs_set) return OBTG_ERR_ARG;
    const size_t n = (size_t)B * c->n_hull_pairs;
    if (n == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    int rc = h2d(c, c->ws_in, Y, sizeof(double) * ysize(c) * B);
    if (rc) return rc;
    GjkOut o;
    if ((rc = reserve_gjk(c, n, 7, o))) return rc;
    rc = launch_gjk_swarm(c, c->ws_in.as<double>(), B, max_iter, md_cap, o.flag, o.p1, o.p2, o.dist, o.aux, o.status);
    if (rc) return rc;
    if ((rc = download_gjk(c, o, n, flag, nsup, status, p1, p2))) return rc;
    return d2h(c, dist, o.dist, sizeof(double) * n);
}

// ------------------------------------------------------------------ the pair order of obtg_min_dist / obtg_min_dist_mixed
// The order the worker waves take the pairs in: by the previous evaluation's node counts, longest search first, when this very
// pair list was evaluated before (an SLSQP run evaluates one list over and over at nearby x); list order else.
extern "C++" {
struct MdOrder {
    unsigned long long sig;        // of the pair lists (count + hash)
    int hist;                      // its entry of c->md_hist, -1: none yet
    bool have;                     // an order was uploaded behind the queue counter (WS_QUEUE)
    std::vector<int> qbuf;         // [0] the queue counter, [1..] the order: the upload's source, which lives as long as this
                                   // does -- in the entry point, until its synchronising download (the uploads are asynchronous)
};

static int md_order_upload(obtg_ctx* c, const int* pair_a, const int* pair_b, int n_pairs, MdOrder& o)
{
    o.sig = 1469598103934665603ull ^ (unsigned long long)n_pairs;
    for (int k = 0; k < n_pairs; ++k) {
        o.sig = (o.sig ^ (unsigned)pair_a[k]) * 1099511628211ull;
        o.sig = (o.sig ^ (unsigned)pair_b[k]) * 1099511628211ull;
    }
    static const bool use_hist = !(getenv("OBTG_MD_HISTORY") && getenv("OBTG_MD_HISTORY")[0] == '0');
    std::vector<int>& qbuf = o.qbuf;
    qbuf.assign((size_t)n_pairs + 1, 0);
    o.hist = -1;
    for (size_t h = 0; h < c->md_hist.size(); ++h)
        if (c->md_hist[h].sig == o.sig && (int)c->md_hist[h].nodes.size() == n_pairs) o.hist = (int)h;
    o.have = use_hist && o.hist >= 0;
    for (int k = 0; k < n_pairs; ++k) qbuf[1 + k] = k;
    if (o.have) {
        const std::vector<int>& hn = c->md_hist[o.hist].nodes;
        std::stable_sort(qbuf.begin() + 1, qbuf.end(), [&](int a, int b) { return hn[a] > hn[b]; });
    }
    return h2d(c, c->ws_misc[WS_QUEUE], qbuf.data(), sizeof(int) * qbuf.size());
}

// download_search, then this evaluation's node counts become the list's history (most recent last, four lists kept)
static int md_download_record(obtg_ctx* c, const MdOrder& o, int n_pairs, double* res, int* info, int* status)
{
    std::vector<int> own_info;                               // the history needs the node counts whether the caller asked for info or not
    if (!info) { own_info.resize((size_t)4 * n_pairs); info = own_info.data(); }
    const int rc = download_search(c, n_pairs, 3, res, info, status);
    if (rc) return rc;
    if (o.hist >= 0) c->md_hist.erase(c->md_hist.begin() + o.hist);
    if (c->md_hist.size() >= 4) c->md_hist.erase(c->md_hist.begin());
    c->md_hist.push_back({ o.sig, std::vector<int>((size_t)n_pairs) });
    for (int k = 0; k < n_pairs; ++k) c->md_hist.back().nodes[k] = info[4 * k];
    return OBTG_OK;
}
}

// ------------------------------------------------------------------ minDist, collCheck (the host path: "batched searches over a pair list" above)
int obtg_min_dist(obtg_ctx* c, const double* curves, int n_curves, int K, const int* pair_a, const int* pair_b,
                  int n_pairs, double eps, int max_iter, int md_cap, int max_depth, int max_nodes, double* res,
                  int* info, int* status)
{
    if (!check_ctx(c) || !curves || !pair_a || !pair_b || !res || n_curves < 1 || n_pairs < 0) return OBTG_ERR_ARG;
    if (K < 2 || max_iter < 1 || md_cap < 1 || max_depth < 1 || max_nodes < 1) return OBTG_ERR_ARG;
    int rc = check_pairs(pair_a, n_curves, pair_b, n_curves, n_pairs);
    if (rc) return rc;
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    if ((rc = upload_operands(c, curves, n_curves, K, nullptr, pair_a, pair_b, n_pairs))) return rc;
    const bool planar = curves_planar(curves, n_curves, K);
    if ((rc = reserve_search(c, min_dist_stack_doubles(c, K, max_depth, n_pairs, planar), 3, n_pairs))) return rc;
    MdOrder ord;
    if ((rc = md_order_upload(c, pair_a, pair_b, n_pairs, ord))) return rc;
    int* d_queue = slot<int>(c, WS_QUEUE);
    rc = launch_min_dist(c, c->ws_in.as<double>(), K, slot<int>(c, WS_PAIR_A), slot<int>(c, WS_PAIR_B), n_pairs, eps, max_iter,
                         md_cap, max_depth, max_nodes, slot<double>(c, WS_STACK), c->ws_out.as<double>(), slot<int>(c, WS_INFO),
                         ord.have ? d_queue + 1 : nullptr, d_queue, planar);
    if (rc) return rc;
    return md_download_record(c, ord, n_pairs, res, info, status);
}

// _minDist on curves of different degree (bezier.py:1283-1408 takes any two): obtg_min_dist's host path with the curves as
// offsets into one control-point array.  Every K_i equal: the call IS obtg_min_dist (that layout is its curves[n][3][K]).
int obtg_min_dist_mixed(obtg_ctx* c, const double* cpts, const int* curve_off, int n_curves, const int* pair_a,
                        const int* pair_b, int n_pairs, double eps, int max_iter, int md_cap, int max_depth, int max_nodes,
                        double* res, int* info, int* status)
{
    if (!check_ctx(c) || !cpts || !curve_off || !pair_a || !pair_b || !res || n_curves < 1 || n_pairs < 0) return OBTG_ERR_ARG;
    if (max_iter < 1 || md_cap < 1 || max_depth < 1 || max_nodes < 1 || curve_off[0] != 0) return OBTG_ERR_ARG;
    bool equal = true, too_long = false;
    for (int i = 0; i < n_curves; ++i) {
        const int K = curve_off[i + 1] - curve_off[i];
        if (K < 2) return OBTG_ERR_ARG;              // (a non-monotone offset list ends here too)
        too_long |= K > kMdMaxCurveK;
        equal &= K == curve_off[1];
    }
    if (too_long) return OBTG_ERR_UNSUPPORTED;
    int rc = check_pairs(pair_a, n_curves, pair_b, n_curves, n_pairs);
    if (rc) return rc;
    if (equal)
        return obtg_min_dist(c, cpts, n_curves, curve_off[1], pair_a, pair_b, n_pairs, eps, max_iter, md_cap, max_depth, max_nodes,
                             res, info, status);
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    const int n_pts = curve_off[n_curves];
    int kt_max = 0;
    for (int k = 0; k < n_pairs; ++k)
        kt_max = std::max(kt_max, curve_off[pair_a[k] + 1] - curve_off[pair_a[k]] + curve_off[pair_b[k] + 1] - curve_off[pair_b[k]]);
    // (the control points as ONE operand of 3 n_pts doubles: the kernel finds a curve by its offset)
    if ((rc = upload_operands(c, cpts, 1, n_pts, nullptr, pair_a, pair_b, n_pairs))) return rc;
    if ((rc = h2d(c, c->ws_misc[WS_CURVE_OFF], curve_off, sizeof(int) * (n_curves + 1)))) return rc;
    bool planar = true;
    for (int i = 0; i < n_curves && planar; ++i)
        planar = curves_planar(cpts + 3 * (size_t)curve_off[i], 1, curve_off[i + 1] - curve_off[i]);
    const size_t stack = min_dist_mixed_stack_doubles(c, kt_max, max_depth, n_pairs);
    if (!stack) return OBTG_ERR_UNSUPPORTED;         // (max_depth frames of scalars that no workgroup's LDS holds)
    if ((rc = reserve_search(c, stack, 3, n_pairs))) return rc;
    MdOrder ord;
    if ((rc = md_order_upload(c, pair_a, pair_b, n_pairs, ord))) return rc;
    int* d_queue = slot<int>(c, WS_QUEUE);
    rc = launch_min_dist_mixed(c, c->ws_in.as<double>(), slot<int>(c, WS_CURVE_OFF), kt_max, slot<int>(c, WS_PAIR_A),
                               slot<int>(c, WS_PAIR_B), n_pairs, eps, max_iter, md_cap, max_depth, max_nodes,
                               slot<double>(c, WS_STACK), c->ws_out.as<double>(), slot<int>(c, WS_INFO),
                               ord.have ? d_queue + 1 : nullptr, d_queue, planar);
    if (rc) return rc;
    return md_download_record(c, ord, n_pairs, res, info, status);
}

constexpr int kRobustCap = 1024, kRobustMaxLevel = 48;       // frontier capacity per pair and subdivision depth of the robust searches

int obtg_min_dist_robust(obtg_ctx* c, const double* curves, int n_curves, int K, const int* pair_a, const int* pair_b,
                         int n_pairs, double eps, int max_nodes, double* res, int* info, int* status)
{
    if (!check_ctx(c) || !curves || !pair_a || !pair_b || !res || n_curves < 1 || n_pairs < 0) return OBTG_ERR_ARG;
    if (K < 2 || max_nodes < 1 || !(eps > 0)) return OBTG_ERR_ARG;
    int rc = check_pairs(pair_a, n_curves, pair_b, n_curves, n_pairs);
    if (rc) return rc;
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    if ((rc = upload_operands(c, curves, n_curves, K, nullptr, pair_a, pair_b, n_pairs))) return rc;
    if ((rc = reserve_search(c, (size_t)2 * kRobustCap * 3 * n_pairs, 3, n_pairs))) return rc;
    rc = launch_min_dist_robust(c, c->ws_in.as<double>(), K, slot<int>(c, WS_PAIR_A), slot<int>(c, WS_PAIR_B), n_pairs, eps,
                                max_nodes, kRobustMaxLevel, kRobustCap, slot<double>(c, WS_STACK), c->ws_out.as<double>(),
                                slot<int>(c, WS_INFO));
    if (rc) return rc;
    return download_search(c, n_pairs, 3, res, info, status);
}

int obtg_min_dist2poly(obtg_ctx* c, const double* curves, int n_curves, int K, const double* pts, int n_pts,
                       const int* poly_off, int n_poly, const int* pair_curve, const int* pair_poly, int n_pairs,
                       double eps, int max_iter, int md_cap, int max_depth, int max_nodes, double* res, int* info,
                       int* status)
{
    if (!check_ctx(c) || !curves || !pts || !pair_curve || !pair_poly || !res || n_curves < 1 || n_pairs < 0)
        return OBTG_ERR_ARG;
    if (K < 2 || max_iter < 1 || md_cap < 1 || max_depth < 1 || max_nodes < 1) return OBTG_ERR_ARG;
    int rc = check_polys(poly_off, n_poly, n_pts);
    if (rc) return rc;
    if ((rc = check_pairs(pair_curve, n_curves, pair_poly, n_poly, n_pairs))) return rc;
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    const PolySoa polys(pts, poly_off, n_poly);
    if ((rc = upload_operands(c, curves, n_curves, K, &polys, pair_curve, pair_poly, n_pairs))) return rc;
    // 2-D curves against polygons in the plane (bezier.py:1416-1430 pads both with z = 0)
    const bool planar = curves_planar(curves, n_curves, K) && polys_planar(pts, n_pts, true);
    if ((rc = reserve_search(c, min_dist2poly_stack_doubles(K, max_depth, n_pairs, polys.max_K, planar), 5, n_pairs))) return rc;
    rc = launch_min_dist2poly(c, c->ws_in.as<double>(), K, c->ws_in2.as<double>(), slot<int>(c, WS_POLY_OFF), slot<int>(c, WS_PAIR_A),
                              slot<int>(c, WS_PAIR_B), n_pairs, eps, max_iter, md_cap, max_depth, max_nodes,
                              slot<double>(c, WS_STACK), c->ws_out.as<double>(), slot<int>(c, WS_INFO), polys.max_K, planar);
    if (rc) return rc;
    return download_search(c, n_pairs, 5, res, info, status);
}

int obtg_min_dist2poly_robust(obtg_ctx* c, const double* curves, int n_curves, int K, const double* pts, int n_pts,
                              const int* poly_off, int n_poly, const int* pair_curve, const int* pair_poly, int n_pairs,
                              double eps, int max_nodes, double* res, int* info, int* status)
{
    if (!check_ctx(c) || !curves || !pts || !pair_curve || !pair_poly || !res || n_curves < 1 || n_pairs < 0)
        return OBTG_ERR_ARG;
    if (K < 2 || max_nodes < 1 || !(eps > 0)) return OBTG_ERR_ARG;
    int rc = check_polys(poly_off, n_poly, n_pts);
    if (rc) return rc;
    if ((rc = check_pairs(pair_curve, n_curves, pair_poly, n_poly, n_pairs))) return rc;
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    const PolySoa polys(pts, poly_off, n_poly);
    if ((rc = upload_operands(c, curves, n_curves, K, &polys, pair_curve, pair_poly, n_pairs))) return rc;
    if ((rc = reserve_search(c, (size_t)2 * kRobustCap * 2 * n_pairs, 5, n_pairs))) return rc;
    rc = launch_min_dist2poly_robust(c, c->ws_in.as<double>(), K, c->ws_in2.as<double>(), slot<int>(c, WS_POLY_OFF),
                                     slot<int>(c, WS_PAIR_A), slot<int>(c, WS_PAIR_B), n_pairs, eps, max_nodes, kRobustMaxLevel,
                                     kRobustCap, polys.max_K, slot<double>(c, WS_STACK), c->ws_out.as<double>(), slot<int>(c, WS_INFO));
    if (rc) return rc;
    return download_search(c, n_pairs, 5, res, info, status);
}

int obtg_coll_check(obtg_ctx* c, const double* curves, int n_curves, int K, const int* pair_a, const int* pair_b,
                    int n_pairs, double eps, int max_iter, int md_cap, int max_nodes, double* res, int* info, int* status)
{
    if (!check_ctx(c) || !curves || n_curves < 1 || n_pairs < 0) return OBTG_ERR_ARG;
    if (n_pairs > 0 && (!pair_a || !pair_b || !res)) return OBTG_ERR_ARG;
    if (K < 2 || max_iter < 1 || md_cap < 1 || max_nodes < 1) return OBTG_ERR_ARG;
    int rc = check_pairs(pair_a, n_curves, pair_b, n_curves, n_pairs);
    if (rc) return rc;
    if (!coll_check_supported(K, 0)) return OBTG_ERR_UNSUPPORTED;
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    if ((rc = upload_operands(c, curves, n_curves, K, nullptr, pair_a, pair_b, n_pairs))) return rc;
    const bool planar = curves_planar(curves, n_curves, K) && all_finite(curves, (size_t)3 * K * n_curves);
    if ((rc = reserve_search(c, coll_check_stack_doubles(c, K, n_pairs, false, planar), 1, n_pairs))) return rc;
    if ((rc = c->ws_misc[WS_QUEUE].reserve(sizeof(int)))) return rc;
    rc = launch_coll_check(c, c->ws_in.as<double>(), K, slot<int>(c, WS_PAIR_A), slot<int>(c, WS_PAIR_B), n_pairs, eps, max_iter,
                           md_cap, max_nodes, slot<double>(c, WS_STACK), c->ws_out.as<double>(), slot<int>(c, WS_INFO),
                           slot<int>(c, WS_QUEUE), planar);
    if (rc) return rc;
    return download_search(c, n_pairs, 1, res, info, status);
}

int obtg_coll_check2poly(obtg_ctx* c, const double* curves, int n_curves, int K, const double* pts, int n_pts,
                         const int* poly_off, int n_poly, const int* pair_curve, const int* pair_poly, int n_pairs,
                         int max_iter, int md_cap, int max_nodes, double* res, int* info, int* status)
{
    if (!check_ctx(c) || !curves || !pts || n_curves < 1 || n_pairs < 0) return OBTG_ERR_ARG;
    if (n_pairs > 0 && (!pair_curve || !pair_poly || !res)) return OBTG_ERR_ARG;
    if (K < 2 || max_iter < 1 || md_cap < 1 || max_nodes < 1) return OBTG_ERR_ARG;
    int rc = check_polys(poly_off, n_poly, n_pts);
    if (rc) return rc;
    if ((rc = check_pairs(pair_curve, n_curves, pair_poly, n_poly, n_pairs))) return rc;
    if (!coll_check_supported(K, max_poly_size(poly_off, n_poly))) return OBTG_ERR_UNSUPPORTED;
    if (n_pairs == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    const PolySoa polys(pts, poly_off, n_poly);
    if ((rc = upload_operands(c, curves, n_curves, K, &polys, pair_curve, pair_poly, n_pairs))) return rc;
    const bool planar = curves_planar(curves, n_curves, K) && polys_planar(pts, n_pts, true) &&
                        all_finite(curves, (size_t)3 * K * n_curves) && all_finite(pts, (size_t)3 * n_pts);
    if ((rc = reserve_search(c, coll_check_stack_doubles(c, K, n_pairs, true, planar), 1, n_pairs))) return rc;
    if ((rc = c->ws_misc[WS_QUEUE].reserve(sizeof(int)))) return rc;
    rc = launch_coll_check2poly(c, c->ws_in.as<double>(), K, c->ws_in2.as<double>(), slot<int>(c, WS_POLY_OFF), slot<int>(c, WS_PAIR_A),
                                slot<int>(c, WS_PAIR_B), n_pairs, max_iter, md_cap, max_nodes, slot<double>(c, WS_STACK),
                                c->ws_out.as<double>(), slot<int>(c, WS_INFO), slot<int>(c, WS_QUEUE), polys.max_K, planar);
    if (rc) return rc;
    return download_search(c, n_pairs, 1, res, info, status);
}

// ------------------------------------------------------------------ true Bernstein extrema (extrema_kernels.hip)
static int bern_extrema_args(const obtg_ctx* c, const double* coef, int M, int K, double eps_rel, double eps_abs, int max_nodes,
                             const double* val, bool need_status, const int* status)
{
    if (!check_ctx(c) || M < 0 || !bern_extrema_supported(K) || max_nodes < 1) return OBTG_ERR_ARG;
    if (!(eps_rel >= 0.0) || !(eps_abs >= 0.0)) return OBTG_ERR_ARG;
    if (M > 0 && (!coef || !val || (need_status && !status))) return OBTG_ERR_ARG;
    return OBTG_OK;
}

int obtg_bern_extrema_dev(obtg_ctx* c, const double* d_c, int M, int K, int want_max, double eps_rel, double eps_abs,
                          int max_nodes, double* d_val, double* d_t_star, double* d_bound, int* d_nodes, int* d_status)
{
    if (int rc = bern_extrema_args(c, d_c, M, K, eps_rel, eps_abs, max_nodes, d_val, false, d_status)) return rc;
    (void)hipSetDevice(c->device);
    return launch_bern_extrema(c, d_c, M, K, want_max != 0, eps_rel, eps_abs, max_nodes, d_val, d_t_star, d_bound, d_nodes,
                               d_status);
}

int obtg_bern_extrema(obtg_ctx* c, const double* coef, int M, int K, int want_max, double eps_rel, double eps_abs,
                      int max_nodes, double* val, double* t_star, double* bound, int* nodes, int* status)
{
    if (int rc = bern_extrema_args(c, coef, M, K, eps_rel, eps_abs, max_nodes, val, true, status)) return rc;
    if (M == 0) return OBTG_OK;
    const size_t m = (size_t)M;
    HostCall h(c);
    const double* d_c = h.in(c->ws_in, coef, m * K);
    double* dv = h.out<double>(c->ws_out, 3 * m);         // val | t_star | bound
    int* dn = h.out<int>(c->ws_misc[WS_INFO], 2 * m);      // nodes | status
    h.run([&] { return launch_bern_extrema(c, d_c, M, K, want_max != 0, eps_rel, eps_abs, max_nodes, dv, dv + m, dv + 2 * m, dn, dn + m); });
    h.fetch(t_star, dv + m, m);
    h.fetch(bound, dv + 2 * m, m);
    h.fetch(nodes, dn, m);
    h.fetch(status, dn + m, m);
    return h.finish(val, dv, m);
}

// ------------------------------------------------------------------ the true-minimum row families
// The one path of obtg_temporal_sep_true_min[_jac][_dev], obtg_speed_true_min[_jac][_dev], obtg_accel_true_min[_jac][_dev],
// obtg_jerk_true_min[_jac][_dev] and obtg_ang_rate_true_min[_jac][_dev]: each entry point is its own argument check and its family's descriptor
// (obtg_internal.h RowFamily); the launch chain (true_min_chain), the host body (true_min_host) and the _dev body
// (true_min_dev) are shared.  A further family starts as a copy of the speed entry points, as the angular-rate ones did
// (they answer as the speed calls do, and dim != 2 with OBTG_ERR_ARG).
// What the entry points do NOT share -- each keeps the answer it has given since it was added:
//  - check style: the separation calls check with a bool (true_min_args_ok), the speed calls with a code (speed_true_min_args);
//  - deg > 31: the speed calls answer OBTG_ERR_UNSUPPORTED before the Y / jac check and before the empty batch;
//    obtg_temporal_sep_true_min_jac answers it only from inside the chain (an empty batch or a context without pairs
//    answers OBTG_OK first; its _dev twin has no such early answer); obtg_temporal_sep_true_min answers it from
//    bern_extrema_supported(2 deg + 1), so only with items to evaluate;
//  - the empty case: B == 0 || n_pairs == 0 for separation, B == 0 for speed, both after the pointer checks;
//  - optional outputs: t_star, status, jac_tf; required: out, jac, tf;
//  - launches per route, all timed under the family's kernel id: fused 1; blocks in a launch of their own on a listed
//    degree (OBTG_TRUE_MIN_JAC_FUSED=0) 2; a degree off the list 2 for values, 3 with blocks.
//
// The chain: the fused kernel where the shape has one (with the blocks, d_jac set, only if true_min_jac_fused); else the
// values -- the fused value kernel, or the family's rows at R = 0 into a workspace and obtg_bern_extrema on them (the family's
// own search where it names one: the curvature rows' two polynomials) -- and then the blocks from Y and t_star (and the rows'
// values) in a launch of their own.
static int true_min_chain(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double eps_rel, int max_nodes, double* d_out,
                          double* d_t, int* d_status, double* d_jac, double* d_jac_tf)
{
    if (d_jac && c->deg + 1 > 32) return OBTG_ERR_UNSUPPORTED;
    int rc = OBTG_ERR_UNSUPPORTED;
    if (!d_jac || c->true_min_jac_fused) rc = launch_true_min(c, f, dY, B, eps_rel, max_nodes, d_out, d_t, d_status, d_jac, d_jac_tf);
    if (rc != OBTG_ERR_UNSUPPORTED) return rc;
    if (d_jac) {
        if (!d_t) {
            DevBuf& wt = c->ws_misc[WS_L_TSTAR];
            if ((rc = wt.reserve(sizeof(double) * (size_t)B * f.items))) return rc;
            d_t = wt.as<double>();
        }
        rc = launch_true_min(c, f, dY, B, eps_rel, max_nodes, d_out, d_t, d_status);
    }
    if (rc == OBTG_ERR_UNSUPPORTED) {
        const int K = row_len(f, c->deg);
        if (!bern_extrema_supported(K)) return OBTG_ERR_UNSUPPORTED;
        const long items = (long)B * f.items;
        DevBuf& ws = c->ws_misc[WS_L_ROWS];
        if ((rc = ws.reserve(sizeof(double) * (size_t)items * K * f.ws_rows))) return rc;
        if ((rc = f.rows_r0(c, f, dY, B, ws.as<double>()))) return rc;
        rc = f.search ? f.search(c, f, ws.as<double>(), items, eps_rel, max_nodes, d_out, d_t, d_status)
                      : launch_bern_extrema(c, ws.as<double>(), items, K, 0, eps_rel, 0.0, max_nodes, d_out, d_t, nullptr, nullptr, d_status,
                                            f.kernel_id);
    }
    if (rc || !d_jac) return rc;
    return launch_true_min_envelope(c, f, dY, B, d_t, d_jac, d_jac_tf, d_out);
}

// the host body: Y (and tf, where the family has one) up, val | t_star | jac_tf | jac in ws_out, status in WS_STATUS
static int true_min_host(obtg_ctx* c, RowFamily f, const double* Y, const double* tf, int B, double eps_rel, int max_nodes,
                         double* out, double* t_star, int* status, double* jac, double* jac_tf)
{
    const size_t n = (size_t)B * f.items, nj = jac ? n * c->dim * (c->deg + 1) : 0;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    if (tf) f.d_tf = h.in(c->ws_in2, tf, (size_t)B, true);
    double* dv = h.out<double>(c->ws_out, (jac ? 3 : 2) * n + nj);
    int* ds = h.out<int>(c->ws_misc[WS_STATUS], n);
    double* dj = jac ? dv + 3 * n : nullptr;
    h.run([&] { return true_min_chain(c, f, dY, B, eps_rel, max_nodes, dv, dv + n, ds, dj, jac ? dv + 2 * n : nullptr); });
    h.fetch(t_star, dv + n, n);
    h.fetch(status, ds, n);
    h.fetch(jac_tf, dv + 2 * n, n);
    h.fetch(jac, dj, nj);
    return h.finish(out, dv, n);
}

static int true_min_dev(obtg_ctx* c, const RowFamily& f, const double* dY, int B, double eps_rel, int max_nodes, double* d_out,
                        double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf)
{
    (void)hipSetDevice(c->device);
    return with_batch(c, dY, B, false, [&](const double* src) {
        return true_min_chain(c, f, src, B, eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac, d_jac_tf); });
}

// what obtg_temporal_sep_true_min[_jac] and their _dev twins check alike (the host calls: Y too; the _jac calls: jac too)
static bool true_min_args_ok(const obtg_ctx* c, const double* out, int B, int max_nodes, double eps_rel)
{
    return check_ctx(c) && out && B >= 0 && max_nodes >= 1 && eps_rel >= 0.0;
}

int obtg_temporal_sep_true_min_dev(obtg_ctx* c, const double* dY, int B, double max_sep, double eps_rel, int max_nodes,
                                   double* d_out, double* d_t_star, int* d_status)
{
    if (!true_min_args_ok(c, d_out, B, max_nodes, eps_rel)) return OBTG_ERR_ARG;
    return true_min_dev(c, tsep_row_family(c, max_sep), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, nullptr, nullptr);
}

int obtg_temporal_sep_true_min(obtg_ctx* c, const double* Y, int B, double max_sep, double eps_rel, int max_nodes,
                               double* out, double* t_star, int* status)
{
    if (!true_min_args_ok(c, out, B, max_nodes, eps_rel) || !Y) return OBTG_ERR_ARG;
    if (B == 0 || c->n_pairs == 0) return OBTG_OK;
    return true_min_host(c, tsep_row_family(c, max_sep), Y, nullptr, B, eps_rel, max_nodes, out, t_star, status, nullptr, nullptr);
}

int obtg_temporal_sep_true_min_jac_dev(obtg_ctx* c, const double* dY, int B, double max_sep, double eps_rel, int max_nodes,
                                       double* d_out, double* d_t_star, int* d_status, double* d_jac)
{
    if (!true_min_args_ok(c, d_out, B, max_nodes, eps_rel) || !d_jac) return OBTG_ERR_ARG;
    return true_min_dev(c, tsep_row_family(c, max_sep), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac, nullptr);
}

int obtg_temporal_sep_true_min_jac(obtg_ctx* c, const double* Y, int B, double max_sep, double eps_rel, int max_nodes,
                                   double* out, double* t_star, int* status, double* jac)
{
    if (!true_min_args_ok(c, out, B, max_nodes, eps_rel) || !Y || !jac) return OBTG_ERR_ARG;
    if (B == 0 || c->n_pairs == 0) return OBTG_OK;
    return true_min_host(c, tsep_row_family(c, max_sep), Y, nullptr, B, eps_rel, max_nodes, out, t_star, status, jac, nullptr);
}

// what obtg_speed_true_min[_jac] and their _dev twins check alike (the host calls: Y too; the _jac calls: jac too)
static int speed_true_min_args(const obtg_ctx* c, const double* tf, const double* out, int B, int max_nodes, double eps_rel)
{
    if (!check_ctx(c) || !tf || !out || B < 0 || max_nodes < 1 || !(eps_rel >= 0.0)) return OBTG_ERR_ARG;
    return c->deg > 31 ? OBTG_ERR_UNSUPPORTED : OBTG_OK;
}

int obtg_speed_true_min_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, int is_max, double eps_rel,
                            int max_nodes, double* d_out, double* d_t_star, int* d_status)
{
    if (int rc = speed_true_min_args(c, d_tf, d_out, B, max_nodes, eps_rel)) return rc;
    return true_min_dev(c, speed_row_family(c, d_tf, bound, is_max), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, nullptr,
                        nullptr);
}

int obtg_speed_true_min(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, int is_max, double eps_rel,
                        int max_nodes, double* out, double* t_star, int* status)
{
    if (int rc = speed_true_min_args(c, tf, out, B, max_nodes, eps_rel)) return rc;
    if (!Y) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, speed_row_family(c, nullptr, bound, is_max), Y, tf, B, eps_rel, max_nodes, out, t_star, status, nullptr,
                         nullptr);
}

int obtg_speed_true_min_jac_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, int is_max, double eps_rel,
                                int max_nodes, double* d_out, double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf)
{
    if (int rc = speed_true_min_args(c, d_tf, d_out, B, max_nodes, eps_rel)) return rc;
    if (!d_jac) return OBTG_ERR_ARG;
    return true_min_dev(c, speed_row_family(c, d_tf, bound, is_max), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac,
                        d_jac_tf);
}

int obtg_speed_true_min_jac(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, int is_max, double eps_rel,
                            int max_nodes, double* out, double* t_star, int* status, double* jac, double* jac_tf)
{
    if (int rc = speed_true_min_args(c, tf, out, B, max_nodes, eps_rel)) return rc;
    if (!Y || !jac) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, speed_row_family(c, nullptr, bound, is_max), Y, tf, B, eps_rel, max_nodes, out, t_star, status, jac,
                         jac_tf);
}

// The acceleration family: the speed entry points with accel_row_family (checks: speed_true_min_args)
int obtg_accel_true_min_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, double eps_rel, int max_nodes,
                            double* d_out, double* d_t_star, int* d_status)
{
    if (int rc = speed_true_min_args(c, d_tf, d_out, B, max_nodes, eps_rel)) return rc;
    return true_min_dev(c, accel_row_family(c, d_tf, bound), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, nullptr, nullptr);
}

int obtg_accel_true_min(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, double eps_rel, int max_nodes,
                        double* out, double* t_star, int* status)
{
    if (int rc = speed_true_min_args(c, tf, out, B, max_nodes, eps_rel)) return rc;
    if (!Y) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, accel_row_family(c, nullptr, bound), Y, tf, B, eps_rel, max_nodes, out, t_star, status, nullptr, nullptr);
}

int obtg_accel_true_min_jac_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, double eps_rel, int max_nodes,
                                double* d_out, double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf)
{
    if (int rc = speed_true_min_args(c, d_tf, d_out, B, max_nodes, eps_rel)) return rc;
    if (!d_jac) return OBTG_ERR_ARG;
    return true_min_dev(c, accel_row_family(c, d_tf, bound), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac, d_jac_tf);
}

int obtg_accel_true_min_jac(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, double eps_rel, int max_nodes,
                            double* out, double* t_star, int* status, double* jac, double* jac_tf)
{
    if (int rc = speed_true_min_args(c, tf, out, B, max_nodes, eps_rel)) return rc;
    if (!Y || !jac) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, accel_row_family(c, nullptr, bound), Y, tf, B, eps_rel, max_nodes, out, t_star, status, jac, jac_tf);
}

// The jerk family: the speed entry points with jerk_row_family (checks: speed_true_min_args)
int obtg_jerk_true_min_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, double eps_rel, int max_nodes,
                            double* d_out, double* d_t_star, int* d_status)
{
    if (int rc = speed_true_min_args(c, d_tf, d_out, B, max_nodes, eps_rel)) return rc;
    return true_min_dev(c, jerk_row_family(c, d_tf, bound), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, nullptr, nullptr);
}

int obtg_jerk_true_min(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, double eps_rel, int max_nodes,
                        double* out, double* t_star, int* status)
{
    if (int rc = speed_true_min_args(c, tf, out, B, max_nodes, eps_rel)) return rc;
    if (!Y) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, jerk_row_family(c, nullptr, bound), Y, tf, B, eps_rel, max_nodes, out, t_star, status, nullptr, nullptr);
}

int obtg_jerk_true_min_jac_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double bound, double eps_rel, int max_nodes,
                                double* d_out, double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf)
{
    if (int rc = speed_true_min_args(c, d_tf, d_out, B, max_nodes, eps_rel)) return rc;
    if (!d_jac) return OBTG_ERR_ARG;
    return true_min_dev(c, jerk_row_family(c, d_tf, bound), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac, d_jac_tf);
}

int obtg_jerk_true_min_jac(obtg_ctx* c, const double* Y, const double* tf, int B, double bound, double eps_rel, int max_nodes,
                            double* out, double* t_star, int* status, double* jac, double* jac_tf)
{
    if (int rc = speed_true_min_args(c, tf, out, B, max_nodes, eps_rel)) return rc;
    if (!Y || !jac) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, jerk_row_family(c, nullptr, bound), Y, tf, B, eps_rel, max_nodes, out, t_star, status, jac, jac_tf);
}

// what obtg_ang_rate_poly, obtg_ang_rate_true_min[_jac] and their _dev twins check alike: the speed calls' checks, and the
// planar vehicle of obtg_ang_rate (the host calls: Y too; the _jac calls: jac too)
static int ang_true_min_args(const obtg_ctx* c, const double* tf, const double* out, int B, int max_nodes, double eps_rel)
{
    if (!check_ctx(c) || c->dim != 2) return OBTG_ERR_ARG;
    return speed_true_min_args(c, tf, out, B, max_nodes, eps_rel);
}

int obtg_ang_rate_poly_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double max_rate, double* d_out)
{
    if (int rc = ang_true_min_args(c, d_tf, d_out, B, 1, 0.0)) return rc;
    (void)hipSetDevice(c->device);
    const RowFamily f = ang_row_family(c, d_tf, max_rate);
    return with_batch(c, dY, B, false, [&](const double* src) { return launch_ang_rows(c, f, src, B, d_out); });
}

int obtg_ang_rate_poly(obtg_ctx* c, const double* Y, const double* tf, int B, double max_rate, double* out)
{
    if (int rc = ang_true_min_args(c, tf, out, B, 1, 0.0)) return rc;
    if (!Y) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)B * c->n_veh * 2 * (2 * c->deg + 1);
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    const double* d_tf = h.in(c->ws_in2, tf, (size_t)B, true);
    double* d_out = h.out<double>(c->ws_out, n);
    h.run([&] { return launch_ang_rows(c, ang_row_family(c, d_tf, max_rate), dY, B, d_out); });
    return h.finish(out, d_out, n);
}

int obtg_ang_rate_true_min_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double max_rate, double eps_rel,
                               int max_nodes, double* d_out, double* d_t_star, int* d_status)
{
    if (int rc = ang_true_min_args(c, d_tf, d_out, B, max_nodes, eps_rel)) return rc;
    return true_min_dev(c, ang_row_family(c, d_tf, max_rate), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, nullptr, nullptr);
}

int obtg_ang_rate_true_min(obtg_ctx* c, const double* Y, const double* tf, int B, double max_rate, double eps_rel, int max_nodes,
                           double* out, double* t_star, int* status)
{
    if (int rc = ang_true_min_args(c, tf, out, B, max_nodes, eps_rel)) return rc;
    if (!Y) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, ang_row_family(c, nullptr, max_rate), Y, tf, B, eps_rel, max_nodes, out, t_star, status, nullptr, nullptr);
}

int obtg_ang_rate_true_min_jac_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double max_rate, double eps_rel,
                                   int max_nodes, double* d_out, double* d_t_star, int* d_status, double* d_jac, double* d_jac_tf)
{
    if (int rc = ang_true_min_args(c, d_tf, d_out, B, max_nodes, eps_rel)) return rc;
    if (!d_jac) return OBTG_ERR_ARG;
    return true_min_dev(c, ang_row_family(c, d_tf, max_rate), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac, d_jac_tf);
}

int obtg_ang_rate_true_min_jac(obtg_ctx* c, const double* Y, const double* tf, int B, double max_rate, double eps_rel, int max_nodes,
                               double* out, double* t_star, int* status, double* jac, double* jac_tf)
{
    if (int rc = ang_true_min_args(c, tf, out, B, max_nodes, eps_rel)) return rc;
    if (!Y || !jac) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, ang_row_family(c, nullptr, max_rate), Y, tf, B, eps_rel, max_nodes, out, t_star, status, jac, jac_tf);
}

// The two curvature families, ROWS_CURV (dim 2) and ROWS_SCURV (dim 3): the angular-rate entry points without a time span
// (nothing takes tf), with curvature_row_family(kind).  jac_tf does not exist: the rows do not depend on the span.  One host
// path for both; `kind` picks the family.  The one difference in refusals: a planar call on a context that is not planar is
// OBTG_ERR_ARG, a space call on a context that is not in space OBTG_ERR_UNSUPPORTED.
static int curvature_args(const obtg_ctx* c, RowKind kind, const double* out, int B, int max_nodes, double eps_rel)
{
    if (!check_ctx(c) || (kind == ROWS_CURV && c->dim != 2) || !out || B < 0 || max_nodes < 1 || !(eps_rel >= 0.0)) return OBTG_ERR_ARG;
    return (kind == ROWS_SCURV && c->dim != 3) || c->deg > 31 ? OBTG_ERR_UNSUPPORTED : OBTG_OK;
}

static int curvature_poly_dev(obtg_ctx* c, RowKind kind, const double* dY, int B, double* d_out)
{
    if (int rc = curvature_args(c, kind, d_out, B, 1, 0.0)) return rc;
    (void)hipSetDevice(c->device);
    const RowFamily f = curvature_row_family(c, kind, 0.0);
    return with_batch(c, dY, B, false, [&](const double* src) { return launch_curvature_rows(c, f, src, B, d_out); });
}

static int curvature_poly(obtg_ctx* c, RowKind kind, const double* Y, int B, double* out)
{
    if (int rc = curvature_args(c, kind, out, B, 1, 0.0)) return rc;
    if (!Y) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)B * c->n_veh * curvature_shape(kind).np * (2 * c->deg + 1);
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    double* d_out = h.out<double>(c->ws_out, n);
    h.run([&] { return launch_curvature_rows(c, curvature_row_family(c, kind, 0.0), dY, B, d_out); });
    return h.finish(out, d_out, n);
}

// want_jac: the _jac entry points, where the blocks are not optional
static int curvature_true_min_dev(obtg_ctx* c, RowKind kind, const double* dY, int B, double max_curv, double eps_rel, int max_nodes,
                                  double* d_out, double* d_t_star, int* d_status, bool want_jac, double* d_jac)
{
    if (int rc = curvature_args(c, kind, d_out, B, max_nodes, eps_rel)) return rc;
    if (want_jac && !d_jac) return OBTG_ERR_ARG;
    return true_min_dev(c, curvature_row_family(c, kind, max_curv), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac, nullptr);
}

static int curvature_true_min(obtg_ctx* c, RowKind kind, const double* Y, int B, double max_curv, double eps_rel, int max_nodes,
                              double* out, double* t_star, int* status, bool want_jac, double* jac)
{
    if (int rc = curvature_args(c, kind, out, B, max_nodes, eps_rel)) return rc;
    if (!Y || (want_jac && !jac)) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, curvature_row_family(c, kind, max_curv), Y, nullptr, B, eps_rel, max_nodes, out, t_star, status, jac, nullptr);
}

// The keep-in family (ROWS_KEEP_IN): the curvature entry points' shape -- no time span, nothing takes tf, no jac_tf -- with
// keep_in_row_family, whose operand is the region obtg_ctx_set_keep_in left on the context.  Refusals, all before any launch:
// no region set or a context that is neither planar nor in space is OBTG_ERR_ARG; a degree above 31 OBTG_ERR_UNSUPPORTED.  The
// _dev calls take dY itself: the batch of an open obtg_fd_view (dY == NULL) is not built for this family, OBTG_ERR_ARG.
int obtg_ctx_set_keep_in(obtg_ctx* c, const double* H, int F, const int* VF, int P)
{
    if (!check_ctx(c) || F < 0 || P < 0) return OBTG_ERR_ARG;
    if (P > 0) {
        if ((c->dim != 2 && c->dim != 3) || F < 1 || !H || !VF) return OBTG_ERR_ARG;
        for (int k = 0; k < P; ++k)
            if (VF[2 * k] < 0 || VF[2 * k] >= c->n_veh || VF[2 * k + 1] < 0 || VF[2 * k + 1] >= F) return OBTG_ERR_ARG;
    }
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->keep_F = c->keep_P = 0;             // (set again once both tables are on the device)
    if (P == 0) return OBTG_OK;
    int rc = upload(c, c->d_keep_H, H, sizeof(double) * (size_t)F * (c->dim + 1));
    if (!rc) rc = upload(c, c->d_keep_VF, VF, sizeof(int) * 2 * (size_t)P);
    if (rc) return rc;
    c->keep_F = F; c->keep_P = P;
    return OBTG_OK;
}

int obtg_len_keep_in(const obtg_ctx* c) { return c ? c->keep_P * (c->deg + c->R + 1) : 0; }

static int keep_in_args(const obtg_ctx* c, const double* out, int B, int max_nodes, double eps_rel)
{
    if (!check_ctx(c) || c->keep_P <= 0 || (c->dim != 2 && c->dim != 3) || !out || B < 0 || max_nodes < 1 || !(eps_rel >= 0.0))
        return OBTG_ERR_ARG;
    return c->deg > 31 ? OBTG_ERR_UNSUPPORTED : OBTG_OK;
}

int obtg_keep_in_dev(obtg_ctx* c, const double* dY, int B, double* d_out)
{
    if (int rc = keep_in_args(c, d_out, B, 1, 0.0)) return rc;
    if (!dY) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return launch_keep_in_rows(c, keep_in_row_family(c), dY, B, c->R, d_out);
}

int obtg_keep_in(obtg_ctx* c, const double* Y, int B, double* out)
{
    if (int rc = keep_in_args(c, out, B, 1, 0.0)) return rc;
    if (!Y) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)obtg_len_keep_in(c) * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    double* d_out = h.out<double>(c->ws_out, n, true);
    h.run([&] { return launch_keep_in_rows(c, keep_in_row_family(c), dY, B, c->R, d_out); });
    return h.finish(out, d_out, n);
}

// want_jac: the _jac entry points, where the blocks are not optional
static int keep_in_true_min_dev(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, double* d_out, double* d_t_star,
                                int* d_status, bool want_jac, double* d_jac)
{
    if (int rc = keep_in_args(c, d_out, B, max_nodes, eps_rel)) return rc;
    if (!dY || (want_jac && !d_jac)) return OBTG_ERR_ARG;
    return true_min_dev(c, keep_in_row_family(c), dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac, nullptr);
}

static int keep_in_true_min(obtg_ctx* c, const double* Y, int B, double eps_rel, int max_nodes, double* out, double* t_star,
                            int* status, bool want_jac, double* jac)
{
    if (int rc = keep_in_args(c, out, B, max_nodes, eps_rel)) return rc;
    if (!Y || (want_jac && !jac)) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    return true_min_host(c, keep_in_row_family(c), Y, nullptr, B, eps_rel, max_nodes, out, t_star, status, jac, nullptr);
}

int obtg_keep_in_true_min_dev(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, double* d_out, double* d_t_star,
                              int* d_status)
{
    return keep_in_true_min_dev(c, dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, false, nullptr);
}

int obtg_keep_in_true_min(obtg_ctx* c, const double* Y, int B, double eps_rel, int max_nodes, double* out, double* t_star, int* status)
{
    return keep_in_true_min(c, Y, B, eps_rel, max_nodes, out, t_star, status, false, nullptr);
}

int obtg_keep_in_true_min_jac_dev(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, double* d_out, double* d_t_star,
                                  int* d_status, double* d_jac)
{
    return keep_in_true_min_dev(c, dY, B, eps_rel, max_nodes, d_out, d_t_star, d_status, true, d_jac);
}

int obtg_keep_in_true_min_jac(obtg_ctx* c, const double* Y, int B, double eps_rel, int max_nodes, double* out, double* t_star,
                              int* status, double* jac)
{
    return keep_in_true_min(c, Y, B, eps_rel, max_nodes, out, t_star, status, true, jac);
}

// The proximity family (extrema_kernels.hip ProxRows): "come close" and "stay close" rows -- items (a, b, kind) with
// (rho, tau0, tau1) of the tables obtg_ctx_set_proximity left on the context, b a vehicle or one of the family's own points.  The
// keep-in entry points' shape -- no time span, nothing takes tf, no jac_tf -- with bound and nodes beside val, t_star and
// status, so the family has a chain and a host body of its own on HostCall, laid out as true_min_chain and true_min_host are:
// the fused kernel where the shape has one (with the blocks only if true_min_jac_fused); else the values -- the fused value
// kernel, or the rows into WS_L_ROWS and their search -- and then the blocks from Y and t_star in a launch of their own.
// Refusals, all before any launch: no items set or a context that is neither planar nor in space is OBTG_ERR_ARG; a degree above
// 31 OBTG_ERR_UNSUPPORTED.  The _dev calls take dY itself (dY == NULL inside an obtg_fd_view: OBTG_ERR_ARG).
int obtg_ctx_set_proximity(obtg_ctx* c, const int* items, const double* params, const double* points, int P, int Q)
{
    if (!check_ctx(c) || P < 0 || Q < 0) return OBTG_ERR_ARG;
    if (P > 0) {
        if ((c->dim != 2 && c->dim != 3) || !items || !params || (Q > 0 && !points)) return OBTG_ERR_ARG;
        for (int k = 0; k < P; ++k) {
            const int a = items[3 * k], b = items[3 * k + 1], kind = items[3 * k + 2];
            const double rho = params[3 * k], tau0 = params[3 * k + 1], tau1 = params[3 * k + 2];
            if (a < 0 || a >= c->n_veh || b < 0 || b >= c->n_veh + Q || a == b) return OBTG_ERR_ARG;
            if (kind != OBTG_PROX_WITHIN && kind != OBTG_PROX_REACH) return OBTG_ERR_ARG;
            if (!(rho > 0.0) || !std::isfinite(rho)) return OBTG_ERR_ARG;
            if (!(0.0 <= tau0 && tau0 < tau1 && tau1 <= 1.0)) return OBTG_ERR_ARG;      // (a NaN end is refused too)
        }
    }
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->prox_P = c->prox_Q = 0;             // (set again once the tables are on the device)
    if (P == 0) return OBTG_OK;
    int rc = upload(c, c->d_prox_items, items, sizeof(int) * 3 * (size_t)P);
    if (!rc) rc = upload(c, c->d_prox_par, params, sizeof(double) * 3 * (size_t)P);
    if (!rc && Q > 0) rc = upload(c, c->d_prox_pts, points, sizeof(double) * (size_t)Q * c->dim);
    if (rc) return rc;
    c->prox_P = P; c->prox_Q = Q;
    return OBTG_OK;
}

int obtg_len_proximity(const obtg_ctx* c) { return c ? c->prox_P : 0; }

static int proximity_args(const obtg_ctx* c, const double* out, int B, int max_nodes, double eps_rel)
{
    if (!check_ctx(c) || c->prox_P <= 0 || (c->dim != 2 && c->dim != 3) || !out || B < 0 || max_nodes < 1 || !(eps_rel >= 0.0))
        return OBTG_ERR_ARG;
    return c->deg > 31 ? OBTG_ERR_UNSUPPORTED : OBTG_OK;
}

int obtg_proximity_poly_dev(obtg_ctx* c, const double* dY, int B, double* d_out)
{
    if (int rc = proximity_args(c, d_out, B, 1, 0.0)) return rc;
    if (!dY) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return launch_proximity_rows(c, dY, B, d_out);
}

int obtg_proximity_poly(obtg_ctx* c, const double* Y, int B, double* out)
{
    if (int rc = proximity_args(c, out, B, 1, 0.0)) return rc;
    if (!Y) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)B * c->prox_P * (2 * c->deg + 1);
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    double* d_out = h.out<double>(c->ws_out, n);
    h.run([&] { return launch_proximity_rows(c, dY, B, d_out); });
    return h.finish(out, d_out, n);
}

static int proximity_chain(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, ProxOut o, double* d_jac)
{
    int rc = OBTG_ERR_UNSUPPORTED;
    if (!d_jac || c->true_min_jac_fused) rc = launch_proximity_true(c, dY, B, eps_rel, max_nodes, o, d_jac);
    if (rc != OBTG_ERR_UNSUPPORTED) return rc;
    const size_t n = (size_t)B * c->prox_P;
    if (d_jac) {
        if (!o.t) {
            DevBuf& wt = c->ws_misc[WS_L_TSTAR];
            if ((rc = wt.reserve(sizeof(double) * n))) return rc;
            o.t = wt.as<double>();
        }
        rc = launch_proximity_true(c, dY, B, eps_rel, max_nodes, o, nullptr);
    }
    if (rc == OBTG_ERR_UNSUPPORTED) {
        DevBuf& ws = c->ws_misc[WS_L_ROWS];
        if ((rc = ws.reserve(sizeof(double) * n * (2 * c->deg + 1)))) return rc;
        if ((rc = launch_proximity_rows(c, dY, B, ws.as<double>()))) return rc;
        rc = launch_proximity_search(c, ws.as<double>(), B, eps_rel, max_nodes, o);
    }
    if (rc || !d_jac) return rc;
    return launch_proximity_envelope(c, dY, B, o.t, d_jac);
}

// want_jac: the _jac entry points, where the blocks are not optional
static int proximity_true_dev(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, const ProxOut& o, bool want_jac,
                              double* d_jac)
{
    if (int rc = proximity_args(c, o.val, B, max_nodes, eps_rel)) return rc;
    if (!dY || (want_jac && !d_jac)) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return proximity_chain(c, dY, B, eps_rel, max_nodes, o, d_jac);
}

// the host body: Y up, val | t_star | bound | jac in ws_out, nodes | status in WS_STATUS
static int proximity_true_host(obtg_ctx* c, const double* Y, int B, double eps_rel, int max_nodes, const ProxOut& o, bool want_jac,
                               double* jac)
{
    if (int rc = proximity_args(c, o.val, B, max_nodes, eps_rel)) return rc;
    if (!Y || (want_jac && !jac)) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = (size_t)B * c->prox_P, nj = jac ? n * c->dim * (c->deg + 1) : 0;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    double* dv = h.out<double>(c->ws_out, 3 * n + nj);
    int* di = h.out<int>(c->ws_misc[WS_STATUS], 2 * n);
    double* dj = jac ? dv + 3 * n : nullptr;
    h.run([&] { return proximity_chain(c, dY, B, eps_rel, max_nodes, ProxOut{ dv, dv + n, dv + 2 * n, di, di + n }, dj); });
    h.fetch(o.t, dv + n, n);
    h.fetch(o.bound, dv + 2 * n, n);
    h.fetch(o.nodes, di, n);
    h.fetch(o.status, di + n, n);
    h.fetch(jac, dj, nj);
    return h.finish(o.val, dv, n);
}

int obtg_proximity_true_dev(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, double* d_val, double* d_t_star,
                            double* d_bound, int* d_nodes, int* d_status)
{
    return proximity_true_dev(c, dY, B, eps_rel, max_nodes, ProxOut{ d_val, d_t_star, d_bound, d_nodes, d_status }, false, nullptr);
}

int obtg_proximity_true(obtg_ctx* c, const double* Y, int B, double eps_rel, int max_nodes, double* val, double* t_star, double* bound,
                        int* nodes, int* status)
{
    return proximity_true_host(c, Y, B, eps_rel, max_nodes, ProxOut{ val, t_star, bound, nodes, status }, false, nullptr);
}

int obtg_proximity_true_jac_dev(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, double* d_val, double* d_t_star,
                                double* d_bound, int* d_nodes, int* d_status, double* d_jac)
{
    return proximity_true_dev(c, dY, B, eps_rel, max_nodes, ProxOut{ d_val, d_t_star, d_bound, d_nodes, d_status }, true, d_jac);
}

int obtg_proximity_true_jac(obtg_ctx* c, const double* Y, int B, double eps_rel, int max_nodes, double* val, double* t_star,
                            double* bound, int* nodes, int* status, double* jac)
{
    return proximity_true_host(c, Y, B, eps_rel, max_nodes, ProxOut{ val, t_star, bound, nodes, status }, true, jac);
}

// The keep-out rows (keepout_kernels.hip): items are (vehicle, obstacle) pairs of the tables obtg_ctx_set_keep_out left on the
// context; an obstacle is a run of faces of H.  The search is a kernel of its own (a minimum over t of a maximum over faces),
// not a RowFamily: there is no polynomial row to write.  Refusals as keep-in's, all before any launch; more than 16 faces in an
// obstacle or a degree above 31 is OBTG_ERR_UNSUPPORTED.  The _dev calls take dY itself (dY == NULL: OBTG_ERR_ARG).
constexpr int kKeepOutMaxFaces = 16;

int obtg_ctx_set_keep_out(obtg_ctx* c, const double* H, const int* obs_off, int O, const int* VO, int P)
{
    if (!check_ctx(c) || O < 0 || P < 0) return OBTG_ERR_ARG;
    int F = 0;
    if (P > 0) {
        if ((c->dim != 2 && c->dim != 3) || O < 1 || !H || !obs_off || !VO || obs_off[0] != 0) return OBTG_ERR_ARG;
        for (int o = 0; o < O; ++o)
            if (obs_off[o + 1] <= obs_off[o]) return OBTG_ERR_ARG;           // (an empty obstacle, offsets that do not ascend)
        for (int k = 0; k < P; ++k)
            if (VO[2 * k] < 0 || VO[2 * k] >= c->n_veh || VO[2 * k + 1] < 0 || VO[2 * k + 1] >= O) return OBTG_ERR_ARG;
        for (int o = 0; o < O; ++o)
            if (obs_off[o + 1] - obs_off[o] > kKeepOutMaxFaces) return OBTG_ERR_UNSUPPORTED;
        F = obs_off[O];
    }
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->ko_F = c->ko_O = c->ko_P = 0;       // (set again once the tables are on the device)
    c->ko_motion = false;                  // new tables: every obstacle stands still until obtg_ctx_set_keep_out_motion says otherwise
    c->ko_eu_state = 0;
    if (P == 0) return OBTG_OK;
    int rc = upload(c, c->d_ko_H, H, sizeof(double) * (size_t)F * (c->dim + 1));
    if (!rc) rc = upload(c, c->d_ko_off, obs_off, sizeof(int) * ((size_t)O + 1));
    if (!rc) rc = upload(c, c->d_ko_VO, VO, sizeof(int) * 2 * (size_t)P);
    if (rc) return rc;
    c->ko_F = F; c->ko_O = O; c->ko_P = P;
    c->h_ko_H.assign(H, H + (size_t)F * (c->dim + 1));       // (for the Euclidean calls' tables, made on their first use)
    c->h_ko_off.assign(obs_off, obs_off + O + 1);
    return OBTG_OK;
}

int obtg_len_keep_out(const obtg_ctx* c) { return c ? c->ko_P : 0; }

// The Euclidean metric (include/obtg.h "Euclidean keep-out clearance"; csrc/keepout_features.h): the signed Euclidean distance in
// place of the largest face value.  The normalised faces and the feature records are host work, done once per table.
int obtg_keep_out_features(const double* H, int F, int d, double* Hn, int* idx, double* ginv, int* n)
{
    if (!H || !Hn || !idx || !ginv || !n || F < 1 || (d != 2 && d != 3)) return OBTG_ERR_ARG;
    if (F > kKoFeatMaxFaces) return OBTG_ERR_UNSUPPORTED;
    keep_out_normalise(H, F, d, Hn);
    *n = keep_out_enumerate(Hn, F, d, kKoMaxFeatures, idx, ginv);
    return *n > kKoMaxFeatures ? OBTG_ERR_UNSUPPORTED : OBTG_OK;
}

// the device records of one obstacle behind `rec`: Gram^-1 (6) | the faces a byte each, 0xff for none
static void keep_out_pack_features(const int* idx, const double* ginv, int n, std::vector<double>& rec)
{
    for (int k = 0; k < n; ++k) {
        for (int e = 0; e < 6; ++e) rec.push_back(ginv[6 * k + e]);
        const long long pk = (long long)(idx[3 * k] & 0xff) | ((long long)(idx[3 * k + 1] & 0xff) << 8) | ((long long)(idx[3 * k + 2] & 0xff) << 16);
        double slot;
        std::memcpy(&slot, &pk, sizeof slot);
        rec.push_back(slot);
    }
}

// Moving keep-out obstacles (include/obtg.h "moving keep-out obstacles"): obstacle o's faces are translated by a Bezier offset
// on [0, T_o]; the search runs on the relative curve, formed per item in the kernel's prologue (tf differs per batch row).
// The motion lives beside the keep-out tables and goes when they are set again.
int obtg_ctx_set_keep_out_motion(obtg_ctx* c, const double* Q, const int* q_off, const double* T, int O)
{
    if (!check_ctx(c) || O < 0) return OBTG_ERR_ARG;
    if (O > 0) {
        if (c->ko_P <= 0 || O != c->ko_O || !q_off || !T || q_off[0] != 0) return OBTG_ERR_ARG;
        for (int o = 0; o < O; ++o) {
            if (q_off[o + 1] < q_off[o]) return OBTG_ERR_ARG;
            if (q_off[o + 1] > q_off[o] && !(T[o] > 0.0 && std::isfinite(T[o]))) return OBTG_ERR_ARG;
        }
        if (q_off[O] > 0 && !Q) return OBTG_ERR_ARG;
        for (int o = 0; o < O; ++o)
            if (q_off[o + 1] - q_off[o] > c->deg + 1) return OBTG_ERR_UNSUPPORTED;
    }
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->ko_motion = false;
    if (O == 0) return OBTG_OK;
    const size_t nq = (size_t)q_off[O] * c->dim;
    const double none = 0.0;
    int rc = upload(c, c->d_ko_Q, nq ? Q : &none, sizeof(double) * (nq ? nq : 1));
    if (!rc) rc = upload(c, c->d_ko_qoff, q_off, sizeof(int) * ((size_t)O + 1));
    if (!rc) rc = upload(c, c->d_ko_T, T, sizeof(double) * (size_t)O);
    if (rc) return rc;
    c->ko_motion = true;
    return OBTG_OK;
}

// Vehicle pairs against ONE separation region (include/obtg.h "polytopic vehicle-to-vehicle separation"): the keep-out kernel on
// D = Y_i - Y_j, the pairs i < j in lexicographic order from a table made here.  The region is a state of its own: the obstacle
// tables and their motion neither read nor write it.
int obtg_ctx_set_pair_keep_out(obtg_ctx* c, const double* H, int F)
{
    if (!check_ctx(c) || F < 0) return OBTG_ERR_ARG;
    if (F > 0) {
        if ((c->dim != 2 && c->dim != 3) || !H) return OBTG_ERR_ARG;
        if (F > kKeepOutMaxFaces) return OBTG_ERR_UNSUPPORTED;
        for (int f = 0; f < F; ++f)
            if (H[(size_t)f * (c->dim + 1) + c->dim] <= 0.0) return OBTG_ERR_ARG;        // (the origin is strictly inside; a NaN passes)
    }
    (void)hipSetDevice(c->device);
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    c->pk_F = c->pk_NF = c->pk_eu_state = 0;
    if (F == 0) return OBTG_OK;
    const int N = c->n_veh;
    std::vector<int> ij;
    for (int i = 0; i < N; ++i)
        for (int j = i + 1; j < N; ++j) { ij.push_back(i); ij.push_back(j); }
    if (ij.empty()) ij.assign(2, 0);               // (one vehicle: no pair, the table is never read)
    int rc = upload(c, c->d_pk_H, H, sizeof(double) * (size_t)F * (c->dim + 1));
    if (!rc) rc = upload(c, c->d_pk_IJ, ij.data(), sizeof(int) * ij.size());
    if (rc) return rc;
    c->h_pk_H.assign(H, H + (size_t)F * (c->dim + 1));
    c->pk_F = F;
    return OBTG_OK;
}

int obtg_len_pair_keep_out(const obtg_ctx* c) { return c && c->pk_F > 0 ? c->n_veh * (c->n_veh - 1) / 2 : 0; }

// ------------------------------------------------------------------ the keep-out family's one host path
// A form is a set of these bits; KO_FREE: the free-curve calls (obtg_bern_keep_out*), whose only outputs are val, t and status
enum : unsigned { KO_MOVING = 1, KO_EUCLID = 2, KO_PAIR = 4, KO_FREE = 8 };

// The output columns of a keep-out call, in the order of the workspace -- the doubles in ws_out, the ints in WS_STATUS -- and
// of the downloads: the per-item doubles, the ints, then the blocks, the order every keep-out call has downloaded in since
// it was added.  val is first and is downloaded last (finish, the call's ONE synchronise).  The partition of the workspace and
// the list of downloads both come from walking this table; a new output is a new line here and a member of KeepOutOutputs.
constexpr int kKoPerDim = -1, kKoPerBlock = -2;       // elements per item: dim, dim K
struct KoColumn {
    double* KeepOutOutputs::*d;     // a column of doubles, or
    int* KeepOutOutputs::*i;        // a column of ints
    int per_item;                   // 1, 2, 3, kKoPerDim or kKoPerBlock
    unsigned only, never;           // the forms that have it: one bit of `only` set (0: any form) and no bit of `never`
    bool on_request;                // true: on the device only when the caller asked for it (a null pointer: the kernel skips the
                                    // stores); false: always given device storage, whatever the caller's pointer is
};
static const KoColumn kKoColumns[] = {
    { &KeepOutOutputs::val, nullptr, 1, 0, 0, false },
    { &KeepOutOutputs::t, nullptr, 1, 0, 0, false },
    { &KeepOutOutputs::lam, nullptr, 1, 0, KO_EUCLID | KO_FREE, false },
    { &KeepOutOutputs::dir, nullptr, kKoPerDim, KO_EUCLID, KO_FREE, false },
    { &KeepOutOutputs::bound, nullptr, 1, 0, KO_FREE, false },
    { &KeepOutOutputs::jac_tf, nullptr, 1, KO_MOVING, KO_FREE, true },
    { nullptr, &KeepOutOutputs::face, 2, 0, KO_EUCLID | KO_FREE, false },
    { nullptr, &KeepOutOutputs::faces3, 3, KO_EUCLID, KO_FREE, false },
    { nullptr, &KeepOutOutputs::nodes, 1, 0, KO_FREE, false },
    { nullptr, &KeepOutOutputs::status, 1, 0, 0, false },
    { &KeepOutOutputs::rel, nullptr, kKoPerBlock, KO_MOVING | KO_PAIR, KO_FREE, true },
    { &KeepOutOutputs::jac, nullptr, kKoPerBlock, 0, KO_FREE, true },
};

// elements per item of a column in this call; 0: the call has no such column on the device (the on-request columns are doubles)
static size_t ko_per_item(const KoColumn& col, unsigned form, int dim, int K, const KeepOutOutputs& host)
{
    if ((col.only && !(form & col.only)) || (form & col.never) || (col.on_request && !(host.*col.d))) return 0;
    return col.per_item == kKoPerDim ? dim : col.per_item == kKoPerBlock ? dim * K : col.per_item;
}

// the device side of a call of n items: the workspace reserved and handed out column by column
static KeepOutOutputs keep_out_device_outputs(HostCall& h, unsigned form, int dim, int K, size_t n, const KeepOutOutputs& host)
{
    size_t nd = 0, ni = 0;
    for (const KoColumn& col : kKoColumns) (col.d ? nd : ni) += n * ko_per_item(col, form, dim, K, host);
    double* dv = h.out<double>(h.c->ws_out, nd);
    int* di = h.out<int>(h.c->ws_misc[WS_STATUS], ni);
    KeepOutOutputs dev{};
    for (const KoColumn& col : kKoColumns) {
        const size_t k = n * ko_per_item(col, form, dim, K, host);
        if (!k) continue;
        if (col.d) { dev.*col.d = dv; dv += k; }
        else { dev.*col.i = di; di += k; }
    }
    return dev;
}

// one download per optional output the caller gave a pointer for, then val
static int keep_out_download(HostCall& h, unsigned form, int dim, int K, size_t n, const KeepOutOutputs& host, const KeepOutOutputs& dev)
{
    for (const KoColumn& col : kKoColumns) {
        const size_t k = n * ko_per_item(col, form, dim, K, host);
        if (!k || col.d == &KeepOutOutputs::val) continue;
        if (col.d) h.fetch(host.*col.d, dev.*col.d, k);
        else h.fetch(host.*col.i, dev.*col.i, k);
    }
    return h.finish(host.val, dev.val, n);
}

// The Euclidean tables of the face ranges off[0 .. O] of H: the normalised faces and, range by range, the feature records
// (normalise, enumerate, pack), then the upload -- Hn to d_Hn, the records to d_feat (null: behind Hn, in the same buffer), the
// ranges' record offsets to d_foff (null: not kept); *nf: the records of the last range.  A range with more than
// kKoMaxFeatures records: OBTG_ERR_UNSUPPORTED, nothing uploaded.
static int keep_out_feature_tables(obtg_ctx* c, const double* H, const int* off, int O, int d, DevBuf& d_Hn, DevBuf* d_feat, DevBuf* d_foff,
                                   int* nf)
{
    std::vector<double> Hn((size_t)off[O] * (d + 1)), rec, ginv(6 * (size_t)kKoMaxFeatures);
    std::vector<int> foff(O + 1, 0), idx(3 * (size_t)kKoMaxFeatures);
    for (int o = 0; o < O; ++o) {
        const size_t at = (size_t)off[o] * (d + 1);
        const int F = off[o + 1] - off[o];
        keep_out_normalise(H + at, F, d, Hn.data() + at);
        const int n = keep_out_enumerate(Hn.data() + at, F, d, kKoMaxFeatures, idx.data(), ginv.data());
        if (n > kKoMaxFeatures) return OBTG_ERR_UNSUPPORTED;
        keep_out_pack_features(idx.data(), ginv.data(), n, rec);
        foff[o + 1] = foff[o] + n;
    }
    (void)hipSetDevice(c->device);
    if (!d_feat) Hn.insert(Hn.end(), rec.begin(), rec.end());
    else if (rec.empty()) rec.push_back(0.0);      // (no range has a feature: the buffer is never read)
    int rc = upload(c, d_Hn, Hn.data(), sizeof(double) * Hn.size());
    if (!rc && d_feat) rc = upload(c, *d_feat, rec.data(), sizeof(double) * rec.size());
    if (!rc && d_foff) rc = upload(c, *d_foff, foff.data(), sizeof(int) * foff.size());
    if (!rc && nf) *nf = foff[O] - foff[O - 1];
    return rc;
}

// the context's Euclidean tables -- the obstacles', or with `pair` the region's -- made on the first Euclidean call after the
// tables were set; a refusal is remembered (ko_eu_state / pk_eu_state) and answered again
static int keep_out_euclid_tables(obtg_ctx* c, bool pair)
{
    int& state = pair ? c->pk_eu_state : c->ko_eu_state;
    if (state) return state == 1 ? OBTG_OK : state;
    const int region[2] = {0, c->pk_F};
    const int rc = pair ? keep_out_feature_tables(c, c->h_pk_H.data(), region, 1, c->dim, c->d_pk_Hn, &c->d_pk_feat, nullptr, &c->pk_NF)
                        : keep_out_feature_tables(c, c->h_ko_H.data(), c->h_ko_off.data(), c->ko_O, c->dim, c->d_ko_Hn, &c->d_ko_feat,
                                                  &c->d_ko_foff, nullptr);
    if (rc == OBTG_OK) state = 1;
    else if (rc == OBTG_ERR_UNSUPPORTED) state = rc;
    return rc;
}

// What an entry point of the context forms passes beside its outputs.  tf: the moving forms'; want_jac: the _jac entry points,
// where the blocks (and the moving forms' jac_tf) are not optional
struct KoCall {
    unsigned form;
    bool want_jac;
    const double* Y;
    const double* tf;
    int B;
    double margin, eps_rel;
    int max_nodes;
};

static KoCall ko_call(unsigned form, bool want_jac, const double* Y, const double* tf, int B, double margin, double eps_rel, int max_nodes)
{
    KoCall k{};
    k.form = form; k.want_jac = want_jac; k.Y = Y; k.tf = tf; k.B = B; k.margin = margin; k.eps_rel = eps_rel; k.max_nodes = max_nodes;
    return k;
}

// The refusals of the context forms, in the order a caller can observe; all before any launch
static int keep_out_args(obtg_ctx* c, const KoCall& k, const KeepOutOutputs& o)
{
    const bool pair = k.form & KO_PAIR;
    if (!check_ctx(c) || (pair ? c->pk_F : c->ko_P) <= 0 || (c->dim != 2 && c->dim != 3) || !o.val || k.B < 0 || k.max_nodes < 1 ||
        !(k.eps_rel >= 0.0) || k.margin != k.margin)
        return OBTG_ERR_ARG;
    if (c->deg > 31) return OBTG_ERR_UNSUPPORTED;
    if (k.form == KO_EUCLID && c->ko_motion) return OBTG_ERR_UNSUPPORTED;       // moving obstacles under this metric are not built
    if (k.form & KO_EUCLID)
        if (int rc = keep_out_euclid_tables(c, pair)) return rc;
    // (a moving call on a context without a motion is a caller who forgot to set one, not a request for the static rows)
    if ((k.form & KO_MOVING) && (!c->ko_motion || !k.tf || (k.want_jac && !o.jac_tf))) return OBTG_ERR_ARG;
    return !k.Y || (k.want_jac && !o.jac) ? OBTG_ERR_ARG : OBTG_OK;
}

// the launch of a context form: the context's tables by name
static int keep_out_launch(obtg_ctx* c, const KoCall& k, const double* dY, const double* d_tf, const KeepOutOutputs& dev)
{
    KeepOutLaunch a{};
    a.dim = c->dim; a.K = c->deg + 1; a.n_veh = c->n_veh;
    a.moving = k.form & KO_MOVING; a.euclid = k.form & KO_EUCLID; a.pair = k.form & KO_PAIR;
    a.Y = dY; a.margin = k.margin; a.eps_rel = k.eps_rel; a.max_nodes = k.max_nodes; a.out = dev;
    if (a.pair) {
        a.P = obtg_len_pair_keep_out(c); a.F_all = c->pk_F;
        a.H = (a.euclid ? c->d_pk_Hn : c->d_pk_H).as<double>(); a.VO_or_IJ = c->d_pk_IJ.as<int>();
        if (a.euclid) { a.feat = c->d_pk_feat.as<double>(); a.NF_all = c->pk_NF; }
    } else {
        a.P = c->ko_P;
        a.H = (a.euclid ? c->d_ko_Hn : c->d_ko_H).as<double>(); a.off = c->d_ko_off.as<int>(); a.VO_or_IJ = c->d_ko_VO.as<int>();
        if (a.euclid) { a.feat = c->d_ko_feat.as<double>(); a.feat_off = c->d_ko_foff.as<int>(); }
        if (a.moving) { a.Q = c->d_ko_Q.as<double>(); a.q_off = c->d_ko_qoff.as<int>(); a.T = c->d_ko_T.as<double>(); a.tf = d_tf; }
    }
    a.M = (long)k.B * a.P;
    return launch_keep_out(c, a);
}

// the _dev body: Y, tf and the outputs are the caller's device memory (an empty call is the launcher's OBTG_OK)
static int keep_out_dev(obtg_ctx* c, const KoCall& k, const KeepOutOutputs& o)
{
    if (int rc = keep_out_args(c, k, o)) return rc;
    (void)hipSetDevice(c->device);
    return keep_out_launch(c, k, k.Y, k.tf, o);
}

// the host body: Y (and tf) up zero-copy, the columns of the table in the workspace, one download per output asked for
static int keep_out_host(obtg_ctx* c, const KoCall& k, const KeepOutOutputs& o)
{
    if (int rc = keep_out_args(c, k, o)) return rc;
    const size_t n = (size_t)k.B * ((k.form & KO_PAIR) ? obtg_len_pair_keep_out(c) : c->ko_P);
    if (n == 0) return OBTG_OK;                // (B == 0, or a pair call on a context of one vehicle)
    HostCall h(c);
    const double* dY = h.in(c->ws_in, k.Y, ysize(c) * k.B, true);
    const double* d_tf = (k.form & KO_MOVING) ? h.in(c->ws_in2, k.tf, (size_t)k.B, true) : nullptr;
    const KeepOutOutputs dev = keep_out_device_outputs(h, k.form, c->dim, c->deg + 1, n, o);
    h.run([&] { return keep_out_launch(c, k, dY, d_tf, dev); });
    return keep_out_download(h, k.form, c->dim, c->deg + 1, n, o, dev);
}

// Free curves cv[M][dim][K] against ONE face table H[F][dim+1] (a host array in both forms), whatever the context's shape is:
// the same kernel, one obstacle of all F faces, margin 0; KO_EUCLID: under the Euclidean metric (Hn | the records in one buffer);
// KO_MOVING: the obstacle moves by Q[dim][Km] (a host array in both forms), r[M] per curve the part [0, r] of the motion's
// parameter that the curve spans (null: 1; device memory in the _dev forms).  The context's own keep-out tables are not touched:
// the tables of the call go to WS_ARG_A and WS_ARG_B.  dev: cv, r and the outputs are device memory.
static int bern_keep_out(obtg_ctx* c, unsigned form, bool dev, const double* cv, int M, int dim, int K, const double* H, int F,
                         const double* Q, int Km, const double* r, double eps_rel, int max_nodes, double* val, double* t_star, int* status)
{
    if (!check_ctx(c) || M < 0 || (dim != 2 && dim != 3) || K < 2 || F < 1 || !H || max_nodes < 1 || !(eps_rel >= 0.0)) return OBTG_ERR_ARG;
    if (K > kMdMaxCurveK || F > kKeepOutMaxFaces) return OBTG_ERR_UNSUPPORTED;
    if (M > 0 && !(cv && val)) return OBTG_ERR_ARG;
    if (form & KO_MOVING) {                    // (a bad motion is refused in an empty call too)
        if (Km < 1 || !Q) return OBTG_ERR_ARG;
        if (Km > K) return OBTG_ERR_UNSUPPORTED;
    }
    if (M == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    DevBuf &dH = c->ws_misc[WS_ARG_A], &dQ = c->ws_misc[WS_ARG_B];
    const int faces[2] = {0, F};
    KeepOutLaunch a{};
    a.dim = dim; a.K = K; a.M = M; a.n_veh = a.P = 1; a.F_all = F; a.moving = form & KO_MOVING; a.euclid = form & KO_EUCLID;
    a.eps_rel = eps_rel; a.max_nodes = max_nodes;
    if (int rc = a.euclid ? keep_out_feature_tables(c, H, faces, 1, dim, dH, nullptr, nullptr, &a.NF_all)
                          : upload(c, dH, H, sizeof(double) * (size_t)F * (dim + 1)))
        return rc;
    a.H = dH.as<double>();
    if (a.euclid) a.feat = a.H + (size_t)F * (dim + 1);
    if (a.moving) {
        if (int rc = upload(c, dQ, Q, sizeof(double) * (size_t)Km * dim)) return rc;
        a.Q = dQ.as<double>(); a.Km = Km;
    }
    KeepOutOutputs o{};
    o.val = val; o.t = t_star; o.status = status;
    if (dev) {
        a.Y = cv; a.r = r; a.out = o;
        return launch_keep_out(c, a);
    }
    const size_t n = (size_t)M;
    HostCall h(c);
    a.Y = h.in(c->ws_in, cv, n * dim * K);
    a.r = r ? h.in(c->ws_in2, r, n) : nullptr;
    a.out = keep_out_device_outputs(h, form | KO_FREE, dim, K, n, o);
    h.run([&] { return launch_keep_out(c, a); });
    return keep_out_download(h, form | KO_FREE, dim, K, n, o, a.out);
}

// The entry points: each names its form and passes its pointers.  include/obtg.h has two orders of the outputs, the faces
// metric's (face, lam) and the Euclidean metric's (faces, dir); rel, jac and jac_tf follow where the entry point has them.
static KeepOutOutputs ko_out(double* val, double* t, int* face, double* lam, double* bound, int* nodes, int* status, double* rel = nullptr,
                             double* jac = nullptr, double* jac_tf = nullptr)
{
    KeepOutOutputs o{};
    o.val = val; o.t = t; o.face = face; o.lam = lam; o.bound = bound; o.nodes = nodes; o.status = status;
    o.rel = rel; o.jac = jac; o.jac_tf = jac_tf;
    return o;
}

static KeepOutOutputs ko_out_euclid(double* val, double* t, int* faces3, double* dir, double* bound, int* nodes, int* status,
                                    double* rel = nullptr, double* jac = nullptr)
{
    KeepOutOutputs o{};
    o.val = val; o.t = t; o.faces3 = faces3; o.dir = dir; o.bound = bound; o.nodes = nodes; o.status = status;
    o.rel = rel; o.jac = jac;
    return o;
}

int obtg_keep_out_true_min_dev(obtg_ctx* c, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                               double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes, int* d_status)
{
    return keep_out_dev(c, ko_call(0, false, dY, nullptr, B, margin, eps_rel, max_nodes),
                        ko_out(d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status));
}

int obtg_keep_out_true_min(obtg_ctx* c, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out, double* t_star,
                           int* face, double* lam, double* bound, int* nodes, int* status)
{
    return keep_out_host(c, ko_call(0, false, Y, nullptr, B, margin, eps_rel, max_nodes),
                         ko_out(out, t_star, face, lam, bound, nodes, status));
}

int obtg_keep_out_true_min_jac_dev(obtg_ctx* c, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                                   double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes, int* d_status,
                                   double* d_jac)
{
    return keep_out_dev(c, ko_call(0, true, dY, nullptr, B, margin, eps_rel, max_nodes),
                        ko_out(d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, nullptr, d_jac));
}

int obtg_keep_out_true_min_jac(obtg_ctx* c, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                               double* t_star, int* face, double* lam, double* bound, int* nodes, int* status, double* jac)
{
    return keep_out_host(c, ko_call(0, true, Y, nullptr, B, margin, eps_rel, max_nodes),
                         ko_out(out, t_star, face, lam, bound, nodes, status, nullptr, jac));
}

int obtg_keep_out_euclid_true_min_dev(obtg_ctx* c, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                                      double* d_t_star, int* d_faces, double* d_dir, double* d_bound, int* d_nodes, int* d_status)
{
    return keep_out_dev(c, ko_call(KO_EUCLID, false, dY, nullptr, B, margin, eps_rel, max_nodes),
                        ko_out_euclid(d_out, d_t_star, d_faces, d_dir, d_bound, d_nodes, d_status));
}

int obtg_keep_out_euclid_true_min(obtg_ctx* c, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                  double* t_star, int* faces, double* dir, double* bound, int* nodes, int* status)
{
    return keep_out_host(c, ko_call(KO_EUCLID, false, Y, nullptr, B, margin, eps_rel, max_nodes),
                         ko_out_euclid(out, t_star, faces, dir, bound, nodes, status));
}

int obtg_keep_out_euclid_true_min_jac_dev(obtg_ctx* c, const double* dY, int B, double margin, double eps_rel, int max_nodes,
                                          double* d_out, double* d_t_star, int* d_faces, double* d_dir, double* d_bound, int* d_nodes,
                                          int* d_status, double* d_jac)
{
    return keep_out_dev(c, ko_call(KO_EUCLID, true, dY, nullptr, B, margin, eps_rel, max_nodes),
                        ko_out_euclid(d_out, d_t_star, d_faces, d_dir, d_bound, d_nodes, d_status, nullptr, d_jac));
}

int obtg_keep_out_euclid_true_min_jac(obtg_ctx* c, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                      double* t_star, int* faces, double* dir, double* bound, int* nodes, int* status, double* jac)
{
    return keep_out_host(c, ko_call(KO_EUCLID, true, Y, nullptr, B, margin, eps_rel, max_nodes),
                         ko_out_euclid(out, t_star, faces, dir, bound, nodes, status, nullptr, jac));
}

int obtg_keep_out_moving_true_min_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double margin, double eps_rel, int max_nodes,
                                      double* d_out, double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes,
                                      int* d_status, double* d_rel)
{
    return keep_out_dev(c, ko_call(KO_MOVING, false, dY, d_tf, B, margin, eps_rel, max_nodes),
                        ko_out(d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, d_rel));
}

int obtg_keep_out_moving_true_min(obtg_ctx* c, const double* Y, const double* tf, int B, double margin, double eps_rel, int max_nodes,
                                  double* out, double* t_star, int* face, double* lam, double* bound, int* nodes, int* status, double* rel)
{
    return keep_out_host(c, ko_call(KO_MOVING, false, Y, tf, B, margin, eps_rel, max_nodes),
                         ko_out(out, t_star, face, lam, bound, nodes, status, rel));
}

int obtg_keep_out_moving_true_min_jac_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double margin, double eps_rel,
                                          int max_nodes, double* d_out, double* d_t_star, int* d_face, double* d_lam, double* d_bound,
                                          int* d_nodes, int* d_status, double* d_rel, double* d_jac, double* d_jac_tf)
{
    return keep_out_dev(c, ko_call(KO_MOVING, true, dY, d_tf, B, margin, eps_rel, max_nodes),
                        ko_out(d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, d_rel, d_jac, d_jac_tf));
}

int obtg_keep_out_moving_true_min_jac(obtg_ctx* c, const double* Y, const double* tf, int B, double margin, double eps_rel, int max_nodes,
                                      double* out, double* t_star, int* face, double* lam, double* bound, int* nodes, int* status,
                                      double* rel, double* jac, double* jac_tf)
{
    return keep_out_host(c, ko_call(KO_MOVING, true, Y, tf, B, margin, eps_rel, max_nodes),
                         ko_out(out, t_star, face, lam, bound, nodes, status, rel, jac, jac_tf));
}

int obtg_pair_keep_out_true_min_dev(obtg_ctx* c, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                                    double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes, int* d_status,
                                    double* d_rel)
{
    return keep_out_dev(c, ko_call(KO_PAIR, false, dY, nullptr, B, margin, eps_rel, max_nodes),
                        ko_out(d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, d_rel));
}

int obtg_pair_keep_out_true_min(obtg_ctx* c, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                double* t_star, int* face, double* lam, double* bound, int* nodes, int* status, double* rel)
{
    return keep_out_host(c, ko_call(KO_PAIR, false, Y, nullptr, B, margin, eps_rel, max_nodes),
                         ko_out(out, t_star, face, lam, bound, nodes, status, rel));
}

int obtg_pair_keep_out_true_min_jac_dev(obtg_ctx* c, const double* dY, int B, double margin, double eps_rel, int max_nodes, double* d_out,
                                        double* d_t_star, int* d_face, double* d_lam, double* d_bound, int* d_nodes, int* d_status,
                                        double* d_rel, double* d_jac)
{
    return keep_out_dev(c, ko_call(KO_PAIR, true, dY, nullptr, B, margin, eps_rel, max_nodes),
                        ko_out(d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, d_rel, d_jac));
}

int obtg_pair_keep_out_true_min_jac(obtg_ctx* c, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                    double* t_star, int* face, double* lam, double* bound, int* nodes, int* status, double* rel,
                                    double* jac)
{
    return keep_out_host(c, ko_call(KO_PAIR, true, Y, nullptr, B, margin, eps_rel, max_nodes),
                         ko_out(out, t_star, face, lam, bound, nodes, status, rel, jac));
}

int obtg_pair_keep_out_euclid_true_min_dev(obtg_ctx* c, const double* dY, int B, double margin, double eps_rel, int max_nodes,
                                           double* d_out, double* d_t_star, int* d_faces, double* d_dir, double* d_bound, int* d_nodes,
                                           int* d_status, double* d_rel)
{
    return keep_out_dev(c, ko_call(KO_PAIR | KO_EUCLID, false, dY, nullptr, B, margin, eps_rel, max_nodes),
                        ko_out_euclid(d_out, d_t_star, d_faces, d_dir, d_bound, d_nodes, d_status, d_rel));
}

int obtg_pair_keep_out_euclid_true_min(obtg_ctx* c, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                       double* t_star, int* faces, double* dir, double* bound, int* nodes, int* status, double* rel)
{
    return keep_out_host(c, ko_call(KO_PAIR | KO_EUCLID, false, Y, nullptr, B, margin, eps_rel, max_nodes),
                         ko_out_euclid(out, t_star, faces, dir, bound, nodes, status, rel));
}

int obtg_pair_keep_out_euclid_true_min_jac_dev(obtg_ctx* c, const double* dY, int B, double margin, double eps_rel, int max_nodes,
                                               double* d_out, double* d_t_star, int* d_faces, double* d_dir, double* d_bound,
                                               int* d_nodes, int* d_status, double* d_rel, double* d_jac)
{
    return keep_out_dev(c, ko_call(KO_PAIR | KO_EUCLID, true, dY, nullptr, B, margin, eps_rel, max_nodes),
                        ko_out_euclid(d_out, d_t_star, d_faces, d_dir, d_bound, d_nodes, d_status, d_rel, d_jac));
}

int obtg_pair_keep_out_euclid_true_min_jac(obtg_ctx* c, const double* Y, int B, double margin, double eps_rel, int max_nodes, double* out,
                                           double* t_star, int* faces, double* dir, double* bound, int* nodes, int* status, double* rel,
                                           double* jac)
{
    return keep_out_host(c, ko_call(KO_PAIR | KO_EUCLID, true, Y, nullptr, B, margin, eps_rel, max_nodes),
                         ko_out_euclid(out, t_star, faces, dir, bound, nodes, status, rel, jac));
}

int obtg_bern_keep_out_dev(obtg_ctx* c, const double* d_c, int M, int dim, int K, const double* H, int F, double eps_rel, int max_nodes,
                           double* d_val, double* d_t_star, int* d_status)
{
    return bern_keep_out(c, 0, true, d_c, M, dim, K, H, F, nullptr, 0, nullptr, eps_rel, max_nodes, d_val, d_t_star, d_status);
}

int obtg_bern_keep_out(obtg_ctx* c, const double* cv, int M, int dim, int K, const double* H, int F, double eps_rel, int max_nodes,
                       double* val, double* t_star, int* status)
{
    return bern_keep_out(c, 0, false, cv, M, dim, K, H, F, nullptr, 0, nullptr, eps_rel, max_nodes, val, t_star, status);
}

int obtg_bern_keep_out_euclid_dev(obtg_ctx* c, const double* d_c, int M, int dim, int K, const double* H, int F, double eps_rel,
                                  int max_nodes, double* d_val, double* d_t_star, int* d_status)
{
    return bern_keep_out(c, KO_EUCLID, true, d_c, M, dim, K, H, F, nullptr, 0, nullptr, eps_rel, max_nodes, d_val, d_t_star, d_status);
}

int obtg_bern_keep_out_euclid(obtg_ctx* c, const double* cv, int M, int dim, int K, const double* H, int F, double eps_rel, int max_nodes,
                              double* val, double* t_star, int* status)
{
    return bern_keep_out(c, KO_EUCLID, false, cv, M, dim, K, H, F, nullptr, 0, nullptr, eps_rel, max_nodes, val, t_star, status);
}

int obtg_bern_keep_out_moving_dev(obtg_ctx* c, const double* d_c, int M, int dim, int K, const double* H, int F, const double* Q, int Km,
                                  const double* d_r, double eps_rel, int max_nodes, double* d_val, double* d_t_star, int* d_status)
{
    return bern_keep_out(c, KO_MOVING, true, d_c, M, dim, K, H, F, Q, Km, d_r, eps_rel, max_nodes, d_val, d_t_star, d_status);
}

int obtg_bern_keep_out_moving(obtg_ctx* c, const double* cv, int M, int dim, int K, const double* H, int F, const double* Q, int Km,
                              const double* r, double eps_rel, int max_nodes, double* val, double* t_star, int* status)
{
    return bern_keep_out(c, KO_MOVING, false, cv, M, dim, K, H, F, Q, Km, r, eps_rel, max_nodes, val, t_star, status);
}

// Free curves c[M][dim][K], any K from 2 to 32 whatever the context's shape is: the family's rows kernel and workspace search
// on them (max_curv = 0; planar: no clamp, both extrema; space: the maximum itself).  The context's shape does not enter, so
// this is not a RowFamily (which describes rows of the context's vehicles); the launchers are the family's.  The product table
// of degree K - 1 is kept from call to call and serves both families.
static int curvature_table(obtg_ctx* c, int n, const double** d_tab)
{
    if (c->curv_tab_n != n) {
        c->curv_tab_n = -1;
        auto t = ang_rows_table(n);
        if (int rc = upload(c, c->d_curv_tab, t.data(), t.size() * sizeof(double))) return rc;
        c->curv_tab_n = n;
    }
    *d_tab = c->d_curv_tab.as<double>();
    return OBTG_OK;
}

// k_min and t_min: the planar family's second side; null in space
static int bern_curvature_args(const obtg_ctx* c, RowKind kind, int M, int K, double eps_rel, int max_nodes, const double* coef,
                               const double* k_max, const double* t_max, const double* k_min, const double* t_min)
{
    if (!check_ctx(c) || M < 0 || K < 2 || max_nodes < 1 || !(eps_rel >= 0.0)) return OBTG_ERR_ARG;
    if (!curvature_supported(K)) return OBTG_ERR_UNSUPPORTED;
    if (M > 0 && (!coef || !k_max || !t_max || (kind == ROWS_CURV && (!k_min || !t_min)))) return OBTG_ERR_ARG;
    return OBTG_OK;
}

// rows into WS_L_ROWS, then the search: both launches timed under OBTG_K_ANG_RATE
static int bern_curvature_chain(obtg_ctx* c, RowKind kind, const double* d_c, int M, int K, double eps_rel, int max_nodes,
                                double* d_k_max, double* d_t_max, double* d_k_min, double* d_t_min, int* d_status)
{
    const CurvShape s = curvature_shape(kind);
    const double* d_tab = nullptr;
    int rc = curvature_table(c, K - 1, &d_tab);
    if (rc) return rc;
    DevBuf& ws = c->ws_misc[WS_L_ROWS];
    if ((rc = ws.reserve(sizeof(double) * (size_t)M * s.np * (2 * K - 1)))) return rc;
    if ((rc = launch_curv_rows(c, kind, d_c, d_tab, M, K, ws.as<double>(), OBTG_K_ANG_RATE))) return rc;
    return launch_curv_search(c, kind, ws.as<double>(), (long)s.sides * M, K, 0.0, 1, eps_rel, max_nodes, d_k_max, d_t_max, d_k_min, d_t_min,
                              d_status, OBTG_K_ANG_RATE);
}

static int bern_curvature_dev(obtg_ctx* c, RowKind kind, const double* d_c, int M, int K, double eps_rel, int max_nodes,
                              double* d_k_max, double* d_t_max, double* d_k_min, double* d_t_min, int* d_status)
{
    if (int rc = bern_curvature_args(c, kind, M, K, eps_rel, max_nodes, d_c, d_k_max, d_t_max, d_k_min, d_t_min)) return rc;
    if (M == 0) return OBTG_OK;
    (void)hipSetDevice(c->device);
    return bern_curvature_chain(c, kind, d_c, M, K, eps_rel, max_nodes, d_k_max, d_t_max, d_k_min, d_t_min, d_status);
}

static int bern_curvature(obtg_ctx* c, RowKind kind, const double* coef, int M, int K, double eps_rel, int max_nodes, double* k_max,
                          double* t_max, double* k_min, double* t_min, int* status)
{
    if (int rc = bern_curvature_args(c, kind, M, K, eps_rel, max_nodes, coef, k_max, t_max, k_min, t_min)) return rc;
    if (M == 0) return OBTG_OK;
    const CurvShape s = curvature_shape(kind);
    const size_t m = (size_t)M;
    const bool sides = s.sides == 2;
    HostCall h(c);
    const double* d_c = h.in(c->ws_in, coef, m * s.dim * K);
    double* dv = h.out<double>(c->ws_out, 2 * s.sides * m);          // k_max | t_max [| k_min | t_min]
    int* ds = h.out<int>(c->ws_misc[WS_STATUS], s.sides * m);
    h.run([&] {
        return bern_curvature_chain(c, kind, d_c, M, K, eps_rel, max_nodes, dv, dv + m, sides ? dv + 2 * m : nullptr, sides ? dv + 3 * m : nullptr, ds);
    });
    h.fetch(t_max, dv + m, m);
    if (sides) {
        h.fetch(k_min, dv + 2 * m, m);
        h.fetch(t_min, dv + 3 * m, m);
    }
    h.fetch(status, ds, s.sides * m);
    return h.finish(k_max, dv, m);
}

int obtg_curvature_poly_dev(obtg_ctx* c, const double* dY, int B, double* d_out) { return curvature_poly_dev(c, ROWS_CURV, dY, B, d_out); }
int obtg_curvature_poly(obtg_ctx* c, const double* Y, int B, double* out) { return curvature_poly(c, ROWS_CURV, Y, B, out); }
int obtg_curvature_true_min_dev(obtg_ctx* c, const double* dY, int B, double max_curv, double eps_rel, int max_nodes, double* d_out,
                                double* d_t_star, int* d_status)
{
    return curvature_true_min_dev(c, ROWS_CURV, dY, B, max_curv, eps_rel, max_nodes, d_out, d_t_star, d_status, false, nullptr);
}
int obtg_curvature_true_min(obtg_ctx* c, const double* Y, int B, double max_curv, double eps_rel, int max_nodes, double* out,
                            double* t_star, int* status)
{
    return curvature_true_min(c, ROWS_CURV, Y, B, max_curv, eps_rel, max_nodes, out, t_star, status, false, nullptr);
}
int obtg_curvature_true_min_jac_dev(obtg_ctx* c, const double* dY, int B, double max_curv, double eps_rel, int max_nodes,
                                    double* d_out, double* d_t_star, int* d_status, double* d_jac)
{
    return curvature_true_min_dev(c, ROWS_CURV, dY, B, max_curv, eps_rel, max_nodes, d_out, d_t_star, d_status, true, d_jac);
}
int obtg_curvature_true_min_jac(obtg_ctx* c, const double* Y, int B, double max_curv, double eps_rel, int max_nodes, double* out,
                                double* t_star, int* status, double* jac)
{
    return curvature_true_min(c, ROWS_CURV, Y, B, max_curv, eps_rel, max_nodes, out, t_star, status, true, jac);
}
int obtg_bern_curvature_dev(obtg_ctx* c, const double* d_c, int M, int K, double eps_rel, int max_nodes, double* d_k_min,
                            double* d_t_min, double* d_k_max, double* d_t_max, int* d_status)
{
    return bern_curvature_dev(c, ROWS_CURV, d_c, M, K, eps_rel, max_nodes, d_k_max, d_t_max, d_k_min, d_t_min, d_status);
}
int obtg_bern_curvature(obtg_ctx* c, const double* coef, int M, int K, double eps_rel, int max_nodes, double* k_min, double* t_min,
                        double* k_max, double* t_max, int* status)
{
    return bern_curvature(c, ROWS_CURV, coef, M, K, eps_rel, max_nodes, k_max, t_max, k_min, t_min, status);
}

int obtg_space_curvature_poly_dev(obtg_ctx* c, const double* dY, int B, double* d_out) { return curvature_poly_dev(c, ROWS_SCURV, dY, B, d_out); }
int obtg_space_curvature_poly(obtg_ctx* c, const double* Y, int B, double* out) { return curvature_poly(c, ROWS_SCURV, Y, B, out); }
int obtg_space_curvature_true_min_dev(obtg_ctx* c, const double* dY, int B, double max_curv, double eps_rel, int max_nodes,
                                      double* d_out, double* d_t_star, int* d_status)
{
    return curvature_true_min_dev(c, ROWS_SCURV, dY, B, max_curv, eps_rel, max_nodes, d_out, d_t_star, d_status, false, nullptr);
}
int obtg_space_curvature_true_min(obtg_ctx* c, const double* Y, int B, double max_curv, double eps_rel, int max_nodes, double* out,
                                  double* t_star, int* status)
{
    return curvature_true_min(c, ROWS_SCURV, Y, B, max_curv, eps_rel, max_nodes, out, t_star, status, false, nullptr);
}
int obtg_space_curvature_true_min_jac_dev(obtg_ctx* c, const double* dY, int B, double max_curv, double eps_rel, int max_nodes,
                                          double* d_out, double* d_t_star, int* d_status, double* d_jac)
{
    return curvature_true_min_dev(c, ROWS_SCURV, dY, B, max_curv, eps_rel, max_nodes, d_out, d_t_star, d_status, true, d_jac);
}
int obtg_space_curvature_true_min_jac(obtg_ctx* c, const double* Y, int B, double max_curv, double eps_rel, int max_nodes, double* out,
                                      double* t_star, int* status, double* jac)
{
    return curvature_true_min(c, ROWS_SCURV, Y, B, max_curv, eps_rel, max_nodes, out, t_star, status, true, jac);
}
int obtg_bern_space_curvature_dev(obtg_ctx* c, const double* d_c, int M, int K, double eps_rel, int max_nodes, double* d_k_max,
                                  double* d_t_max, int* d_status)
{
    return bern_curvature_dev(c, ROWS_SCURV, d_c, M, K, eps_rel, max_nodes, d_k_max, d_t_max, nullptr, nullptr, d_status);
}
int obtg_bern_space_curvature(obtg_ctx* c, const double* coef, int M, int K, double eps_rel, int max_nodes, double* k_max,
                              double* t_max, int* status)
{
    return bern_curvature(c, ROWS_SCURV, coef, M, K, eps_rel, max_nodes, k_max, t_max, nullptr, nullptr, status);
}

// ------------------------------------------------------------------ single-curve algebra
int obtg_bern_elev(obtg_ctx* c, const double* in, int rows, int n, int R, double* out)
{
    if (!check_ctx(c) || !in || !out || rows < 0 || n < 0 || R < 0) return OBTG_ERR_ARG;
    if (rows == 0) return OBTG_OK;
    const size_t len = (size_t)rows * (n + R + 1);
    HostCall h(c);
    const double* d_in = h.in(c->ws_in, in, (size_t)rows * (n + 1));
    double* d_out = h.out<double>(c->ws_out, len);
    h.run([&] { return launch_bern_elev(c, d_in, rows, n, R, d_out); });
    return h.finish(out, d_out, len);
}

int obtg_bern_diff(obtg_ctx* c, const double* in, int rows, int n, double T, double* out)
{
    if (!check_ctx(c) || !in || !out || rows < 0 || n < 1) return OBTG_ERR_ARG;
    if (rows == 0) return OBTG_OK;
    const size_t len = (size_t)rows * (n + 1);
    HostCall h(c);
    const double* d_in = h.in(c->ws_in, in, len);
    double* d_out = h.out<double>(c->ws_out, len);
    h.run([&] { return launch_bern_diff(c, d_in, rows, n, T, d_out); });
    return h.finish(out, d_out, len);
}

int obtg_bern_split(obtg_ctx* c, const double* in, int rows, int n, double z, double* left, double* right)
{
    if (!check_ctx(c) || !in || !left || !right || rows < 0 || n < 0) return OBTG_ERR_ARG;
    if (rows == 0) return OBTG_OK;
    const size_t len = (size_t)rows * (n + 1);
    HostCall h(c);
    const double* d_in = h.in(c->ws_in, in, len);
    double* dl = h.out<double>(c->ws_out, 2 * len);         // left | right
    h.run([&] { return launch_bern_split(c, d_in, rows, n, z, dl, dl + len); });
    h.fetch(left, dl, len);
    return h.finish(right, dl + len, len);
}

int obtg_bern_restrict(obtg_ctx* c, const double* in, int rows, int n, const double* span, const double* target, double* out)
{
    if (!check_ctx(c) || !in || !span || !target || !out || rows < 0 || n < 0) return OBTG_ERR_ARG;
    for (int r = 0; r < rows; ++r)
        if (!(span[2 * r] <= target[2 * r] && target[2 * r] < target[2 * r + 1] && target[2 * r + 1] <= span[2 * r + 1])) return OBTG_ERR_ARG;
    if (rows == 0) return OBTG_OK;
    const size_t len = (size_t)rows * (n + 1);
    HostCall h(c);
    const double* d_in = h.in(c->ws_in, in, len);
    const double* d_span = h.in(c->ws_misc[WS_ARG_A], span, 2 * (size_t)rows);
    const double* d_target = h.in(c->ws_misc[WS_ARG_B], target, 2 * (size_t)rows);
    double* d_out = h.out<double>(c->ws_out, len);
    h.run([&] { return launch_bern_restrict(c, d_in, rows, n, d_span, d_target, d_out); });
    return h.finish(out, d_out, len);
}

int obtg_bern_eval(obtg_ctx* c, const double* cpts, int rows, int n, const double* tau, int n_tau, double t0, double tf, double* out)
{
    if (!check_ctx(c) || !cpts || !tau || !out || rows < 0 || n < 0 || n_tau < 0) return OBTG_ERR_ARG;
    if (rows == 0 || n_tau == 0) return OBTG_OK;
    const size_t len = (size_t)rows * n_tau;
    HostCall h(c);
    const double* d_cpts = h.in(c->ws_in, cpts, (size_t)rows * (n + 1));
    const double* d_tau = h.in(c->ws_in2, tau, (size_t)n_tau);
    double* d_out = h.out<double>(c->ws_out, len);
    h.run([&] { return launch_bern_eval(c, d_cpts, rows, n, d_tau, n_tau, t0, tf, d_out); });
    return h.finish(out, d_out, len);
}

int obtg_bern_mul(obtg_ctx* c, const double* a, const double* b, int rows, int m, int n, double* out)
{
    if (!check_ctx(c) || !a || !b || !out || rows < 0 || m < 0 || n < 0) return OBTG_ERR_ARG;
    if (rows == 0) return OBTG_OK;
    const size_t len = (size_t)rows * (m + n + 1);
    HostCall h(c);
    const double* d_a = h.in(c->ws_in, a, (size_t)rows * (m + 1));
    const double* d_b = h.in(c->ws_in2, b, (size_t)rows * (n + 1));
    double* d_out = h.out<double>(c->ws_out, len);
    h.run([&] { return launch_bern_mul(c, d_a, d_b, rows, m, n, d_out); });
    return h.finish(out, d_out, len);
}

int obtg_bern_normsq(obtg_ctx* c, const double* x, int d, int n, double* out)
{
    if (!check_ctx(c) || !x || !out || d < 1 || n < 0) return OBTG_ERR_ARG;
    const size_t len = (size_t)(2 * n + 1);
    HostCall h(c);
    const double* d_x = h.in(c->ws_in, x, (size_t)d * (n + 1));
    double* d_out = h.out<double>(c->ws_out, len);
    h.run([&] { return launch_bern_normsq(c, d_x, d, n, d_out); });
    return h.finish(out, d_out, len);
}

// ------------------------------------------------------------------ objectives
int obtg_euclidean_obj(obtg_ctx* c, const double* Y, int B, double* out)
{
    if (!check_ctx(c) || !Y || !out || B < 0) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    double* d_out = h.out<double>(c->ws_out, (size_t)B, true);
    h.run([&] { return launch_euclidean_obj(c, dY, B, d_out); });
    return h.finish(out, d_out, (size_t)B);
}

static int host_deriv_obj(obtg_ctx* c, const double* Y, const double* tf, int B, int order, double* out)
{
    if (!check_ctx(c) || !Y || !tf || !out || B < 0) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    // one final time for the whole batch, as the reference's objectives have (optimization.py:294-308)
    for (int b = 1; b < B; ++b) if (!(tf[b] == tf[0])) return OBTG_ERR_ARG;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    const double* d_tf = h.in(c->ws_in2, tf, (size_t)B, true);
    double* d_out = h.out<double>(c->ws_out, (size_t)B, true);
    h.run([&] { return launch_deriv_energy_obj(c, dY, d_tf, tf[0], B, order, d_out); });
    return h.finish(out, d_out, (size_t)B);
}

int obtg_accel_obj(obtg_ctx* c, const double* Y, const double* tf, int B, double* out) { return host_deriv_obj(c, Y, tf, B, 2, out); }
int obtg_jerk_obj(obtg_ctx* c, const double* Y, const double* tf, int B, double* out) { return host_deriv_obj(c, Y, tf, B, 3, out); }

// ------------------------------------------------------------------ true arc length (arclen_kernels.hip)
// obtg_bern_arc_length starts as a copy of obtg_bern_extrema (optional outputs, status required in the host form, M == 0 is
// OBTG_OK with null pointers, nothing zero copy); obtg_arc_length_obj as a copy of obtg_euclidean_obj (Y and out zero copy)
// with the optional status and gradient of the _jac calls (not zero copy).
static int arc_length_args(const obtg_ctx* c, const double* coef, int M, int d, int K, double eps_rel, int max_nodes,
                           const double* len, bool need_status, const int* status)
{
    if (!check_ctx(c) || M < 0 || d < 1 || d > 3 || K < 2 || max_nodes < 1 || !(eps_rel >= 0.0)) return OBTG_ERR_ARG;
    if (!arc_length_supported(d, K)) return OBTG_ERR_UNSUPPORTED;
    if (M > 0 && (!coef || !len || (need_status && !status))) return OBTG_ERR_ARG;
    return OBTG_OK;
}

int obtg_bern_arc_length_dev(obtg_ctx* c, const double* d_c, int M, int d, int K, double eps_rel, int max_nodes, double* d_len,
                             double* d_err, int* d_nodes, int* d_status, double* d_grad)
{
    if (int rc = arc_length_args(c, d_c, M, d, K, eps_rel, max_nodes, d_len, false, d_status)) return rc;
    (void)hipSetDevice(c->device);
    return launch_arc_length(c, d_c, M, d, K, eps_rel, max_nodes, d_len, d_err, d_nodes, d_status, d_grad);
}

int obtg_bern_arc_length(obtg_ctx* c, const double* coef, int M, int d, int K, double eps_rel, int max_nodes, double* len,
                         double* err, int* nodes, int* status, double* grad)
{
    if (int rc = arc_length_args(c, coef, M, d, K, eps_rel, max_nodes, len, true, status)) return rc;
    if (M == 0) return OBTG_OK;
    const size_t m = (size_t)M, ng = grad ? m * d * K : 0;
    HostCall h(c);
    const double* d_c = h.in(c->ws_in, coef, m * d * K);
    double* dv = h.out<double>(c->ws_out, 2 * m + ng);      // len | err | grad
    int* dn = h.out<int>(c->ws_misc[WS_INFO], 2 * m);       // nodes | status
    h.run([&] { return launch_arc_length(c, d_c, M, d, K, eps_rel, max_nodes, dv, dv + m, dn, dn + m, grad ? dv + 2 * m : nullptr); });
    h.fetch(err, dv + m, m);
    h.fetch(nodes, dn, m);
    h.fetch(status, dn + m, m);
    h.fetch(grad, dv + 2 * m, ng);
    return h.finish(len, dv, m);
}

static int arc_length_obj_args(const obtg_ctx* c, const double* Y, int B, double eps_rel, int max_nodes, const double* out)
{
    if (!check_ctx(c) || !Y || !out || B < 0 || max_nodes < 1 || !(eps_rel >= 0.0)) return OBTG_ERR_ARG;
    if (!arc_length_supported(c->dim, c->deg + 1)) return OBTG_ERR_UNSUPPORTED;
    return OBTG_OK;
}

int obtg_arc_length_obj_dev(obtg_ctx* c, const double* dY, int B, double eps_rel, int max_nodes, double* d_out, int* d_status,
                            double* d_grad)
{
    if (int rc = arc_length_obj_args(c, dY, B, eps_rel, max_nodes, d_out)) return rc;
    (void)hipSetDevice(c->device);
    return launch_arc_length_obj(c, dY, B, eps_rel, max_nodes, d_out, d_status, d_grad);
}

int obtg_arc_length_obj(obtg_ctx* c, const double* Y, int B, double eps_rel, int max_nodes, double* out, int* status, double* grad)
{
    if (int rc = arc_length_obj_args(c, Y, B, eps_rel, max_nodes, out)) return rc;
    if (B == 0) return OBTG_OK;
    const size_t ng = grad ? ysize(c) * B : 0;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B, true);
    double* d_out = h.out<double>(c->ws_out, (size_t)B + ng, !grad);      // out | grad
    double* d_grad = grad ? d_out + B : nullptr;
    int* d_st = h.out<int>(c->ws_misc[WS_STATUS], (size_t)B);
    h.run([&] { return launch_arc_length_obj(c, dY, B, eps_rel, max_nodes, d_out, d_st, d_grad); });
    h.fetch(status, d_st, (size_t)B);
    h.fetch(grad, d_grad, ng);
    return h.finish(out, d_out, (size_t)B);
}

// ------------------------------------------------------------------ exact derivatives (jac_kernels.hip)
int obtg_temporal_sep_jac_dev(obtg_ctx* c, const double* dY, int B, double* d_out)
{
    if (!check_ctx(c) || B < 0) return OBTG_ERR_ARG;
    if (B == 0 || c->n_pairs == 0) return OBTG_OK;
    if (!dY || !d_out) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return launch_temporal_sep_jac(c, dY, B, d_out);
}

int obtg_temporal_sep_jac(obtg_ctx* c, const double* Y, int B, double* out)
{
    if (!check_ctx(c) || !Y || !out || B < 0) return OBTG_ERR_ARG;
    if (B == 0 || c->n_pairs == 0) return OBTG_OK;
    const size_t n = (size_t)c->n_pairs * (2 * c->deg + c->R + 1) * c->dim * (c->deg + 1) * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B);
    double* d_out = h.out<double>(c->ws_out, n);
    h.run([&] { return launch_temporal_sep_jac(c, dY, B, d_out); });
    return h.finish(out, d_out, n);
}

int obtg_speed_jac_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, int is_max, double* d_out, double* d_out_tf)
{
    if (!check_ctx(c) || B < 0) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    if (!dY || !d_tf || !d_out) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return launch_speed_jac(c, dY, d_tf, B, is_max, d_out, d_out_tf);
}

// the host entry points with a d/dtf output: Y, tf in; out[B][per] and (nullable) out_tf[B][per_tf] back.
// launch(dY, d_tf, d_out, d_out_tf), d_out_tf null with out_tf
extern "C++" {
template <class Launch>
static int host_jac_tf(obtg_ctx* c, const double* Y, const double* tf, int B, size_t per, size_t per_tf, double* out, double* out_tf,
                       Launch launch)
{
    if (!Y || !tf || !out || B < 0) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, ysize(c) * B);
    const double* d_tf = h.in(c->ws_in2, tf, (size_t)B);
    double* d_out = h.out<double>(c->ws_out, per * B);
    double* d_out_tf = out_tf ? h.out<double>(c->ws_misc[WS_OUT_TF], per_tf * B) : nullptr;
    h.run([&] { return launch(dY, d_tf, d_out, d_out_tf); });
    h.fetch(out_tf, d_out_tf, per_tf * B);
    return h.finish(out, d_out, per * B);
}
}  // extern "C++"

// the per-vehicle families: [B][N][rows][d][n+1] and [B][N][rows]
int obtg_speed_jac(obtg_ctx* c, const double* Y, const double* tf, int B, int is_max, double* out, double* out_tf)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    const size_t per_tf = (size_t)c->n_veh * (2 * c->deg + c->R + 1);
    return host_jac_tf(c, Y, tf, B, per_tf * c->dim * (c->deg + 1), per_tf, out, out_tf,
                       [&](const double* dY, const double* d_tf, double* d_out, double* d_out_tf) {
                           return launch_speed_jac(c, dY, d_tf, B, is_max, d_out, d_out_tf); });
}

int obtg_ang_rate_jac_dev(obtg_ctx* c, const double* dY, const double* d_tf, int B, double* d_out, double* d_out_tf)
{
    if (!check_ctx(c) || B < 0 || c->dim != 2) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    if (!dY || !d_tf || !d_out) return OBTG_ERR_ARG;
    (void)hipSetDevice(c->device);
    return launch_ang_rate_jac(c, dY, d_tf, B, d_out, d_out_tf);
}

int obtg_ang_rate_jac(obtg_ctx* c, const double* Y, const double* tf, int B, double* out, double* out_tf)
{
    if (!check_ctx(c) || c->dim != 2) return OBTG_ERR_ARG;
    const size_t per_tf = (size_t)c->n_veh * (4 * (c->deg + c->R) + 1);
    return host_jac_tf(c, Y, tf, B, per_tf * c->dim * (c->deg + 1), per_tf, out, out_tf,
                       [&](const double* dY, const double* d_tf, double* d_out, double* d_out_tf) {
                           return launch_ang_rate_jac(c, dY, d_tf, B, d_out, d_out_tf); });
}

int obtg_euclidean_grad(obtg_ctx* c, const double* Y, int B, double* out)
{
    if (!check_ctx(c) || !Y || !out || B < 0) return OBTG_ERR_ARG;
    if (B == 0) return OBTG_OK;
    const size_t n = ysize(c) * B;
    HostCall h(c);
    const double* dY = h.in(c->ws_in, Y, n);
    double* d_out = h.out<double>(c->ws_out, n);
    h.run([&] { return launch_euclidean_grad(c, dY, B, d_out); });
    return h.finish(out, d_out, n);
}

int obtg_deriv_energy_grad(obtg_ctx* c, const double* Y, const double* tf, int B, int order, double* out, double* out_tf)
{
    if (!check_ctx(c) || order < 1 || order > 4) return OBTG_ERR_ARG;
    return host_jac_tf(c, Y, tf, B, ysize(c), 1, out, out_tf, [&](const double* dY, const double* d_tf, double* d_out, double* d_out_tf) {
        return launch_deriv_energy_grad(c, dY, d_tf, B, order, d_out, d_out_tf); });
}

// ------------------------------------------------------------------ instrumentation
int obtg_set_profiling(obtg_ctx* c, int on)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    if ((on & OBTG_PROFILE_ONLY_FLAG) && (on & 0xff) >= OBTG_K_END) return OBTG_ERR_ARG;
    OBTG_HIP(c, hipStreamSynchronize(c->stream));
    flush_pending_events(c);
    c->profiling = on != 0;
    c->profile_mask = (on & OBTG_PROFILE_ONLY_FLAG) ? (1u << (on & 0xff)) : ~0u;
    return OBTG_OK;
}

int obtg_set_profile_period(obtg_ctx* c, int every)
{
    if (!check_ctx(c) || every < 1) return OBTG_ERR_ARG;
    c->profile_period = every;
    for (auto& n : c->profile_seen) n = 0;
    return OBTG_OK;
}

int obtg_kernel_stats(obtg_ctx* c, int kernel_id, double* total_ms, long long* launches)
{
    if (!check_ctx(c) || kernel_id < 0 || kernel_id >= OBTG_K_END) return OBTG_ERR_ARG;
    flush_pending_events(c);
    if (total_ms) *total_ms = c->stats[kernel_id].ms;
    if (launches) *launches = c->stats[kernel_id].launches;
    return OBTG_OK;
}

int obtg_reset_kernel_stats(obtg_ctx* c)
{
    if (!check_ctx(c)) return OBTG_ERR_ARG;
    flush_pending_events(c);
    for (auto& s : c->stats) s = KernelStat{};
    return OBTG_OK;
}

const char* obtg_kernel_name(int id)
{
    switch (id) {
        case OBTG_K_TEMPORAL_SEP: return "temporal_sep";
        case OBTG_K_SPEED: return "speed";
        case OBTG_K_ANG_RATE: return "ang_rate";
        case OBTG_K_GJK: return "gjk";
        case OBTG_K_MIN_DIST: return "min_dist";
        case OBTG_K_FD_BATCH: return "fd_batch";
        case OBTG_K_BERN: return "bern";
        case OBTG_K_PAIR_SWEEP: return "pair_sweep";
        case OBTG_K_JAC: return "jac";
        case OBTG_K_ARC_LENGTH: return "arc_length";
        default: return "?";
    }
}

}  // extern "C"
