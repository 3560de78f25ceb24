// icp4r_reve.cpp — C ABI of the 3D Doppler ego-velocity estimator (include/icp4r/icp4r_reve.h): the
// kernel of icp4r_reve.hip, then the gate's compaction (icp4r_gate.hip) on the same stream.  No CPU
// fallback: every device entry fails with ICP4R_E_HIP if the device path cannot run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "icp4r/icp4r_reve.h"
#include "icp4r_host.hpp"
#include "icp4r_internal.hpp"
#include "icp4r_reve.hpp"
#include "icp4r_reve_math.hpp"

using icp4r::GateArgs;
using icp4r::ReveArgs;
using icp4r_host::fail;

namespace {

constexpr int32_t kMaxScans = 65535;  // grid.y of the gate's per-scan launches

int check_shape(int32_t nscans, int32_t max_n) {
    if (nscans < 0 || max_n < 0) return fail(ICP4R_E_INVALID, "nscans = %d, max_n = %d", nscans, max_n);
    if (nscans > kMaxScans) return fail(ICP4R_E_TOO_LARGE, "%d scans in one batch (at most %d)", nscans, kMaxScans);
    if (max_n > ICP4R_REVE_MAX_POINTS)
        return fail(ICP4R_E_TOO_LARGE, "max_n = %d (at most %d)", max_n, ICP4R_REVE_MAX_POINTS);
    return ICP4R_OK;
}

// Validates the settings and fills the kernel's copy of them.
int fill_args(const icp4r_reve_params* params, ReveArgs& a) {
    icp4r_reve_params p;
    icp4r_reve_params_default(&p);
    if (params) p = *params;
    if (p.N_ransac_points != 3) return fail(ICP4R_E_INVALID, "N_ransac_points = %d (must be 3)", p.N_ransac_points);
    if (!p.use_ransac) return fail(ICP4R_E_INVALID, "use_ransac = false is not built");
    if (!(p.allowed_outlier_percentage >= 0.0 && p.allowed_outlier_percentage <= 1.0))
        return fail(ICP4R_E_INVALID, "allowed_outlier_percentage outside [0, 1]");
    const double all[] = {p.min_dist, p.max_dist, p.min_db, p.elevation_thresh_deg, p.azimuth_thresh_deg, p.filter_min_z,
                          p.filter_max_z, p.doppler_velocity_correction_factor, p.thresh_zero_velocity,
                          p.sigma_zero_velocity_x, p.sigma_zero_velocity_y, p.sigma_zero_velocity_z, p.sigma_offset_radar_x,
                          p.sigma_offset_radar_y, p.sigma_offset_radar_z, p.max_sigma_x, p.max_sigma_y, p.max_sigma_z,
                          p.max_r_cond, p.inlier_thresh};
    for (double v : all)
        if (v != v) return fail(ICP4R_E_INVALID, "a setting is NaN");
    const int32_t it = icp4r_reve::ransac_iterations(p.success_prob, p.outlier_prob);
    if (it < 0) return fail(ICP4R_E_INVALID, "success_prob / outlier_prob give no hypothesis count");
    if (it > ICP4R_REVE_MAX_ITERATIONS)
        return fail(ICP4R_E_TOO_LARGE, "%d hypotheses (at most %d)", it, ICP4R_REVE_MAX_ITERATIONS);
    memset(&a, 0, sizeof(a));
    a.iterations = it;
    a.use_z = p.use_z_filter == 1;
    a.seed = p.seed;
    a.min_dist = p.min_dist;
    a.max_dist = p.max_dist;
    a.min_db = p.min_db;
    a.az_lim = p.azimuth_thresh_deg * (M_PI / 180.0);
    a.el_lim = p.elevation_thresh_deg * (M_PI / 180.0);
    a.zmin = p.filter_min_z;
    a.zmax = p.filter_max_z;
    a.factor = p.doppler_velocity_correction_factor;
    a.zero_thresh = p.thresh_zero_velocity;
    a.keep = 1.0 - p.allowed_outlier_percentage;
    a.sig_zero[0] = p.sigma_zero_velocity_x;
    a.sig_zero[1] = p.sigma_zero_velocity_y;
    a.sig_zero[2] = p.sigma_zero_velocity_z;
    a.sig_off[0] = p.sigma_offset_radar_x;
    a.sig_off[1] = p.sigma_offset_radar_y;
    a.sig_off[2] = p.sigma_offset_radar_z;
    a.sig_max[0] = p.max_sigma_x;
    a.sig_max[1] = p.max_sigma_y;
    a.sig_max[2] = p.max_sigma_z;
    a.max_cond = p.max_r_cond;
    a.inlier_thresh = p.inlier_thresh;
    return ICP4R_OK;
}

// The estimator over device-resident scans; xyzi / bad: the packing's copy and guard flags, or null.
int run_reve(icp4r_ctx* ctx, ReveArgs& a, const float* records, const int64_t* off, const int32_t* cnt, int32_t nscans,
             int32_t max_n, icp4r_reve_result* results, uint8_t* mask, float4* xyzi, const int32_t* bad, hipStream_t st) {
    a.rec = records;
    a.off = off;
    a.cnt = cnt;
    a.bad = bad;
    a.max_n = max_n;
    a.lds_pts = std::min<int32_t>(max_n, icp4r::kReveLdsPts);
    a.spill_stride = max_n - a.lds_pts;
    a.spill = nullptr;
    if (a.spill_stride > 0) {  // the points past the LDS copy (the sine estimator's feature workspace)
        HIP_TRY(ctx->ego_feat.ensure((size_t)nscans * (size_t)a.spill_stride * sizeof(float4)));
        a.spill = static_cast<float4*>(ctx->ego_feat.p);
    }
    a.xyzi = xyzi;
    a.mask = mask;
    a.results = results;
    HIP_TRY(icp4r::launch_reve(a, nscans, st));
    return ICP4R_OK;
}

// The estimator, then the gate over its mask, for scans that lie within the first `cap` records.
int run_clouds(icp4r_ctx* ctx, ReveArgs& a, const float* records, const int64_t* off, const int32_t* cnt, int32_t nscans,
               int32_t max_n, int64_t cap, icp4r_reve_result* results, uint8_t* mask, float4* clouds, int64_t* pair_off,
               int32_t* pair_n, hipStream_t st) {
    if (cap < 1) cap = 1;
    HIP_TRY(ctx->ego_xyzi.ensure((size_t)cap * sizeof(float4)));
    HIP_TRY(ctx->gate_cnt.ensure((size_t)nscans * sizeof(int32_t)));
    HIP_TRY(ctx->gate_bad.ensure((size_t)nscans * sizeof(int32_t)));
    if (!mask) {
        HIP_TRY(ctx->gate_mask.ensure((size_t)cap));
        mask = static_cast<uint8_t*>(ctx->gate_mask.p);
    }
    int32_t* cnt_safe = static_cast<int32_t*>(ctx->gate_cnt.p);
    int32_t* bad = static_cast<int32_t*>(ctx->gate_bad.p);
    float4* xyzi = static_cast<float4*>(ctx->ego_xyzi.p);
    HIP_TRY(icp4r::launch_gate_guard(off, cnt, nscans, max_n, cap, cnt_safe, bad, st));
    int rc;
    // the kernel reads the caller's counts (a count above max_n is refused there) and the guard's flags
    if ((rc = run_reve(ctx, a, records, off, cnt, nscans, max_n, results, mask, xyzi, bad, st))) return rc;
    // the gate's compaction, as icp4r_compact_by_mask_batch_device launches it
    GateArgs g;
    memset(&g, 0, sizeof(g));
    g.tiles = std::max(1, (max_n + icp4r::kGateTile - 1) / icp4r::kGateTile);
    const size_t entries = (size_t)nscans * (size_t)g.tiles;
    HIP_TRY(ctx->gate_counts.ensure(entries * sizeof(int32_t)));
    HIP_TRY(ctx->gate_base.ensure(entries * sizeof(int64_t)));
    g.xyzi = xyzi;
    g.off = off;
    g.cnt = cnt_safe;  // 0 for a scan outside the workspace; a count outside [0, max_n] packs nothing
    g.mask = mask;
    g.nscans = nscans;
    g.max_n = max_n;
    g.all = 0;
    g.counts = static_cast<int32_t*>(ctx->gate_counts.p);
    g.base = static_cast<int64_t*>(ctx->gate_base.p);
    g.clouds = clouds;
    g.pair_off = pair_off;
    g.pair_n = pair_n;
    HIP_TRY(icp4r::launch_gate(g, st));
    return ICP4R_OK;
}

// Upload one host scan (n records) with off = 0, cnt = n into the sine estimator's staging buffers.
int upload_one(icp4r_ctx* ctx, const float* records, int32_t n, hipStream_t st) {
    const int64_t zero = 0;
    HIP_TRY(ctx->ego_rec.ensure((size_t)(n > 0 ? n : 1) * 5 * sizeof(float)));
    HIP_TRY(ctx->ego_off.ensure(sizeof(int64_t)));
    HIP_TRY(ctx->ego_cnt.ensure(sizeof(int32_t)));
    HIP_TRY(ctx->ego_res.ensure(sizeof(icp4r_reve_result)));
    if (n > 0) HIP_TRY(hipMemcpyAsync(ctx->ego_rec.p, records, (size_t)n * 5 * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->ego_off.p, &zero, sizeof(zero), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->ego_cnt.p, &n, sizeof(n), hipMemcpyHostToDevice, st));
    return ICP4R_OK;
}

}  // namespace

extern "C" {

void icp4r_reve_params_default(icp4r_reve_params* p) {  // radar_odometry.cpp:576-610
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->min_dist = 0.25;
    p->max_dist = 100;
    p->min_db = 0;
    p->elevation_thresh_deg = 60;
    p->azimuth_thresh_deg = 60;
    p->filter_min_z = -3;
    p->filter_max_z = 3;
    p->doppler_velocity_correction_factor = 1.0;
    p->thresh_zero_velocity = 0.05;
    p->allowed_outlier_percentage = 0.25;
    p->sigma_zero_velocity_x = 0.025;
    p->sigma_zero_velocity_y = 0.025;
    p->sigma_zero_velocity_z = 0.025;
    p->sigma_offset_radar_x = 0.05;
    p->sigma_offset_radar_y = 0.025;
    p->sigma_offset_radar_z = 0.05;
    p->max_sigma_x = 0.2;
    p->max_sigma_y = 0.2;
    p->max_sigma_z = 0.2;
    p->max_r_cond = 1000;
    p->use_cholesky_instead_of_bdcsvd = 1;
    p->use_ransac = 1;
    p->outlier_prob = 0.4;
    p->success_prob = 0.9999;
    p->N_ransac_points = 3;
    p->inlier_thresh = 0.15;
    p->use_odr = 1;
    p->sigma_v_d = 0.125;
    p->min_speed_odr = 4.0;
    p->model_noise_offset_deg = 2.0;
    p->model_noise_scale_deg = 10.0;
    p->seed = 0x4E7E5EEDull;
    p->use_z_filter = 0;
}

int32_t icp4r_reve_ransac_iterations(const icp4r_reve_params* params) {
    if (!params) return -1;
    return icp4r_reve::ransac_iterations(params->success_prob, params->outlier_prob);
}

int icp4r_reve_draw(uint64_t seed, int32_t k, int32_t n_valid, int32_t out[3]) {
    if (!out || n_valid < 3 || k < 0) return fail(ICP4R_E_INVALID, "bad draw (k = %d, n_valid = %d)", k, n_valid);
    icp4r_reve::draw(seed, k, n_valid, out);
    return ICP4R_OK;
}

int icp4r_reve_batch_device(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt,
                            int32_t nscans, int32_t max_n, const icp4r_reve_params* params,
                            icp4r_reve_result* results, uint8_t* inlier_mask, void* hip_stream) {
    if (!ctx || !results) return fail(ICP4R_E_INVALID, "ctx / results is NULL");
    int rc;
    ReveArgs a;
    if ((rc = check_shape(nscans, max_n)) || (rc = fill_args(params, a))) return rc;
    if (nscans == 0) return ICP4R_OK;
    if (!records || !off || !cnt) return fail(ICP4R_E_INVALID, "NULL device array");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    return run_reve(ctx, a, records, off, cnt, nscans, max_n, results, inlier_mask, nullptr, nullptr, st);
}

int icp4r_reve_inlier_clouds_batch_device(icp4r_ctx* ctx, const float* records, const int64_t* off,
                                          const int32_t* cnt, int32_t nscans, int32_t max_n,
                                          const icp4r_reve_params* params, icp4r_reve_result* results,
                                          uint8_t* inlier_mask, float* clouds, int64_t* pair_off, int32_t* pair_n,
                                          void* hip_stream) {
    if (!ctx || !results) return fail(ICP4R_E_INVALID, "ctx / results is NULL");
    int rc;
    ReveArgs a;
    if ((rc = check_shape(nscans, max_n)) || (rc = fill_args(params, a))) return rc;
    if (nscans == 0) return ICP4R_OK;
    if (!records || !off || !cnt || !clouds || !pair_off || !pair_n) return fail(ICP4R_E_INVALID, "NULL device array");
    if ((uintptr_t)clouds & 15) return fail(ICP4R_E_INVALID, "clouds not 16-B aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    return run_clouds(ctx, a, records, off, cnt, nscans, max_n, (int64_t)nscans * (max_n > 0 ? max_n : 1), results,
                      inlier_mask, reinterpret_cast<float4*>(clouds), pair_off, pair_n, st);
}

int icp4r_reve_estimate(icp4r_ctx* ctx, const float* records, int32_t n, const icp4r_reve_params* params,
                        icp4r_reve_result* out, uint8_t* inlier_mask_out) {
    if (!ctx || !out) return fail(ICP4R_E_INVALID, "NULL argument");
    if (n < 0 || (n > 0 && !records)) return fail(ICP4R_E_INVALID, "bad scan (n = %d)", n);
    int rc;
    ReveArgs a;
    if ((rc = check_shape(1, n)) || (rc = fill_args(params, a))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if ((rc = upload_one(ctx, records, n, st))) return rc;
    uint8_t* mask = nullptr;
    if (inlier_mask_out && n > 0) {
        HIP_TRY(ctx->ego_mask.ensure((size_t)n));
        mask = static_cast<uint8_t*>(ctx->ego_mask.p);
    }
    if ((rc = run_reve(ctx, a, static_cast<const float*>(ctx->ego_rec.p), static_cast<const int64_t*>(ctx->ego_off.p),
                       static_cast<const int32_t*>(ctx->ego_cnt.p), 1, n, static_cast<icp4r_reve_result*>(ctx->ego_res.p),
                       mask, nullptr, nullptr, st)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->ego_res.p, sizeof(*out), hipMemcpyDeviceToHost, st));
    if (mask) HIP_TRY(hipMemcpyAsync(inlier_mask_out, mask, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n == 0) return fail(ICP4R_E_EMPTY, "empty scan");
    return ICP4R_OK;
}

int icp4r_reve_inlier_cloud(icp4r_ctx* ctx, const float* records, int32_t n, const icp4r_reve_params* params,
                            icp4r_reve_result* out, float* xyzi_out, int32_t* n_inliers) {
    if (!ctx || !out || !n_inliers) return fail(ICP4R_E_INVALID, "NULL argument");
    if (n < 0 || (n > 0 && (!records || !xyzi_out))) return fail(ICP4R_E_INVALID, "bad scan (n = %d)", n);
    int rc;
    ReveArgs a;
    if ((rc = check_shape(1, n)) || (rc = fill_args(params, a))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t cap = (size_t)(n > 0 ? n : 1);
    if ((rc = upload_one(ctx, records, n, st))) return rc;
    HIP_TRY(ctx->gate_clouds.ensure(cap * sizeof(float4)));
    HIP_TRY(ctx->gate_pair_off.ensure(2 * sizeof(int64_t)));
    HIP_TRY(ctx->gate_pair_n.ensure(2 * sizeof(int32_t)));
    if ((rc = run_clouds(ctx, a, static_cast<const float*>(ctx->ego_rec.p), static_cast<const int64_t*>(ctx->ego_off.p),
                         static_cast<const int32_t*>(ctx->ego_cnt.p), 1, n, (int64_t)cap,
                         static_cast<icp4r_reve_result*>(ctx->ego_res.p), nullptr, static_cast<float4*>(ctx->gate_clouds.p),
                         static_cast<int64_t*>(ctx->gate_pair_off.p), static_cast<int32_t*>(ctx->gate_pair_n.p), st)))
        return rc;
    int32_t pn[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(out, ctx->ego_res.p, sizeof(*out), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pn, ctx->gate_pair_n.p, sizeof(pn), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_inliers = pn[1];
    if (pn[1] > 0) {
        HIP_TRY(hipMemcpyAsync(xyzi_out, ctx->gate_clouds.p, (size_t)pn[1] * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (n == 0) return fail(ICP4R_E_EMPTY, "empty scan");
    return ICP4R_OK;
}

}  // extern "C"
