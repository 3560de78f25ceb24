// icp4r_vgicp.cpp — C ABI of the voxelized generalized ICP (include/icp4r/icp4r_vgicp.h).
//
// FastVGICP::align as one stream-ordered launch sequence per batch, on the GICP's host stages
// (icp4r_gicp_host.hpp) and the kernels of icp4r_vgicp.hip:
//
//   begin                          validate, x0 := guess, the k-NN covariances of both clouds
//   launch_vgicp_map               the targets' Gaussian voxel maps
//   repeat                         launch_vgicp_iter (the lookup and linearisation, the trials); no
//                                  nearest-neighbour pass; the active-pair checks as GICP
//   end                            getFitnessScore by one exact NN pass, results, aligned clouds
//
// No CPU fallback: every entry fails with ICP4R_E_HIP if the device path cannot run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "icp4r/icp4r_vgicp.h"
#include "icp4r_batch.hpp"
#include "icp4r_gicp_host.hpp"
#include "icp4r_host.hpp"
#include "icp4r_internal.hpp"
#include "icp4r_vgicp.hpp"
#include "icp4r_vgicp_math.hpp"

using namespace icp4r;
using icp4r_host::EventPair;
using icp4r_host::fail;

namespace {

int check_vparams(const icp4r_vgicp_params* p) {
    int rc;
    if ((rc = icp4r_gicp_host::check_params(&p->gicp))) return rc;
    if (!(p->voxel_resolution > 0) || !isfinite(p->voxel_resolution))
        return fail(ICP4R_E_INVALID, "voxel_resolution must be > 0 and finite");
    if (p->neighbor_search < ICP4R_VGICP_DIRECT1 || p->neighbor_search > ICP4R_VGICP_DIRECT27)
        return fail(ICP4R_E_INVALID, "neighbor_search %d: only DIRECT1, DIRECT7 and DIRECT27 are offered", p->neighbor_search);
    if (p->voxel_accumulation != ICP4R_VGICP_ADDITIVE)
        return fail(ICP4R_E_INVALID, "voxel_accumulation %d: only ADDITIVE is offered", p->voxel_accumulation);
    return ICP4R_OK;
}

int run_vgicp(icp4r_ctx* ctx, const PairArgs& a, int npairs, int max_n, int max_m, const icp4r_vgicp_params& vp,
              hipStream_t st) {
    if (npairs <= 0) return ICP4R_OK;
    // the map's elements are indexed by int32 (npairs * t_stride of them, t_stride = max(max_m, 1) as begin
    // sets it): refused before anything is queued
    if ((int64_t)npairs * (max_m > 0 ? max_m : 1) > INT32_MAX)
        return fail(ICP4R_E_INVALID, "batch of more than 2^31 target slots (%d pairs x %d)", npairs, max_m);
    icp4r_gicp_host::Work k;
    int rc;
    // (with compute_fitness = 0 the target gets no index beyond the one its k-NN covariances walk)
    if ((rc = icp4r_gicp_host::begin(ctx, a, npairs, max_n, max_m, vp.gicp, false, st, k))) return rc;
    VgicpArgs m;
    m.t_stride = k.g.t_stride;
    m.resolution = vp.voxel_resolution;
    m.mode = vp.neighbor_search;
    m.noff = icp4r_vgicp::offset_count(m.mode);
    const VgicpLayout L = vgicp_layout(npairs, m.t_stride, k.w.x_stride, m.noff);
    HIP_TRY(ctx->vgicp_work.ensure(L.bytes));
    vgicp_bind(ctx->vgicp_work.p, L, m);
    HIP_TRY(launch_vgicp_map(a.tgt, a.tgt_off, a.tgt_n, k.g.cov_tgt, k.w.state, m, npairs, st));
    const bool kev = ctx->kernel_timing;
    auto step = [&](int it) -> int {
        int rc;
        EventPair* ue = nullptr;
        if (kev) {
            if ((rc = icp4r_pipe::next_event(ctx->upd_events, ctx->upd_used, &ue))) return rc;
            HIP_TRY(hipEventRecord(ue->start, st));
        }
        HIP_TRY(launch_vgicp_iter(a, k.w, k.g, m, npairs, k.mn, it, st));
        if (kev) HIP_TRY(hipEventRecord(ue->stop, st));
        return ICP4R_OK;
    };
    if ((rc = icp4r_gicp_host::iterate(ctx, k, npairs, vp.gicp.max_iterations, st, step))) return rc;
    return icp4r_gicp_host::end(ctx, a, k, npairs, true, st);
}

}  // namespace

extern "C" {

void icp4r_vgicp_params_default(icp4r_vgicp_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    icp4r_gicp_params_default(&p->gicp);
    p->voxel_resolution = 1.0;
    p->neighbor_search = ICP4R_VGICP_DIRECT1;
    p->voxel_accumulation = ICP4R_VGICP_ADDITIVE;
}

int icp4r_vgicp_align_batch_device(icp4r_ctx* ctx, const icp4r_batch* b, const icp4r_vgicp_params* params,
                                   icp4r_result* results, void* hip_stream) {
    if (!ctx || !b || !results) return fail(ICP4R_E_INVALID, "ctx/batch/results is NULL");
    int rc;
    PairArgs a;
    if ((rc = icp4r_gicp_host::pair_args(b, results, a))) return rc;
    icp4r_vgicp_params vp;
    if (params) vp = *params;
    else icp4r_vgicp_params_default(&vp);
    if ((rc = check_vparams(&vp))) return rc;
    if (b->npairs == 0) return ICP4R_OK;
    if ((rc = icp4r_gicp_host::kparams(vp.gicp, &a.kp))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    return run_vgicp(ctx, a, b->npairs, b->max_src_n, b->max_tgt_n, vp, st);
}

int icp4r_vgicp_align(icp4r_ctx* ctx, const float* src, int32_t n, int32_t src_stride_bytes, const float* tgt,
                      int32_t m, int32_t tgt_stride_bytes, const float* guess, const icp4r_vgicp_params* params,
                      icp4r_result* out, float* aligned_out, int32_t out_stride_bytes) {
    return icp4r_gicp_host::align_host(ctx, src, n, src_stride_bytes, tgt, m, tgt_stride_bytes, guess, out, aligned_out,
                                       out_stride_bytes, "FastVGICP",
                                       [&](const icp4r_batch& b, icp4r_result* res, hipStream_t st) {
                                           return icp4r_vgicp_align_batch_device(ctx, &b, params, res, st);
                                       });
}

int icp4r_vgicp_voxel_map(icp4r_ctx* ctx, const float* cloud, int32_t n, int32_t stride_bytes, const double* cov_in,
                          int32_t k, int32_t regularization, double resolution, int32_t cap, int32_t* coords_out,
                          int32_t* num_points_out, double* mean_out, double* cov_out, int32_t* n_voxels) {
    using namespace icp4r_host;
    if (!ctx || !n_voxels) return fail(ICP4R_E_INVALID, "ctx/n_voxels is NULL");
    *n_voxels = 0;
    if (!(resolution > 0) || !isfinite(resolution)) return fail(ICP4R_E_INVALID, "resolution must be > 0 and finite");
    if (cap < 0) return fail(ICP4R_E_INVALID, "cap < 0");
    int rc;
    if ((rc = check_cloud(cloud, n, stride_bytes, "cloud"))) return rc;
    if (n == 0) return ICP4R_OK;
    // the covariances' upper triangles: the caller's, or the k-NN ones (icp4r_gicp_covariances validates k
    // and the regularisation)
    std::vector<double> c9;
    if (!cov_in) {
        c9.resize((size_t)n * 9);
        if ((rc = icp4r_gicp_covariances(ctx, cloud, n, stride_bytes, k, regularization, c9.data()))) return rc;
        cov_in = c9.data();
    }
    std::vector<double> c6((size_t)n * 6);
    static const int up[6] = {0, 1, 2, 4, 5, 8};
    for (int32_t i = 0; i < n; ++i)
        for (int t = 0; t < 6; ++t) c6[(size_t)i * 6 + t] = cov_in[(size_t)i * 9 + up[t]];
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<float> hc;
    pack_host(cloud, n, stride_bytes, hc);
    for (int32_t i = 0; i < n; ++i)
        if (!(isfinite(hc[4 * (size_t)i]) && isfinite(hc[4 * (size_t)i + 1]) && isfinite(hc[4 * (size_t)i + 2])))
            return fail(ICP4R_E_NONFINITE, "non-finite coordinate in the cloud");
    const int64_t zero64 = 0;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx->tgt.ensure(hc.size() * sizeof(float)));
    HIP_TRY(ctx->tgt_off.ensure(16));
    HIP_TRY(ctx->tgt_n.ensure(16));
    HIP_TRY(ctx->vgicp_cov.ensure(c6.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(ctx->tgt.p, hc.data(), hc.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->tgt_off.p, &zero64, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->tgt_n.p, &n, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->vgicp_cov.p, c6.data(), c6.size() * sizeof(double), hipMemcpyHostToDevice, st));
    VgicpArgs m;
    m.t_stride = n;
    m.resolution = resolution;
    m.mode = ICP4R_VGICP_DIRECT1;
    m.noff = 1;
    const VgicpLayout L = vgicp_layout(1, n, 0, 1);
    HIP_TRY(ctx->vgicp_work.ensure(L.bytes));
    vgicp_bind(ctx->vgicp_work.p, L, m);
    HIP_TRY(launch_vgicp_map(static_cast<const float4*>(ctx->tgt.p), static_cast<const int64_t*>(ctx->tgt_off.p),
                             static_cast<const int32_t*>(ctx->tgt_n.p), static_cast<const double*>(ctx->vgicp_cov.p),
                             nullptr, m, 1, st));
    int32_t head[2] = {0, 0};  // the voxels; the out-of-range flag
    HIP_TRY(hipMemcpyAsync(&head[0], m.total, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&head[1], m.bad, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (head[1]) return fail(ICP4R_E_INVALID, "a coordinate lies outside +-2^20 cells of resolution %g", resolution);
    const int32_t nv = head[0];
    *n_voxels = nv;
    if (nv > cap) return fail(ICP4R_E_INVALID, "%d voxels, room for %d", nv, cap);
    if (nv == 0) return ICP4R_OK;
    std::vector<uint64_t> hk((size_t)nv);
    std::vector<double> hv((size_t)nv * 6);
    HIP_TRY(hipMemcpyAsync(hk.data(), m.vkey, hk.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (num_points_out) HIP_TRY(hipMemcpyAsync(num_points_out, m.vnum, (size_t)nv * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (mean_out) HIP_TRY(hipMemcpyAsync(mean_out, m.vmean, (size_t)nv * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hv.data(), m.vcov, hv.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    static const int idx[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
    for (int32_t v = 0; v < nv; ++v) {
        if (coords_out) icp4r_vgicp::key_cell(hk[(size_t)v], coords_out + (size_t)v * 3);
        if (cov_out)
            for (int t = 0; t < 9; ++t) cov_out[(size_t)v * 9 + t] = hv[(size_t)v * 6 + idx[t]];
    }
    return ICP4R_OK;
}

}  // extern "C"
