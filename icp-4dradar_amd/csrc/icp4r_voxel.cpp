// icp4r_voxel.cpp — C ABI of the voxel-grid filter (include/icp4r/icp4r_voxel.h; kernels:
// icp4r_voxel.hip).  The workspace, the staging buffers and the timing events belong to the context
// and only grow, so calls on one context must not overlap (as with every other entry).  The device
// entries run without a host round trip (the radix sort covers all 31 key bits); the host entries
// read the grid back between the two stages, answer overflow and the empty cloud there, and sort only
// the bits the grid needs.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <math.h>

#include <vector>

#include "icp4r/icp4r_voxel.h"
#include "icp4r_host.hpp"
#include "icp4r_internal.hpp"

using icp4r_host::EventPair;
using icp4r_host::fail;
using icp4r_host::pack_host;

namespace {

int make_args(const icp4r_voxel_params* p, icp4r::VoxelArgs* a) {
    if (!p) return fail(ICP4R_E_INVALID, "params is NULL");
    for (int k = 0; k < 3; ++k) {
        if (!(p->leaf[k] > 0.0f) || !std::isfinite(p->leaf[k]))
            return fail(ICP4R_E_INVALID, "leaf[%d] = %g: must be finite and > 0", k, (double)p->leaf[k]);
        a->inv[k] = 1.0f / p->leaf[k];
    }
    a->all_data = p->downsample_all_data ? 1 : 0;
    a->min_pts = p->min_points_per_voxel;
    return ICP4R_OK;
}

int check_n(int64_t n) {
    if (n < 0) return fail(ICP4R_E_INVALID, "n must be >= 0");
    if (n >= ((int64_t)1 << 31)) return fail(ICP4R_E_TOO_LARGE, "voxel filter: %lld points", (long long)n);
    return ICP4R_OK;
}

int event_pair(icp4r_ctx* ctx, EventPair** ev) {
    if (ctx->vox_used == ctx->vox_events.size()) {
        EventPair e;
        HIP_TRY(hipEventCreate(&e.start));
        HIP_TRY(hipEventCreate(&e.stop));
        ctx->vox_events.push_back(e);
    }
    *ev = &ctx->vox_events[ctx->vox_used++];
    return ICP4R_OK;
}

// The radix sort's key width for a grid of `cells` leaves: 2^bits > cells, so the low bits of the
// non-participating key (all ones) stay above every leaf index.
int key_bits(int64_t cells) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) <= cells) ++b;
    return b;
}

// n > 0 device points -> d_out / d_count on st.  grid_out: the host entries' round trip (the stream
// is synchronised and the grid returned; on overflow or an empty cloud stage 2 is not launched).
int run(icp4r_ctx* ctx, const float4* d_pts, int64_t n, const icp4r::VoxelArgs& a, float4* d_out, int32_t* d_count,
        hipStream_t st, icp4r::VoxelGridDev* grid_out) {
    const icp4r::VoxelLayout L = icp4r::voxel_layout(n);
    HIP_TRY(ctx->vox_work.ensure(L.bytes));
    EventPair* ev = nullptr;
    int rc;
    if ((rc = event_pair(ctx, &ev))) return rc;
    HIP_TRY(hipEventRecord(ev->start, st));
    HIP_TRY(icp4r::launch_voxel_grid(d_pts, n, a, ctx->vox_work.p, st));
    int bits = 31;
    if (grid_out) {
        HIP_TRY(hipMemcpyAsync(grid_out, static_cast<char*>(ctx->vox_work.p) + L.grid, sizeof(*grid_out),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (grid_out->flag != 0) {
            HIP_TRY(hipEventRecord(ev->stop, st));
            return ICP4R_OK;
        }
        bits = key_bits((int64_t)grid_out->div[0] * grid_out->div[1] * grid_out->div[2]);
    }
    HIP_TRY(icp4r::launch_voxel_filter(d_pts, n, a, bits, ctx->vox_work.p, d_out, d_count, st));
    HIP_TRY(hipEventRecord(ev->stop, st));
    return ICP4R_OK;
}

// The host entries' second half: d_pts (n > 0) are on the device.
int run_host(icp4r_ctx* ctx, const float4* d_pts, int64_t n, const icp4r::VoxelArgs& a, float* out, int64_t out_cap,
             int64_t* out_n) {
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx->vox_out.ensure((size_t)n * sizeof(float4)));
    HIP_TRY(ctx->vox_cnt.ensure(sizeof(int32_t)));
    icp4r::VoxelGridDev g = {};
    int rc;
    if ((rc = run(ctx, d_pts, n, a, static_cast<float4*>(ctx->vox_out.p), static_cast<int32_t*>(ctx->vox_cnt.p), st, &g))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (g.flag < 0) {
        *out_n = -1;
        return fail(ICP4R_E_TOO_LARGE, "voxel filter: leaf size is too small for the input dataset (grid overflow)");
    }
    if (g.flag > 0) {
        *out_n = 0;
        return ICP4R_OK;
    }
    int32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, ctx->vox_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_n = cnt;
    if (cnt > out_cap) return fail(ICP4R_E_TOO_LARGE, "voxel filter: %d voxels, out_cap %lld", cnt, (long long)out_cap);
    if (cnt > 0) {
        HIP_TRY(hipMemcpyAsync(out, ctx->vox_out.p, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ICP4R_OK;
}

int check_ctx(const icp4r_ctx* ctx) {
    if (!ctx) return fail(ICP4R_E_INVALID, "ctx is NULL");
    if (ctx->device < 0) return fail(ICP4R_E_INVALID, "voxel filter: a context without a device");
    return ICP4R_OK;
}

}  // namespace

extern "C" {

int icp4r_voxel_params_default(icp4r_voxel_params* p) {
    if (!p) return fail(ICP4R_E_INVALID, "params is NULL");
    p->leaf[0] = p->leaf[1] = p->leaf[2] = 0.0f;
    p->downsample_all_data = 1;
    p->min_points_per_voxel = 0;
    return ICP4R_OK;
}

int icp4r_voxel_filter(icp4r_ctx* ctx, const float* pts, int64_t n, int32_t stride_bytes, const icp4r_voxel_params* params,
                       float* out, int64_t out_cap, int64_t* out_n) {
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!out_n || (out_cap > 0 && !out)) return fail(ICP4R_E_INVALID, "out/out_n is NULL");
    icp4r::VoxelArgs a;
    if ((rc = make_args(params, &a))) return rc;
    if ((rc = check_n(n))) return rc;
    if (stride_bytes < 12 || stride_bytes % 4)
        return fail(ICP4R_E_INVALID, "points: stride %d bytes (need >= 12, multiple of 4)", stride_bytes);
    if (n > 0 && !pts) return fail(ICP4R_E_INVALID, "points is NULL");
    *out_n = 0;
    if (n == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<float> h;
    pack_host(pts, n, stride_bytes, h);
    HIP_TRY(ctx->vox_in.ensure((size_t)n * sizeof(float4)));
    HIP_TRY(hipMemcpyAsync(ctx->vox_in.p, h.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    return run_host(ctx, static_cast<const float4*>(ctx->vox_in.p), n, a, out, out_cap, out_n);  // synchronises: h is done with
}

int icp4r_voxel_filter_device(icp4r_ctx* ctx, const float* d_pts, int64_t n, const icp4r_voxel_params* params, float* d_out,
                              int32_t* d_count, void* hip_stream) {
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!d_count) return fail(ICP4R_E_INVALID, "d_count is NULL");
    icp4r::VoxelArgs a;
    if ((rc = make_args(params, &a))) return rc;
    if ((rc = check_n(n))) return rc;
    if (n > 0 && (!d_pts || !d_out)) return fail(ICP4R_E_INVALID, "d_pts/d_out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int32_t), st));
        return ICP4R_OK;
    }
    return run(ctx, reinterpret_cast<const float4*>(d_pts), n, a, reinterpret_cast<float4*>(d_out), d_count, st, nullptr);
}

int icp4r_map_voxel_filter(icp4r_map* map, const icp4r_voxel_params* params, float* out, int64_t out_cap, int64_t* out_n) {
    if (!map || !out_n || (out_cap > 0 && !out)) return fail(ICP4R_E_INVALID, "NULL argument");
    const float* d_pts = nullptr;
    int64_t n = 0;
    int rc;
    if ((rc = icp4r_map_points_device(map, &d_pts, &n))) return rc;  // a detached map: ICP4R_E_INVALID, no HIP call
    icp4r_ctx* ctx = icp4r_host::map_context(map);
    icp4r::VoxelArgs a;
    if ((rc = make_args(params, &a))) return rc;
    if ((rc = check_n(n))) return rc;
    *out_n = 0;
    if (n == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return run_host(ctx, reinterpret_cast<const float4*>(d_pts), n, a, out, out_cap, out_n);
}

int icp4r_map_voxel_filter_device(icp4r_map* map, const icp4r_voxel_params* params, float* d_out, int32_t* d_count,
                                  void* hip_stream) {
    if (!map) return fail(ICP4R_E_INVALID, "map is NULL");
    const float* d_pts = nullptr;
    int64_t n = 0;
    int rc;
    if ((rc = icp4r_map_points_device(map, &d_pts, &n))) return rc;
    return icp4r_voxel_filter_device(icp4r_host::map_context(map), d_pts, n, params, d_out, d_count, hip_stream);
}

int icp4r_voxel_time_ms(icp4r_ctx* ctx, double* avg_ms, int32_t* calls) {
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!avg_ms) return fail(ICP4R_E_INVALID, "avg_ms is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    double tot = 0.0;
    for (size_t i = 0; i < ctx->vox_used; ++i) {
        HIP_TRY(hipEventSynchronize(ctx->vox_events[i].stop));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->vox_events[i].start, ctx->vox_events[i].stop));
        tot += ms;
    }
    *avg_ms = ctx->vox_used ? tot / (double)ctx->vox_used : 0.0;
    if (calls) *calls = (int32_t)ctx->vox_used;
    return ICP4R_OK;
}

int icp4r_voxel_time_reset(icp4r_ctx* ctx) {
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    ctx->vox_used = 0;
    return ICP4R_OK;
}

}  // extern "C"
