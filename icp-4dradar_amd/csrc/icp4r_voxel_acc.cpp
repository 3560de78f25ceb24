// icp4r_voxel_acc.cpp — C ABI of the incremental voxel grid (include/icp4r/icp4r_voxel_acc.h; kernels:
// icp4r_voxel_acc.hip).  The accumulator owns its state (two structure-of-arrays buffers that the adds
// alternate between), its device head, the add workspace and the host entries' staging; all only grow.
// The host keeps an upper bound on the voxel count (the count last read back + the points added
// since), which sizes every launch and decides growth, so the device entries run without a host round
// trip.  Lifetime as the map store's: a context lists its accumulators and detaches them when it is
// destroyed.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "icp4r/icp4r_voxel_acc.h"
#include "icp4r_host.hpp"
#include "icp4r_internal.hpp"

using icp4r_host::DevBuf;
using icp4r_host::fail;
using icp4r_host::pack_host;

struct icp4r_voxel_acc {
    icp4r_ctx* ctx = nullptr;  // nullptr: detached (the context was destroyed)
    icp4r::VoxelArgs args = {};
    DevBuf meta, work, in, out, cnt, scan;
    DevBuf key[2], sums[2], count[2];
    int cur = 0;          // the buffer that holds the state
    int64_t cap = 0;      // voxels each state buffer holds
    int64_t bound = 0;    // >= the device's voxel count
    uint64_t points = 0;  // the running sum of n
};

namespace {

constexpr int64_t kInitialCap = 4096;

#define ACC_LIVE(a)                                                                                    \
    do {                                                                                               \
        if (!(a)) return fail(ICP4R_E_INVALID, "accumulator is NULL");                                 \
        if (!(a)->ctx) return fail(ICP4R_E_INVALID, "voxel accumulator: its context was destroyed");   \
    } while (0)

icp4r::AccMeta* meta_of(icp4r_voxel_acc* a) { return static_cast<icp4r::AccMeta*>(a->meta.p); }

icp4r::AccState state_of(icp4r_voxel_acc* a, int which) {
    return icp4r::AccState{static_cast<uint64_t*>(a->key[which].p), static_cast<float4*>(a->sums[which].p),
                           static_cast<uint32_t*>(a->count[which].p)};
}

void release_device(icp4r_voxel_acc* a) {
    for (DevBuf* b : {&a->meta, &a->work, &a->in, &a->out, &a->cnt, &a->scan, &a->key[0], &a->key[1], &a->sums[0], &a->sums[1],
                      &a->count[0], &a->count[1]})
        b->release();
    a->cap = a->bound = 0;
}

// After a synchronisation of st: the device's voxel count becomes the bound.
int read_count(icp4r_voxel_acc* a, hipStream_t st) {
    int32_t nv = 0;
    HIP_TRY(hipMemcpyAsync(&nv, &meta_of(a)->nvox, sizeof(nv), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    a->bound = nv;
    return ICP4R_OK;
}

// Room for `need` voxels in both buffers; the state is kept.  The caller has synchronised st.
int grow(icp4r_voxel_acc* a, int64_t need, hipStream_t st) {
    if (need <= a->cap) return ICP4R_OK;
    int64_t cap = std::max<int64_t>(std::max<int64_t>(need, 2 * a->cap), kInitialCap);
    cap = std::min<int64_t>((cap + 1) & ~(int64_t)1, (int64_t)1 << 31);
    DevBuf k, s, c;
    HIP_TRY(k.ensure((size_t)cap * sizeof(uint64_t)));
    HIP_TRY(s.ensure((size_t)cap * sizeof(float4)));
    HIP_TRY(c.ensure((size_t)cap * sizeof(uint32_t)));
    if (a->bound > 0) {
        const size_t nv = (size_t)a->bound;
        HIP_TRY(hipMemcpyAsync(k.p, a->key[a->cur].p, nv * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(s.p, a->sums[a->cur].p, nv * sizeof(float4), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(c.p, a->count[a->cur].p, nv * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    a->key[a->cur].release(), a->sums[a->cur].release(), a->count[a->cur].release();
    a->key[a->cur] = k, a->sums[a->cur] = s, a->count[a->cur] = c;
    const int other = a->cur ^ 1;
    HIP_TRY(a->key[other].ensure((size_t)cap * sizeof(uint64_t)));
    HIP_TRY(a->sums[other].ensure((size_t)cap * sizeof(float4)));
    HIP_TRY(a->count[other].ensure((size_t)cap * sizeof(uint32_t)));
    a->cap = cap;
    return ICP4R_OK;
}

// Capacity for `extra` more voxels: only when the bound says so, a round trip and, if the true count
// says so too, a growth.
int ensure_room(icp4r_voxel_acc* a, int64_t extra, hipStream_t st) {
    if (a->bound + extra <= a->cap) return ICP4R_OK;
    int rc;
    if ((rc = read_count(a, st))) return rc;
    if (a->bound + extra >= ((int64_t)1 << 31))
        return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: %lld voxels", (long long)(a->bound + extra));
    return grow(a, a->bound + extra, st);
}

// The radix sort's key width for a scan box of `cells` cells: 2^bits > cells, so the low bits of the
// non-participating key (all ones) stay above every cell number.
int key_bits(int64_t cells) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) <= cells) ++b;
    return b;
}

// n > 0 device points on st.  host: the entry may synchronise — it reads the scan's verdict back before
// anything merges (a scan outside the range is refused, one without a participating point is done) and
// sorts only the bits the scan's own box needs; it leaves the stream idle and the bound exact.
int add_points(icp4r_voxel_acc* a, const float4* d_pts, int64_t n, hipStream_t st, bool host) {
    if (a->points + (uint64_t)n >= ((uint64_t)1 << 32))
        return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: %llu points added in total", (unsigned long long)(a->points + (uint64_t)n));
    int rc;
    if ((rc = ensure_room(a, n, st))) return rc;
    const icp4r::AccLayout L = icp4r::acc_layout(n);
    HIP_TRY(a->work.ensure(L.bytes));
    HIP_TRY(icp4r::launch_acc_prep(d_pts, n, a->args, meta_of(a), a->work.p, host ? 0 : 1, st));
    int sort_bits = 0;
    if (host) {
        icp4r::AccScanInfo info = {};
        HIP_TRY(hipMemcpyAsync(&info, static_cast<char*>(a->work.p) + L.info, sizeof(info), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (info.skip == 2)
            return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: the scan leaves the range of +-2^20 cells around the origin");
        a->points += (uint64_t)n;
        if (info.skip == 1) return ICP4R_OK;
        if (info.cells <= INT32_MAX) sort_bits = key_bits(info.cells);
    } else {
        a->points += (uint64_t)n;
    }
    HIP_TRY(icp4r::launch_acc_merge(d_pts, n, a->args, sort_bits, meta_of(a), state_of(a, a->cur), state_of(a, a->cur ^ 1),
                                    a->bound, a->work.p, st));
    a->cur ^= 1;
    a->bound += n;
    if (host) return read_count(a, st);
    return ICP4R_OK;
}

int run_filter(icp4r_voxel_acc* a, float4* d_out, int32_t* d_count, hipStream_t st) {
    if (a->args.min_pts > 1) HIP_TRY(a->scan.ensure(icp4r::acc_filter_scan_bytes(a->bound)));
    HIP_TRY(icp4r::launch_acc_filter(meta_of(a), state_of(a, a->cur), a->bound, a->args, static_cast<int32_t*>(a->scan.p), d_out,
                                     d_count, st));
    return ICP4R_OK;
}

}  // namespace

namespace icp4r_host {

void voxel_acc_detach(icp4r_voxel_acc* a) {
    release_device(a);
    a->ctx = nullptr;
}

}  // namespace icp4r_host

extern "C" {

int icp4r_voxel_acc_create(icp4r_ctx* ctx, const icp4r_voxel_params* p, icp4r_voxel_acc** out) {
    if (!ctx || !out) return fail(ICP4R_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (ctx->device < 0) return fail(ICP4R_E_INVALID, "icp4r_voxel_acc_create: a context without a device");
    if (!p) return fail(ICP4R_E_INVALID, "params is NULL");
    icp4r::VoxelArgs args;
    for (int k = 0; k < 3; ++k) {
        if (!(p->leaf[k] > 0.0f) || !std::isfinite(p->leaf[k]))
            return fail(ICP4R_E_INVALID, "leaf[%d] = %g: must be finite and > 0", k, (double)p->leaf[k]);
        args.inv[k] = 1.0f / p->leaf[k];
    }
    args.all_data = p->downsample_all_data ? 1 : 0;
    args.min_pts = p->min_points_per_voxel;
    HIP_TRY(hipSetDevice(ctx->device));
    icp4r_voxel_acc* a = new icp4r_voxel_acc();
    a->args = args;
    hipError_t e = a->meta.ensure(sizeof(icp4r::AccMeta));
    if (e == hipSuccess) e = icp4r::launch_acc_clear(meta_of(a), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        release_device(a);
        delete a;
        return fail(ICP4R_E_HIP, "icp4r_voxel_acc_create: %s", hipGetErrorString(e));
    }
    a->ctx = ctx;
    ctx->voxel_accs.push_back(a);
    *out = a;
    return ICP4R_OK;
}

int icp4r_voxel_acc_destroy(icp4r_voxel_acc* a) {
    if (!a) return ICP4R_OK;
    if (a->ctx) {
        auto& v = a->ctx->voxel_accs;
        v.erase(std::remove(v.begin(), v.end(), a), v.end());
        (void)hipSetDevice(a->ctx->device);
        (void)hipStreamSynchronize(a->ctx->stream);
        release_device(a);
    }
    delete a;
    return ICP4R_OK;
}

int icp4r_voxel_acc_clear(icp4r_voxel_acc* a) {
    ACC_LIVE(a);
    HIP_TRY(hipSetDevice(a->ctx->device));
    HIP_TRY(icp4r::launch_acc_clear(meta_of(a), a->ctx->stream));
    HIP_TRY(hipStreamSynchronize(a->ctx->stream));
    a->bound = 0;
    a->points = 0;
    return ICP4R_OK;
}

int icp4r_voxel_acc_reserve(icp4r_voxel_acc* a, int64_t voxels) {
    ACC_LIVE(a);
    if (voxels < 0) return fail(ICP4R_E_INVALID, "voxels must be >= 0");
    if (voxels >= ((int64_t)1 << 31)) return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: %lld voxels", (long long)voxels);
    if (voxels <= a->cap) return ICP4R_OK;
    HIP_TRY(hipSetDevice(a->ctx->device));
    int rc;
    if ((rc = read_count(a, a->ctx->stream))) return rc;
    return grow(a, voxels, a->ctx->stream);
}

int icp4r_voxel_acc_add(icp4r_voxel_acc* a, const float* pts, int64_t n, int32_t stride_bytes) {
    ACC_LIVE(a);
    if (n < 0) return fail(ICP4R_E_INVALID, "n must be >= 0");
    if (n >= ((int64_t)1 << 31)) return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: %lld points", (long long)n);
    if (stride_bytes < 12 || stride_bytes % 4)
        return fail(ICP4R_E_INVALID, "points: stride %d bytes (need >= 12, multiple of 4)", stride_bytes);
    if (n > 0 && !pts) return fail(ICP4R_E_INVALID, "points is NULL");
    if (n == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(a->ctx->device));
    hipStream_t st = a->ctx->stream;
    std::vector<float> h;
    pack_host(pts, n, stride_bytes, h);
    HIP_TRY(a->in.ensure((size_t)n * sizeof(float4)));
    HIP_TRY(hipMemcpyAsync(a->in.p, h.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, st));
    const int rc = add_points(a, static_cast<const float4*>(a->in.p), n, st, true);
    (void)hipStreamSynchronize(st);  // h is done with on every path
    return rc;
}

int icp4r_voxel_acc_add_device(icp4r_voxel_acc* a, const float* d_pts, int64_t n, void* hip_stream) {
    ACC_LIVE(a);
    if (n < 0) return fail(ICP4R_E_INVALID, "n must be >= 0");
    if (n >= ((int64_t)1 << 31)) return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: %lld points", (long long)n);
    if (n > 0 && !d_pts) return fail(ICP4R_E_INVALID, "d_pts is NULL");
    if (n == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(a->ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : a->ctx->stream;
    return add_points(a, reinterpret_cast<const float4*>(d_pts), n, st, false);
}

int icp4r_voxel_acc_add_map(icp4r_voxel_acc* a, icp4r_map* map) {
    ACC_LIVE(a);
    if (!map) return fail(ICP4R_E_INVALID, "map is NULL");
    const float* d_pts = nullptr;
    int64_t n = 0;
    int rc;
    if ((rc = icp4r_map_points_device(map, &d_pts, &n))) return rc;  // a detached map: ICP4R_E_INVALID, no HIP call
    if (icp4r_host::map_context(map) != a->ctx) return fail(ICP4R_E_INVALID, "voxel accumulator: a map of another context");
    if (n >= ((int64_t)1 << 31)) return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: %lld points", (long long)n);
    if (n == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(a->ctx->device));
    return add_points(a, reinterpret_cast<const float4*>(d_pts), n, a->ctx->stream, true);
}

int icp4r_voxel_acc_filter(icp4r_voxel_acc* a, float* out, int64_t out_cap, int64_t* out_n) {
    ACC_LIVE(a);
    if (!out_n || (out_cap > 0 && !out)) return fail(ICP4R_E_INVALID, "out/out_n is NULL");
    HIP_TRY(hipSetDevice(a->ctx->device));
    hipStream_t st = a->ctx->stream;
    int rc;
    if ((rc = read_count(a, st))) return rc;
    HIP_TRY(a->out.ensure((size_t)std::max<int64_t>(a->bound, 1) * sizeof(float4)));
    HIP_TRY(a->cnt.ensure(sizeof(int32_t)));
    if ((rc = run_filter(a, static_cast<float4*>(a->out.p), static_cast<int32_t*>(a->cnt.p), st))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    int32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, a->cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_n = cnt;
    if (cnt == -1)
        return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: leaf size is too small for the accumulated dataset (grid overflow)");
    if (cnt == -2) return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: a device add left the range and was skipped");
    if (cnt > out_cap) return fail(ICP4R_E_TOO_LARGE, "voxel accumulator: %d voxels, out_cap %lld", cnt, (long long)out_cap);
    if (cnt > 0) {
        HIP_TRY(hipMemcpyAsync(out, a->out.p, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ICP4R_OK;
}

int icp4r_voxel_acc_filter_device(icp4r_voxel_acc* a, float* d_out, int32_t* d_count, void* hip_stream) {
    ACC_LIVE(a);
    if (!d_count) return fail(ICP4R_E_INVALID, "d_count is NULL");
    if (a->bound > 0 && !d_out) return fail(ICP4R_E_INVALID, "d_out is NULL");
    HIP_TRY(hipSetDevice(a->ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : a->ctx->stream;
    return run_filter(a, reinterpret_cast<float4*>(d_out), d_count, st);
}

int icp4r_voxel_acc_size(icp4r_voxel_acc* a, int64_t* voxels, int64_t* points) {
    ACC_LIVE(a);
    HIP_TRY(hipSetDevice(a->ctx->device));
    HIP_TRY(hipDeviceSynchronize());  // adds on a caller's stream too
    int rc;
    if ((rc = read_count(a, a->ctx->stream))) return rc;
    if (voxels) *voxels = a->bound;
    if (points) *points = (int64_t)a->points;
    return ICP4R_OK;
}

}  // extern "C"
