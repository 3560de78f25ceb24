// icp4r_map.cpp — C ABI of the scan-to-map store (include/icp4r/icp4r_map.h).
//
// Host-side mirror of the reference's ikd-Tree (radar_odometry.cpp:92, :347-348, :382-396, and the
// map-maintenance calls of ikd_Tree.h:238-245): a dense float4 store in HBM, in insertion order, that
// grows by doubling.  Sector_Search, Box_Search, Radius_Search and Delete_Point_Boxes are one device
// stream compaction with the keep test as a parameter, the downsampling Add_Points a per-cell
// reduction plus one compaction (icp4r_map.hip); the two edits compact into a second buffer of the
// store's capacity and swap.  Nearest_Search alone has an index behind it: a snapshot of the store in
// Morton order under a 64-ary tree of boxes (icp4r_map_knn.hip), built by the first search that needs
// it, kept across plain appends (the appended tail is swept by brute force) and dropped by whatever
// reorders or moves the store.  No CPU fallback: every entry fails with ICP4R_E_HIP if the device
// path cannot run.
//
// Lifetime: a context keeps a list of its maps.  icp4r_destroy frees the device side of each and
// detaches it (ctx = nullptr); a detached map answers every entry with ICP4R_E_INVALID without
// touching HIP, and icp4r_map_destroy only deletes the host struct.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "icp4r/icp4r_map.h"
#include "icp4r_host.hpp"
#include "icp4r_internal.hpp"

using icp4r_host::check_cloud;
using icp4r_host::DevBuf;
using icp4r_host::EventPair;
using icp4r_host::fail;
using icp4r_host::pack_host;

struct icp4r_map {
    icp4r_ctx* ctx = nullptr;  // nullptr: detached (the context was destroyed)
    float4* pts = nullptr;     // [cap] insertion order
    float4* alt = nullptr;     // [cap] the edits' second buffer (allocated at the first edit), or nullptr
    int64_t n = 0, cap = 0;
    DevBuf staging, counts, offsets, total, out, boxes, ds;
    // the k-NN index (icp4r_map_knn.hip): a snapshot of pts[0, indexed); [indexed, n) is the tail the
    // search sweeps.  Anything that reorders or moves the store drops it (index_valid = false).
    DevBuf knn_index, knn_scratch, knn_q, knn_pts, knn_dist, knn_idx, knn_found;
    bool index_valid = false;
    int64_t indexed = 0;
    int32_t index_builds = 0;
    std::vector<EventPair> events;
    size_t used = 0;
};

namespace {

#define MAP_LIVE(m)                                                                        \
    do {                                                                                   \
        if (!(m)->ctx) return fail(ICP4R_E_INVALID, "the map's context was destroyed");    \
    } while (0)

// Frees everything the map holds on the device (the context's device is current).
void release_device(icp4r_map* m) {
    if (m->pts) (void)hipFree(m->pts);
    if (m->alt) (void)hipFree(m->alt);
    m->pts = m->alt = nullptr;
    for (DevBuf* b : {&m->staging, &m->counts, &m->offsets, &m->total, &m->out, &m->boxes, &m->ds, &m->knn_index,
                      &m->knn_scratch, &m->knn_q, &m->knn_pts, &m->knn_dist, &m->knn_idx, &m->knn_found})
        b->release();
    m->index_valid = false;
    m->indexed = 0;
    for (auto& e : m->events) {
        (void)hipEventDestroy(e.start);
        (void)hipEventDestroy(e.stop);
    }
    m->events.clear();
    m->used = 0;
    m->n = m->cap = 0;
}

// Grow the store to hold `need` points, keeping the first map->n (doubling: amortised O(1) append).
int grow(icp4r_map* m, int64_t need) {
    if (need <= m->cap) return ICP4R_OK;
    int64_t cap = m->cap > 0 ? m->cap : (int64_t)1 << 16;
    while (cap < need) cap *= 2;
    float4* p = nullptr;
    HIP_TRY(hipMalloc(&p, (size_t)cap * sizeof(float4)));
    if (m->n > 0) {
        hipError_t e = hipMemcpyAsync(p, m->pts, (size_t)m->n * sizeof(float4), hipMemcpyDeviceToDevice, m->ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(m->ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return fail(ICP4R_E_HIP, "map grow: %s", hipGetErrorString(e));
        }
    }
    if (m->pts) HIP_TRY(hipFree(m->pts));
    m->pts = p;
    m->cap = cap;
    m->index_valid = false;  // growth moves the store
    if (m->alt) {  // the second buffer follows the capacity: allocated again at the next edit
        float4* a = m->alt;
        m->alt = nullptr;
        HIP_TRY(hipFree(a));
    }
    return ICP4R_OK;
}

// The edits' second buffer, of the store's capacity (at least one allocation's worth).
int ensure_alt(icp4r_map* m) {
    int rc;
    if (m->cap == 0 && (rc = grow(m, 1))) return rc;
    if (!m->alt) HIP_TRY(hipMalloc(&m->alt, (size_t)m->cap * sizeof(float4)));
    return ICP4R_OK;
}

// Upload n host points (any stride) as float4 into the staging buffer.
int stage(icp4r_map* m, const float* pts, int64_t n, int32_t stride, std::vector<float>& h) {
    pack_host(pts, n, stride, h);
    HIP_TRY(m->staging.ensure((size_t)(n > 0 ? n : 1) * sizeof(float4)));
    if (n > 0) HIP_TRY(hipMemcpyAsync(m->staging.p, h.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, m->ctx->stream));
    return ICP4R_OK;
}

int ensure_blocks(icp4r_map* m, int64_t n) {
    const int64_t nblk = icp4r::sector_blocks(n);
    HIP_TRY(m->counts.ensure((size_t)(nblk > 0 ? nblk : 1) * sizeof(int32_t)));
    HIP_TRY(m->offsets.ensure((size_t)(nblk > 0 ? nblk : 1) * sizeof(int32_t)));
    return ICP4R_OK;
}

// Runs `launch` (stream -> hipError_t) between a pair of the map's timing events.
template <class Launch>
int timed(icp4r_map* m, hipStream_t st, Launch launch) {
    if (m->used == m->events.size()) {
        EventPair e;
        HIP_TRY(hipEventCreate(&e.start));
        HIP_TRY(hipEventCreate(&e.stop));
        m->events.push_back(e);
    }
    EventPair& ev = m->events[m->used++];
    HIP_TRY(hipEventRecord(ev.start, st));
    HIP_TRY(launch(st));
    HIP_TRY(hipEventRecord(ev.stop, st));
    return ICP4R_OK;
}

// The three filters, by their arguments: each launches the compaction of the store into out / count.
struct SectorQuery {
    const float* center;
    float radius, heading;
};
struct BoxQuery {
    const float* box6;
};
struct RadiusQuery {
    const float* center;
    float radius;
};

int check_query(const SectorQuery& q) {
    if (!q.center) return fail(ICP4R_E_INVALID, "center is NULL");
    if (!(q.radius >= 0.0f)) return fail(ICP4R_E_INVALID, "radius must be >= 0");
    return ICP4R_OK;
}
int check_query(const BoxQuery& q) { return q.box6 ? ICP4R_OK : fail(ICP4R_E_INVALID, "box is NULL"); }
int check_query(const RadiusQuery& q) {
    if (!q.center) return fail(ICP4R_E_INVALID, "center is NULL");
    if (!(q.radius >= 0.0f)) return fail(ICP4R_E_INVALID, "radius must be >= 0");
    return ICP4R_OK;
}

hipError_t launch_query(icp4r_map* m, const SectorQuery& q, float4* out, int32_t* count, hipStream_t st) {
    icp4r::SectorArgs a;
    a.cx = q.center[0];
    a.cy = q.center[1];
    a.cz = q.center[2];
    a.radius = q.radius;
    a.heading = q.heading;
    return icp4r::launch_sector(m->pts, m->n, a, static_cast<int32_t*>(m->counts.p), static_cast<int32_t*>(m->offsets.p),
                                count, out, st);
}
hipError_t launch_query(icp4r_map* m, const BoxQuery& q, float4* out, int32_t* count, hipStream_t st) {
    icp4r::BoxArgs b;
    memcpy(b.lo, q.box6, sizeof(b.lo));
    memcpy(b.hi, q.box6 + 3, sizeof(b.hi));
    return icp4r::launch_box(m->pts, m->n, b, static_cast<int32_t*>(m->counts.p), static_cast<int32_t*>(m->offsets.p),
                             count, out, st);
}
hipError_t launch_query(icp4r_map* m, const RadiusQuery& q, float4* out, int32_t* count, hipStream_t st) {
    return icp4r::launch_radius(m->pts, m->n, q.center, q.radius, static_cast<int32_t*>(m->counts.p),
                                static_cast<int32_t*>(m->offsets.p), count, out, st);
}

template <class Query>
int query_launch(icp4r_map* m, const Query& q, float4* out, int32_t* count, hipStream_t st) {
    int rc;
    if ((rc = check_query(q))) return rc;
    if ((rc = ensure_blocks(m, m->n))) return rc;
    return timed(m, st, [&](hipStream_t s) { return launch_query(m, q, out, count, s); });
}

// The host variants: the kept points to host memory; *out_n is set even when they do not fit.
template <class Query>
int query_host(icp4r_map* m, const Query& q, float* out, int64_t out_cap, int64_t* out_n, const char* what) {
    if (!m || !out_n || (out_cap > 0 && !out)) return fail(ICP4R_E_INVALID, "NULL argument");
    MAP_LIVE(m);
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = m->ctx->stream;
    HIP_TRY(m->out.ensure((size_t)(m->n > 0 ? m->n : 1) * sizeof(float4)));
    HIP_TRY(m->total.ensure(sizeof(int32_t)));
    int rc;
    if ((rc = query_launch(m, q, static_cast<float4*>(m->out.p), static_cast<int32_t*>(m->total.p), st))) return rc;
    int32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, m->total.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_n = cnt;
    if (cnt > out_cap) return fail(ICP4R_E_TOO_LARGE, "%s kept %d points, out_cap %lld", what, cnt, (long long)out_cap);
    if (cnt > 0) {
        HIP_TRY(hipMemcpyAsync(out, m->out.p, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return ICP4R_OK;
}

template <class Query>
int query_device(icp4r_map* m, const Query& q, float* d_out, int32_t* d_count, void* hip_stream) {
    if (!m || !d_out || !d_count) return fail(ICP4R_E_INVALID, "NULL argument");
    MAP_LIVE(m);
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : m->ctx->stream;
    return query_launch(m, q, reinterpret_cast<float4*>(d_out), d_count, st);
}

// After an edit compacted the new store into m->alt and its size into m->total: adopt it.
int adopt_alt(icp4r_map* m, int64_t* new_n) {
    int32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, m->total.p, sizeof(cnt), hipMemcpyDeviceToHost, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    std::swap(m->pts, m->alt);
    m->index_valid = false;  // the edit moved the survivors
    *new_n = cnt;
    return ICP4R_OK;
}

// ---- k-NN (icp4r_map_knn.hip)
// The tail a search still sweeps by brute force instead of rebuilding the index: with a scan of S
// points appended per frame, a rebuild every T points costs build * S / T + sweep * T / 2 per frame,
// least at T = sqrt(2 * build * S / sweep) — about 11 k points on the 65,536-point map and 49 k on
// the 9.83 M-point one by the first measurements.
constexpr int64_t kKnnTailMin = 16384;
// Maps below this size are searched without an index unless ICP4R_MAP_KNN_INDEX asks for one: for a
// 6,554-query scan the brute sweep was the faster at 1,024 points and the slower at 4,096 (§6b).
constexpr int64_t kKnnBruteBelow = 1024;

int64_t knn_tail_limit(int64_t indexed) { return std::max(kKnnTailMin, indexed / 256); }

bool index_current(const icp4r_map* m) { return m->n == 0 || (m->index_valid && m->indexed == m->n); }

// Builds the index of the whole store on the context's stream and waits for it: a search on any
// stream may follow.
int index_rebuild(icp4r_map* m) {
    if (m->n >= ((int64_t)1 << 31)) return fail(ICP4R_E_TOO_LARGE, "k-NN index: %lld points", (long long)m->n);
    hipStream_t st = m->ctx->stream;
    m->index_valid = false;
    HIP_TRY(m->knn_index.ensure(icp4r::knn_layout(m->n).bytes));
    HIP_TRY(m->knn_scratch.ensure(icp4r::knn_sort_layout(m->n).bytes));
    int rc;
    if ((rc = timed(m, st, [&](hipStream_t s) {
            return icp4r::launch_knn_index(m->pts, m->n, m->knn_index.p, m->knn_scratch.p, s);
        })))
        return rc;
    HIP_TRY(hipStreamSynchronize(st));
    m->index_valid = true;
    m->indexed = m->n;
    ++m->index_builds;
    return ICP4R_OK;
}

int knn_check(const icp4r_map* m, const float* queries, int64_t nq, int32_t k, int32_t flags) {
    if (!m) return fail(ICP4R_E_INVALID, "map is NULL");
    MAP_LIVE(m);
    if (flags & ~(ICP4R_MAP_KNN_BRUTE | ICP4R_MAP_KNN_INDEX)) return fail(ICP4R_E_INVALID, "unknown flag bits 0x%x", flags);
    if ((flags & ICP4R_MAP_KNN_BRUTE) && (flags & ICP4R_MAP_KNN_INDEX))
        return fail(ICP4R_E_INVALID, "ICP4R_MAP_KNN_BRUTE and ICP4R_MAP_KNN_INDEX exclude each other");
    if (k < 1 || k > ICP4R_MAP_KNN_MAX_K) return fail(ICP4R_E_INVALID, "k must be in [1, %d]", ICP4R_MAP_KNN_MAX_K);
    if (nq < 0) return fail(ICP4R_E_INVALID, "nq must be >= 0");
    if (nq > 0 && !queries) return fail(ICP4R_E_INVALID, "queries is NULL");
    if (nq >= ((int64_t)1 << 31) / ICP4R_MAP_KNN_MAX_K) return fail(ICP4R_E_TOO_LARGE, "%lld queries", (long long)nq);
    if (m->n >= ((int64_t)1 << 31)) return fail(ICP4R_E_TOO_LARGE, "nearest search: %lld stored points", (long long)m->n);
    return ICP4R_OK;
}

// The search of nq device queries (float4) on stream st; the index is brought up to date first if the
// path needs it.
int knn_launch(icp4r_map* m, const float4* d_q, int64_t nq, int32_t k, double max_dist, int32_t flags, float4* d_pts,
               float* d_dist, int32_t* d_idx, int32_t* d_found, hipStream_t st) {
    const bool brute = (flags & ICP4R_MAP_KNN_BRUTE) || (!(flags & ICP4R_MAP_KNN_INDEX) && m->n < kKnnBruteBelow);
    int rc;
    icp4r::KnnSearch s = {};
    s.pts = m->pts;
    s.n = m->n;
    s.tail0 = 0;
    if (!brute && m->n > 0) {
        if (!m->index_valid || m->n - m->indexed > knn_tail_limit(m->indexed))
            if ((rc = index_rebuild(m))) return rc;
        if (m->indexed > 0) s.ix = icp4r::knn_view(m->knn_index.p, m->indexed);
        s.tail0 = m->indexed;
        HIP_TRY(m->knn_scratch.ensure(icp4r::knn_sort_layout(std::max(nq, m->indexed)).bytes));
    }
    s.q = d_q;
    s.nq = (int32_t)nq;
    s.k = k;
    // the reference's test: (double)d <= max_dist * max_dist (a NaN finds nothing); the pruning bound
    // is that product rounded up to float
    s.md2 = max_dist * max_dist;
    if (s.md2 != s.md2) {
        s.md2 = -1.0;
        s.bound = -INFINITY;
    } else {
        s.bound = (float)s.md2;
        if ((double)s.bound < s.md2) s.bound = nextafterf(s.bound, INFINITY);
    }
    s.pout = d_pts;
    s.dout = d_dist;
    s.iout = d_idx;
    s.fout = d_found;
    return timed(m, st, [&](hipStream_t t) { return icp4r::launch_knn_search(s, m->knn_scratch.p, t); });
}

}  // namespace

namespace icp4r_host {

void map_detach(icp4r_map* m) {
    release_device(m);
    m->ctx = nullptr;
}

icp4r_ctx* map_context(const icp4r_map* m) { return m->ctx; }

}  // namespace icp4r_host

extern "C" {

int icp4r_map_create(icp4r_ctx* ctx, icp4r_map** out) {
    if (!ctx || !out) return fail(ICP4R_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (ctx->device < 0) return fail(ICP4R_E_INVALID, "icp4r_map_create: a context without a device");
    icp4r_map* m = new icp4r_map();
    m->ctx = ctx;
    ctx->maps.push_back(m);
    *out = m;
    return ICP4R_OK;
}

int icp4r_map_destroy(icp4r_map* m) {
    if (!m) return ICP4R_OK;
    if (m->ctx) {
        auto& maps = m->ctx->maps;
        maps.erase(std::remove(maps.begin(), maps.end(), m), maps.end());
        (void)hipSetDevice(m->ctx->device);
        (void)hipStreamSynchronize(m->ctx->stream);
        release_device(m);
    }
    delete m;
    return ICP4R_OK;
}

int icp4r_map_add_points(icp4r_map* m, const float* pts, int64_t n, int32_t stride_bytes, int32_t downsample_on) {
    if (!m) return fail(ICP4R_E_INVALID, "map is NULL");
    MAP_LIVE(m);
    if (downsample_on)
        return fail(ICP4R_E_INVALID, "Add_Points with downsample_on carries no box length: use icp4r_map_add_points_downsample");
    int rc;
    if ((rc = check_cloud(pts, n, stride_bytes, "points"))) return rc;
    if (n == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    if ((rc = grow(m, m->n + n))) return rc;
    std::vector<float> h;
    pack_host(pts, n, stride_bytes, h);
    HIP_TRY(hipMemcpyAsync(m->pts + m->n, h.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));  // h goes out of scope
    m->n += n;
    return ICP4R_OK;
}

int icp4r_map_add_points_downsample(icp4r_map* m, const float* pts, int64_t n, int32_t stride_bytes, float box_length,
                                    int64_t* counter) {
    if (!m || !counter) return fail(ICP4R_E_INVALID, "map/counter is NULL");
    MAP_LIVE(m);
    if (!(box_length > 0.0f) || !isfinite(box_length)) return fail(ICP4R_E_INVALID, "box_length must be finite and > 0");
    int rc;
    if ((rc = check_cloud(pts, n, stride_bytes, "points"))) return rc;
    *counter = 0;
    if (n == 0) return ICP4R_OK;
    if (m->n + n >= ((int64_t)1 << 30)) return fail(ICP4R_E_TOO_LARGE, "downsampled insert: %lld points", (long long)(m->n + n));
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = m->ctx->stream;
    if ((rc = grow(m, m->n + n))) return rc;  // the new store holds at most every stored and every arriving point
    if ((rc = ensure_alt(m))) return rc;
    std::vector<float> h;
    if ((rc = stage(m, pts, n, stride_bytes, h))) return rc;
    HIP_TRY(m->ds.ensure(icp4r::ds_layout(m->n, n).bytes));
    HIP_TRY(m->total.ensure(sizeof(int32_t)));
    if ((rc = ensure_blocks(m, m->n + n))) return rc;
    int32_t* d_counter = nullptr;
    if ((rc = timed(m, st, [&](hipStream_t s) {
            return icp4r::launch_downsample(m->pts, m->n, static_cast<const float4*>(m->staging.p), n, box_length, m->ds.p,
                                            static_cast<int32_t*>(m->counts.p), static_cast<int32_t*>(m->offsets.p),
                                            static_cast<int32_t*>(m->total.p), m->alt, &d_counter, s);
        })))
        return rc;
    int32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, d_counter, sizeof(cnt), hipMemcpyDeviceToHost, st));
    if ((rc = adopt_alt(m, &m->n))) return rc;  // synchronises: h and cnt are done with
    *counter = cnt;
    return ICP4R_OK;
}

int icp4r_map_delete_boxes(icp4r_map* m, const float* boxes, int32_t nb, int64_t* deleted) {
    if (!m || !deleted || (nb > 0 && !boxes)) return fail(ICP4R_E_INVALID, "NULL argument");
    MAP_LIVE(m);
    if (nb < 0) return fail(ICP4R_E_INVALID, "nb must be >= 0");
    *deleted = 0;
    if (nb == 0 || m->n == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = m->ctx->stream;
    int rc;
    if ((rc = ensure_alt(m))) return rc;
    HIP_TRY(m->boxes.ensure((size_t)nb * 6 * sizeof(float)));
    HIP_TRY(m->total.ensure(sizeof(int32_t)));
    if ((rc = ensure_blocks(m, m->n))) return rc;
    HIP_TRY(hipMemcpyAsync(m->boxes.p, boxes, (size_t)nb * 6 * sizeof(float), hipMemcpyHostToDevice, st));
    if ((rc = timed(m, st, [&](hipStream_t s) {
            return icp4r::launch_outside_boxes(m->pts, m->n, static_cast<const float*>(m->boxes.p), nb,
                                               static_cast<int32_t*>(m->counts.p), static_cast<int32_t*>(m->offsets.p),
                                               static_cast<int32_t*>(m->total.p), m->alt, s);
        })))
        return rc;
    int64_t kept = 0;
    if ((rc = adopt_alt(m, &kept))) return rc;
    *deleted = m->n - kept;
    m->n = kept;
    return ICP4R_OK;
}

int icp4r_map_build(icp4r_map* m, const float* pts, int64_t n, int32_t stride_bytes) {
    if (!m) return fail(ICP4R_E_INVALID, "map is NULL");
    MAP_LIVE(m);
    int rc;
    if ((rc = check_cloud(pts, n, stride_bytes, "points"))) return rc;
    m->n = 0;  // KD_TREE::Build replaces the tree
    m->index_valid = false;
    return icp4r_map_add_points(m, pts, n, stride_bytes, 0);
}

int icp4r_map_add_scan(icp4r_map* m, const float* scan, int64_t n, int32_t stride_bytes, const double* R,
                       const double* t, float* world_out) {
    if (!m || !R || !t) return fail(ICP4R_E_INVALID, "map/R/t is NULL");
    MAP_LIVE(m);
    int rc;
    if ((rc = check_cloud(scan, n, stride_bytes, "scan"))) return rc;
    if (n == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    if ((rc = grow(m, m->n + n))) return rc;
    std::vector<float> h;
    if ((rc = stage(m, scan, n, stride_bytes, h))) return rc;
    icp4r::Mat3x4d M;
    memcpy(M.R, R, sizeof(M.R));
    memcpy(M.t, t, sizeof(M.t));
    HIP_TRY(icp4r::launch_associate(static_cast<const float4*>(m->staging.p), n, M, m->pts + m->n, m->ctx->stream));
    if (world_out)
        HIP_TRY(hipMemcpyAsync(world_out, m->pts + m->n, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    m->n += n;
    return ICP4R_OK;
}

int icp4r_map_size(const icp4r_map* m, int64_t* n) {
    if (!m || !n) return fail(ICP4R_E_INVALID, "NULL argument");
    MAP_LIVE(m);
    *n = m->n;
    return ICP4R_OK;
}

int icp4r_map_sector_search(icp4r_map* m, const float* center, float radius, float heading_deg, float* out,
                            int64_t out_cap, int64_t* out_n) {
    return query_host(m, SectorQuery{center, radius, heading_deg}, out, out_cap, out_n, "sector search");
}

int icp4r_map_sector_search_device(icp4r_map* m, const float* center, float radius, float heading_deg, float* d_out,
                                   int32_t* d_count, void* hip_stream) {
    return query_device(m, SectorQuery{center, radius, heading_deg}, d_out, d_count, hip_stream);
}

int icp4r_map_box_search(icp4r_map* m, const float* box6, float* out, int64_t out_cap, int64_t* out_n) {
    return query_host(m, BoxQuery{box6}, out, out_cap, out_n, "box search");
}

int icp4r_map_box_search_device(icp4r_map* m, const float* box6, float* d_out, int32_t* d_count, void* hip_stream) {
    return query_device(m, BoxQuery{box6}, d_out, d_count, hip_stream);
}

int icp4r_map_radius_search(icp4r_map* m, const float* center, float radius, float* out, int64_t out_cap,
                            int64_t* out_n) {
    return query_host(m, RadiusQuery{center, radius}, out, out_cap, out_n, "radius search");
}

int icp4r_map_radius_search_device(icp4r_map* m, const float* center, float radius, float* d_out, int32_t* d_count,
                                   void* hip_stream) {
    return query_device(m, RadiusQuery{center, radius}, d_out, d_count, hip_stream);
}

int icp4r_map_nearest_search_device(icp4r_map* m, const float* d_queries, int64_t nq, int32_t k, double max_dist,
                                    int32_t flags, float* d_points, float* d_dist, int32_t* d_index, int32_t* d_found,
                                    void* hip_stream) {
    int rc;
    if ((rc = knn_check(m, d_queries, nq, k, flags))) return rc;
    if (nq == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : m->ctx->stream;
    return knn_launch(m, reinterpret_cast<const float4*>(d_queries), nq, k, max_dist, flags,
                      reinterpret_cast<float4*>(d_points), d_dist, d_index, d_found, st);
}

int icp4r_map_nearest_search(icp4r_map* m, const float* queries, int64_t nq, int32_t stride_bytes, int32_t k,
                             double max_dist, int32_t flags, float* points_out, float* dist_out, int32_t* index_out,
                             int32_t* found_out) {
    int rc;
    if ((rc = knn_check(m, queries, nq, k, flags))) return rc;
    if (stride_bytes < 12 || stride_bytes % 4)
        return fail(ICP4R_E_INVALID, "queries: stride %d bytes (need >= 12, multiple of 4)", stride_bytes);
    if (nq == 0) return ICP4R_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = m->ctx->stream;
    const size_t rows = (size_t)nq * (size_t)k;
    std::vector<float> h;
    pack_host(queries, nq, stride_bytes, h);
    HIP_TRY(m->knn_q.ensure((size_t)nq * sizeof(float4)));
    if (points_out) HIP_TRY(m->knn_pts.ensure(rows * sizeof(float4)));
    if (dist_out) HIP_TRY(m->knn_dist.ensure(rows * sizeof(float)));
    if (index_out) HIP_TRY(m->knn_idx.ensure(rows * sizeof(int32_t)));
    if (found_out) HIP_TRY(m->knn_found.ensure((size_t)nq * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(m->knn_q.p, h.data(), (size_t)nq * sizeof(float4), hipMemcpyHostToDevice, st));
    if ((rc = knn_launch(m, static_cast<const float4*>(m->knn_q.p), nq, k, max_dist, flags,
                         points_out ? static_cast<float4*>(m->knn_pts.p) : nullptr,
                         dist_out ? static_cast<float*>(m->knn_dist.p) : nullptr,
                         index_out ? static_cast<int32_t*>(m->knn_idx.p) : nullptr,
                         found_out ? static_cast<int32_t*>(m->knn_found.p) : nullptr, st))) {
        (void)hipStreamSynchronize(st);  // h goes out of scope
        return rc;
    }
    if (points_out) HIP_TRY(hipMemcpyAsync(points_out, m->knn_pts.p, rows * sizeof(float4), hipMemcpyDeviceToHost, st));
    if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out, m->knn_dist.p, rows * sizeof(float), hipMemcpyDeviceToHost, st));
    if (index_out) HIP_TRY(hipMemcpyAsync(index_out, m->knn_idx.p, rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (found_out) HIP_TRY(hipMemcpyAsync(found_out, m->knn_found.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ICP4R_OK;
}

int icp4r_map_index_build(icp4r_map* m) {
    if (!m) return fail(ICP4R_E_INVALID, "map is NULL");
    MAP_LIVE(m);
    if (index_current(m)) return ICP4R_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    return index_rebuild(m);
}

int icp4r_map_index_stats(const icp4r_map* m, int64_t* indexed, int64_t* tail, int64_t* tail_limit, int32_t* builds) {
    if (!m) return fail(ICP4R_E_INVALID, "map is NULL");
    MAP_LIVE(m);
    const int64_t ix = m->index_valid ? m->indexed : 0;
    if (indexed) *indexed = ix;
    if (tail) *tail = m->n - ix;
    if (tail_limit) *tail_limit = knn_tail_limit(ix);
    if (builds) *builds = m->index_builds;
    return ICP4R_OK;
}

int icp4r_map_points_device(icp4r_map* m, const float** d_points, int64_t* n) {
    if (!m || !d_points || !n) return fail(ICP4R_E_INVALID, "NULL argument");
    MAP_LIVE(m);
    *d_points = reinterpret_cast<const float*>(m->pts);
    *n = m->n;
    return ICP4R_OK;
}

int icp4r_map_time_ms(icp4r_map* m, double* avg_ms, int32_t* calls) {
    if (!m || !avg_ms) return fail(ICP4R_E_INVALID, "NULL argument");
    MAP_LIVE(m);
    HIP_TRY(hipSetDevice(m->ctx->device));
    double tot = 0.0;
    for (size_t i = 0; i < m->used; ++i) {
        HIP_TRY(hipEventSynchronize(m->events[i].stop));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, m->events[i].start, m->events[i].stop));
        tot += ms;
    }
    *avg_ms = m->used ? tot / (double)m->used : 0.0;
    if (calls) *calls = (int32_t)m->used;
    return ICP4R_OK;
}

int icp4r_map_time_reset(icp4r_map* m) {
    if (!m) return fail(ICP4R_E_INVALID, "map is NULL");
    MAP_LIVE(m);
    m->used = 0;
    return ICP4R_OK;
}

}  // extern "C"
