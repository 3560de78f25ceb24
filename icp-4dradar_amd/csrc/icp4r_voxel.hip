// icp4r_voxel.hip — voxel-grid downsampling for gfx950 (pcl::VoxelGrid<PointT>::applyFilter of PCL
// 1.8.1, the surround-map step of radar_odometry.cpp:426-429; include/icp4r/icp4r_voxel.h states the
// contract, DESIGN.md §6b.1 the pipeline).
//
// PCL sorts N (leaf index, point index) records and averages each run.  Here: the bounding box of the
// finite points by integer atomics (launch_finite_bbox) -> one thread turns it into min_b, div and the
// overflow flag on the device -> one key per point (the leaf index; INT32_MAX for a point that does not
// take part) -> the store's stable LSD radix sort of (key, i), which leaves each voxel's members
// adjacent and in input order -> segment heads compacted into a list of voxel starts -> the voxels
// that pass min_points_per_voxel compacted into (start, members) records, whose rank is the output
// position -> per voxel four sequential float chains over its members and one division.  Every step
// is a fixed-order computation on integers or a per-voxel sequential float sum: no float atomics, and
// the output bytes do not depend on the launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icp4r_voxel_common.hpp"

namespace icp4r {

constexpr int32_t kVxNoKey = INT32_MAX;   // a point that does not take part (idx <= INT32_MAX - 1)

// min_b, div and the overflow flag from the bounding box (one thread; voxel_grid_from_bbox states the
// rule, which the incremental grid shares).
__global__ void voxel_grid_kernel(const uint32_t* __restrict__ bbox, VoxelArgs a, VoxelGridDev* __restrict__ g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    *g = voxel_grid_from_bbox(bbox, a);
}

// (key, i) of every point.  Without a grid every key is kVxNoKey and nothing comes out.
__global__ __launch_bounds__(kVxWG) void voxel_keys_kernel(const float4* __restrict__ pts, int32_t n, VoxelArgs a,
                                                          const VoxelGridDev* __restrict__ g, int2* __restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * kVxWG + threadIdx.x;
    if (i >= n) return;
    int32_t key = kVxNoKey;
    const float4 p = pts[i];
    if (g->flag == 0 && finite_xyz(p)) {
        const int32_t i0 = (int32_t)(floorf(p.x * a.inv[0]) - (float)g->min_b[0]);
        const int32_t i1 = (int32_t)(floorf(p.y * a.inv[1]) - (float)g->min_b[1]);
        const int32_t i2 = (int32_t)(floorf(p.z * a.inv[2]) - (float)g->min_b[2]);
        key = i0 + i1 * g->div[0] + i2 * (g->div[0] * g->div[1]);
    }
    pairs[i] = make_int2(key, (int32_t)i);
}

// ---- two stable compactions (vx_compact, icp4r_voxel_common.hpp): keep(i) is the test, emit(i, rank)
// the ordered write.
struct HeadPred {  // the sorted positions where a run of equal keys starts (the kVxNoKey run included)
    const int2* pairs;
    int32_t n;
    int32_t* heads;
    __device__ __forceinline__ int32_t size() const { return n; }
    __device__ __forceinline__ bool keep(int64_t t) const { return t == 0 || pairs[t - 1].x != pairs[t].x; }
    __device__ __forceinline__ void emit(int64_t t, int32_t rank) const { heads[rank] = (int32_t)t; }
};

struct VoxelPred {  // the runs that are voxels with enough members; rank = the output position
    const int2* pairs;
    int32_t n;
    const int32_t* heads;
    const int32_t* nheads;  // device: the number of runs
    uint32_t min_pts;
    int2* kept;             // (first sorted position, members)
    __device__ __forceinline__ int32_t size() const { return *nheads; }
    __device__ __forceinline__ int32_t members(int64_t r) const {
        return (r + 1 < *nheads ? heads[r + 1] : n) - heads[r];
    }
    __device__ __forceinline__ bool keep(int64_t r) const {
        return pairs[heads[r]].x != kVxNoKey && (uint32_t)members(r) >= min_pts;
    }
    __device__ __forceinline__ void emit(int64_t r, int32_t rank) const { kept[rank] = make_int2(heads[r], members(r)); }
};

// Centroids: a lane per kept voxel.  A voxel of at most kVxShort members is walked by its lane, four
// gathers ahead of the four dependent adds.  The longer ones are then taken one at a time by the whole
// wave: 64 members gathered at once (the next 64 already in flight), then added in member order by
// reading lane after lane, so a voxel costs its own length and the sums are the same sequential
// chains from +0.0f either way.  Thread 0 also stores the count (-1: grid overflow).
__global__ __launch_bounds__(kVxWG) void voxel_centroid_kernel(const float4* __restrict__ pts,
                                                              const int2* __restrict__ pairs,
                                                              const int2* __restrict__ kept,
                                                              const int32_t* __restrict__ nkept,
                                                              const VoxelGridDev* __restrict__ g, int32_t all_data,
                                                              float4* __restrict__ out, int32_t* __restrict__ count) {
    const int32_t K = *nkept;
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * kVxWG + threadIdx.x;
    if (v == 0) *count = g->flag < 0 ? -1 : K;
    if (v - lane >= K) return;  // (the whole wave)
    const bool have = v < K;
    const int2 sv = have ? kept[v] : make_int2(0, 0);
    const int32_t start = sv.x, m = sv.y;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
    if (have && m <= kVxShort) {
        for (int32_t u = 0; u < m; u += 4) {
            float4 p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = pts[pairs[start + min(u + j, m - 1)].y];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (u + j < m) {
                    sx += p[j].x;
                    sy += p[j].y;
                    sz += p[j].z;
                    sw += p[j].w;
                }
        }
    }
    uint64_t todo = __ballot(have && m > kVxShort);
    while (todo) {
        const int owner = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int32_t st = __builtin_amdgcn_readlane(start, owner), mm = __builtin_amdgcn_readlane(m, owner);
        float cx = 0.0f, cy = 0.0f, cz = 0.0f, cw = 0.0f;
        float4 next = make_float4(0.f, 0.f, 0.f, 0.f);  // (lanes past the voxel's end: never read)
        if (lane < mm) next = pts[pairs[st + lane].y];
        for (int64_t c = 0; c < mm; c += 64) {
            const float4 cur = next;
            if (c + 64 + lane < mm) next = pts[pairs[st + c + 64 + lane].y];
            const int cnt = (int)(mm - c < 64 ? mm - c : 64);
            for (int j = 0; j < cnt; ++j) {
                cx += vx_lane(cur.x, j);
                cy += vx_lane(cur.y, j);
                cz += vx_lane(cur.z, j);
                cw += vx_lane(cur.w, j);
            }
        }
        if (lane == owner) sx = cx, sy = cy, sz = cz, sw = cw;
    }
    if (have) {
        const float fm = (float)m;
        out[v] = make_float4(__fdiv_rn(sx, fm), __fdiv_rn(sy, fm), __fdiv_rn(sz, fm), all_data ? __fdiv_rn(sw, fm) : 0.0f);
    }
}

static size_t vx_align(size_t x) { return (x + 255) & ~(size_t)255; }

VoxelLayout voxel_layout(int64_t n) {
    VoxelLayout L;
    const size_t m = (size_t)(n > 0 ? n : 1);
    const size_t nblk = 256 * (size_t)sector_blocks((int64_t)m);  // the radix sort's counts; the compactions need fewer
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += vx_align(bytes);
        return at;
    };
    L.bbox = take(6 * sizeof(uint32_t));
    L.grid = take(sizeof(VoxelGridDev));
    L.tot = take(4 * sizeof(int32_t));  // runs, kept voxels, the radix scans' total
    L.pa = take(m * sizeof(int2));
    L.pb = take(m * sizeof(int2));
    L.counts = take(nblk * sizeof(int32_t));
    L.offsets = take(nblk * sizeof(int32_t));
    L.heads = take(m * sizeof(int32_t));
    L.kept = take(m * sizeof(int2));
    L.bytes = o;
    return L;
}

hipError_t launch_voxel_grid(const float4* pts, int64_t n, const VoxelArgs& a, void* work, hipStream_t st) {
    const VoxelLayout L = voxel_layout(n);
    char* w = static_cast<char*>(work);
    uint32_t* bbox = reinterpret_cast<uint32_t*>(w + L.bbox);
    hipError_t e;
    if ((e = launch_finite_bbox(pts, n, bbox, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(voxel_grid_kernel, dim3(1), dim3(64), 0, st, bbox, a, reinterpret_cast<VoxelGridDev*>(w + L.grid));
    return hipGetLastError();
}

hipError_t launch_voxel_filter(const float4* pts, int64_t n, const VoxelArgs& a, int bits, void* work, float4* out,
                               int32_t* count, hipStream_t st) {
    const VoxelLayout L = voxel_layout(n);
    char* w = static_cast<char*>(work);
    const VoxelGridDev* g = reinterpret_cast<const VoxelGridDev*>(w + L.grid);
    int32_t* tot = reinterpret_cast<int32_t*>(w + L.tot);
    int32_t* counts = reinterpret_cast<int32_t*>(w + L.counts);
    int32_t* offsets = reinterpret_cast<int32_t*>(w + L.offsets);
    int32_t* heads = reinterpret_cast<int32_t*>(w + L.heads);
    int2* kept = reinterpret_cast<int2*>(w + L.kept);
    int2* pa = reinterpret_cast<int2*>(w + L.pa);
    const int32_t n32 = (int32_t)n;
    hipLaunchKernelGGL(voxel_keys_kernel, dim3((unsigned)((n + kVxWG - 1) / kVxWG)), dim3(kVxWG), 0, st, pts, n32, a, g, pa);
    const int2* sorted = launch_radix_sort(pa, reinterpret_cast<int2*>(w + L.pb), n32, bits, counts, offsets, tot + 2, st);
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = vx_compact(HeadPred{sorted, n32, heads}, n, counts, offsets, tot, st)) != hipSuccess) return e;
    if ((e = vx_compact(VoxelPred{sorted, n32, heads, tot, a.min_pts, kept}, n, counts, offsets, tot + 1, st)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(voxel_centroid_kernel, dim3((unsigned)((n + kVxWG - 1) / kVxWG)), dim3(kVxWG), 0, st, pts, sorted, kept,
                       tot + 1, g, a.all_data, out, count);
    return hipGetLastError();
}

}  // namespace icp4r
