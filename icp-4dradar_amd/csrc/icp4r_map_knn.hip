// icp4r_map_knn.hip — the scan-to-map store's index and batched exact k-NN for gfx950
// (KD_TREE::Nearest_Search, ikd_Tree.cpp:368-398 and :877-1021; include/icp4r/icp4r_map.h).
//
// The index is a snapshot of the store: bounding box of the finite points -> a 30-bit Morton key per
// point (11 bits for x and y, 8 for z: radar maps are flat) -> the store's stable radix sort of
// (key, position) -> a float4 copy in that order -> boxes of the leaves (16 consecutive positions) and
// of every 64 consecutive nodes of the level below.  The search sorts its queries by the same key, so
// a wave holds 16 neighbouring queries with 4 lanes each, and walks the 64-ary box tree nearest first
// under the wave's bounds: one lane-parallel box load and one ballot per node.  What was appended
// since the snapshot, or with ICP4R_MAP_KNN_BRUTE the whole store, is swept through LDS tiles by the
// same kernel.  Keys are (d² bits << 32 | position): the k smallest are the contract's answer.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icp4r_device.hpp"
#include "icp4r_internal.hpp"

namespace icp4r {

constexpr int kKnnWG = 256;
constexpr int kKnnL = 4;                // lanes per query
constexpr int kKnnQW = kKnnWG / kKnnL;  // queries per workgroup (16 per wave)
constexpr int kKnnTile = 1024;          // points per LDS tile of the sweep
constexpr uint32_t kKnnKeyBits = 31;    // 30 Morton bits; bit 30: a non-finite point, sorted last
static_assert(kKnnLeaf % kKnnL == 0 && kKnnFan == 64, "a node's children are one wave's lanes");

// The key grid of a bounding box: 2047 / 2047 / 255 cells along x / y / z; a zero, infinite or
// undefined extent gives scale 0, so every point of a flat, single-point or empty cloud has cell 0.
struct KnnGrid {
    float lo[3], sc[3];
};
__device__ __forceinline__ KnnGrid knn_grid(const uint32_t* __restrict__ bbox) {
    KnnGrid g;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.lo[k] = float_unord(bbox[k]);
        const float ext = float_unord(bbox[3 + k]) - g.lo[k];
        g.sc[k] = (ext > 0.0f && ext < INFINITY) ? (k == 2 ? 255.0f : 2047.0f) / ext : 0.0f;
    }
    return g;
}
__device__ __forceinline__ uint32_t knn_cell(float v, float lo, float sc, float top) {
    return (uint32_t)fminf(fmaxf((v - lo) * sc, 0.0f), top);  // clamped: a query may lie outside; NaN -> 0
}
__device__ __forceinline__ uint32_t knn_part3(uint32_t v) {  // 8 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// x and y carry 11 bits, z 8: the top 3 bits of x and y interleave two ways (6 bits), the low 8 bits
// of all three interleave three ways (24 bits).
__device__ __forceinline__ uint32_t knn_morton(const float4 p, const KnnGrid& g) {
    const uint32_t cx = knn_cell(p.x, g.lo[0], g.sc[0], 2047.0f), cy = knn_cell(p.y, g.lo[1], g.sc[1], 2047.0f),
                   cz = knn_cell(p.z, g.lo[2], g.sc[2], 255.0f);
    const uint32_t xh = cx >> 8, yh = cy >> 8;
    uint32_t top = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) top |= (((xh >> b) & 1u) << (2 * b + 1)) | (((yh >> b) & 1u) << (2 * b));
    return (top << 24) | (knn_part3(cx & 255u) << 2) | (knn_part3(cy & 255u) << 1) | knn_part3(cz);
}

// (key, position) of every point; a point with a non-finite coordinate sorts behind every finite one
__global__ __launch_bounds__(256) void knn_keys_kernel(const float4* __restrict__ pts, int32_t n,
                                                       const uint32_t* __restrict__ bbox, int2* __restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const KnnGrid g = knn_grid(bbox);
    const float4 p = pts[i];
    pairs[i] = make_int2(finite_xyz(p) ? (int32_t)knn_morton(p, g) : (int32_t)(1u << 30), (int32_t)i);
}

// The copy in key order, a whole number of leaves long: a non-finite point and the padding hold NaN
// coordinates (their distance to anything is NaN, which no candidate test passes).
__global__ __launch_bounds__(256) void knn_gather_kernel(const float4* __restrict__ pts, const int2* __restrict__ pairs,
                                                         int32_t n, int32_t npad, float4* __restrict__ sorted) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= npad) return;
    const float nan = __uint_as_float(0x7fc00000u);
    float4 v = make_float4(nan, nan, nan, __uint_as_float(0xFFFFFFFFu));
    if (t < n) {
        const int32_t i = pairs[t].y;
        const float4 p = pts[i];
        if (finite_xyz(p)) v = p;
        v.w = __uint_as_float((uint32_t)i);
    }
    sorted[t] = v;
}

// Leaf boxes: 16 consecutive positions each (a row of the DPP reductions); a leaf of NaN points only
// gets the empty box (+inf, -inf), whose lower bound to anything is +inf.
__global__ __launch_bounds__(256) void knn_leaf_box_kernel(const float4* __restrict__ sorted, int32_t npad,
                                                           float4* __restrict__ box) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (npad is a multiple of 16: whole rows)
    const float nan = __uint_as_float(0x7fc00000u);
    const float4 v = t < npad ? sorted[t] : make_float4(nan, nan, nan, 0.0f);
    const bool ok = v.x == v.x;
    const float lx = seg_minf(ok ? v.x : INFINITY, 16), ly = seg_minf(ok ? v.y : INFINITY, 16),
                lz = seg_minf(ok ? v.z : INFINITY, 16);
    const float hx = seg_maxf(ok ? v.x : -INFINITY, 16), hy = seg_maxf(ok ? v.y : -INFINITY, 16),
                hz = seg_maxf(ok ? v.z : -INFINITY, 16);
    if ((threadIdx.x & 15) == 0 && t < npad) {
        box[2 * (t / kKnnLeaf)] = make_float4(lx, ly, lz, 0.0f);
        box[2 * (t / kKnnLeaf) + 1] = make_float4(hx, hy, hz, 0.0f);
    }
}

// A level above: one wave per node, a lane per child.
__global__ __launch_bounds__(256) void knn_node_box_kernel(const float4* __restrict__ child, int32_t nchild,
                                                           float4* __restrict__ parent, int32_t nparent) {
    const int64_t node = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (node >= nparent) return;  // (a whole wave leaves)
    const int64_t c = node * kKnnFan + (threadIdx.x & 63);
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    if (c < nchild) {
        lo = child[2 * c];
        hi = child[2 * c + 1];
    }
    const float lx = wave_minf(lo.x), ly = wave_minf(lo.y), lz = wave_minf(lo.z);
    const float hx = wave_maxf(hi.x), hy = wave_maxf(hi.y), hz = wave_maxf(hi.z);
    if ((threadIdx.x & 63) == 0) {
        parent[2 * node] = make_float4(lx, ly, lz, 0.0f);
        parent[2 * node + 1] = make_float4(hx, hy, hz, 0.0f);
    }
}

static size_t knn_align(size_t x) { return (x + 255) & ~(size_t)255; }

KnnLayout knn_layout(int64_t n) {
    KnnLayout L = {};
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += knn_align(bytes);
        return at;
    };
    int64_t c = (n + kKnnLeaf - 1) / kKnnLeaf;
    L.sorted = take((size_t)(c > 0 ? c : 1) * kKnnLeaf * sizeof(float4));
    L.levels = 0;
    while (c > 0) {
        L.cnt[L.levels] = (int32_t)c;
        L.box[L.levels] = take((size_t)c * 2 * sizeof(float4));
        ++L.levels;
        if (c <= kKnnFan || L.levels == kKnnMaxLevels) break;
        c = (c + kKnnFan - 1) / kKnnFan;
    }
    L.bbox = take(6 * sizeof(uint32_t));
    L.bytes = o;
    return L;
}

KnnSortLayout knn_sort_layout(int64_t n) {
    KnnSortLayout L;
    const size_t nblk = (size_t)sector_blocks(n > 0 ? n : 1), m = (size_t)(n > 0 ? n : 1);
    L.pa = 0;
    L.pb = L.pa + knn_align(m * sizeof(int2));
    L.counts = L.pb + knn_align(m * sizeof(int2));
    L.offsets = L.counts + knn_align(256 * nblk * sizeof(int32_t));
    L.total = L.offsets + knn_align(256 * nblk * sizeof(int32_t));
    L.bytes = L.total + 256;
    return L;
}

KnnIndex knn_view(const void* index, int64_t n) {
    const KnnLayout L = knn_layout(n);
    const char* w = static_cast<const char*>(index);
    KnnIndex ix;
    ix.sorted = reinterpret_cast<const float4*>(w + L.sorted);
    for (int l = 0; l < L.levels; ++l) {
        ix.box[l] = reinterpret_cast<const float4*>(w + L.box[l]);
        ix.cnt[l] = L.cnt[l];
    }
    ix.levels = L.levels;
    ix.bbox = reinterpret_cast<const uint32_t*>(w + L.bbox);
    return ix;
}

// (key, i) pairs of the n points of pts by the box at bbox, sorted; -> the sorted pairs (in scratch)
static int2* knn_sorted_pairs(const float4* pts, int32_t n, const uint32_t* bbox, void* scratch, hipStream_t st) {
    const KnnSortLayout S = knn_sort_layout(n);
    char* w = static_cast<char*>(scratch);
    int2* pa = reinterpret_cast<int2*>(w + S.pa);
    int2* pb = reinterpret_cast<int2*>(w + S.pb);
    hipLaunchKernelGGL(knn_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, n, bbox, pa);
    return launch_radix_sort(pa, pb, n, (int)kKnnKeyBits, reinterpret_cast<int32_t*>(w + S.counts),
                             reinterpret_cast<int32_t*>(w + S.offsets), reinterpret_cast<int32_t*>(w + S.total), st);
}

hipError_t launch_knn_index(const float4* pts, int64_t n, void* index, void* scratch, hipStream_t st) {
    const KnnLayout L = knn_layout(n);
    char* w = static_cast<char*>(index);
    uint32_t* bbox = reinterpret_cast<uint32_t*>(w + L.bbox);
    float4* sorted = reinterpret_cast<float4*>(w + L.sorted);
    hipError_t e;
    if ((e = launch_finite_bbox(pts, n, bbox, st)) != hipSuccess) return e;
    const int2* pairs = knn_sorted_pairs(pts, (int32_t)n, bbox, scratch, st);
    const int32_t npad = L.cnt[0] * kKnnLeaf;
    const unsigned gp = (unsigned)(((int64_t)npad + 255) / 256);
    hipLaunchKernelGGL(knn_gather_kernel, dim3(gp), dim3(256), 0, st, pts, pairs, (int32_t)n, npad, sorted);
    hipLaunchKernelGGL(knn_leaf_box_kernel, dim3(gp), dim3(256), 0, st, sorted, npad, reinterpret_cast<float4*>(w + L.box[0]));
    for (int l = 1; l < L.levels; ++l)
        hipLaunchKernelGGL(knn_node_box_kernel, dim3((unsigned)((L.cnt[l] + 3) / 4)), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(w + L.box[l - 1]), L.cnt[l - 1],
                           reinterpret_cast<float4*>(w + L.box[l]), L.cnt[l]);
    return hipGetLastError();
}

// ---- the search
// One query's state in its kKnnL lanes: each lane keeps the K smallest keys of the points it was
// given; the lists merge at the end.  The bound a box must beat is the least of the lanes' k-th best
// and of max_dist² rounded up (the k-th best of the union is no larger than any lane's).
template <int K>
struct KnnLane {
    uint64_t best[K];
    float x, y, z;
    double md2;  // candidates: (double)d <= md2; negative for a lane without a query
    float lim;   // md2 rounded up to float, -inf without a query
    int k;

    __device__ __forceinline__ void consider(float px, float py, float pz, uint32_t idx, bool stored_finite) {
        const float d = map_calc_dist(x, y, z, px, py, pz);
        if (stored_finite && (double)d <= md2) knn_insert<K>(best, make_key(d, idx));  // (a NaN d fails)
    }
    __device__ __forceinline__ float bound() const {
        float kth = INFINITY;
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s == k - 1) kth = __uint_as_float((uint32_t)(best[s] >> 32));
        float b = fminf(kth, lim);
#pragma unroll
        for (int o = 1; o < kKnnL; o <<= 1) b = fminf(b, __shfl_xor(b, o, 64));
        return b;
    }
};

template <int K>
struct KnnWalk {
    KnnLane<K>& q;
    const KnnIndex& ix;
    const int lane, sub;
    float qlo[3], qhi[3];  // the box of the wave's queries
    float gb, qmax;        // this query's bound, the wave's largest

    // Nodes [grp * 64, grp * 64 + 64) of level LV: a lane per node tests its box against the wave's
    // query box and largest bound; the survivors are taken nearest first, each tested again per query
    // (wave-uniform box loads), and entered: a leaf is swept, a node's children are group `node` of
    // the level below.  The walk of a group ends when its nearest remaining node is beyond the bound.
    template <int LV>
    __device__ __forceinline__ void group(int grp) {
        const int cnt = ix.cnt[LV];
        const int mine = grp * kKnnFan + lane;
        const v4f* bv = reinterpret_cast<const v4f*>(ix.box[LV]);
        const int ld = min(mine, cnt - 1);
        const v4f mlo = bv[2 * (int64_t)ld], mhi = bv[2 * (int64_t)ld + 1];
        const float gx = fmaxf(fmaxf(mlo.x - qhi[0], qlo[0] - mhi.x), 0.0f);
        const float gy = fmaxf(fmaxf(mlo.y - qhi[1], qlo[1] - mhi.y), 0.0f);
        const float gz = fmaxf(fmaxf(mlo.z - qhi[2], qlo[2] - mhi.z), 0.0f);
        const float gap = __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx)) * kLbShrink;
        uint64_t cm = __ballot(mine < cnt && gap <= qmax);
        const cv4f_ptr bs = as_const(ix.box[LV]);
        while (cm) {
            const float g = ((cm >> lane) & 1) ? gap : INFINITY;
            const float mn = wave_minf(g);
            if (!(mn <= qmax)) break;
            const int c = __builtin_ctzll(__ballot(((cm >> lane) & 1) && g == mn));
            cm &= ~(1ull << c);
            const int node = grp * kKnnFan + c;
            const v4f lo = bs[2 * (int64_t)node], hi = bs[2 * (int64_t)node + 1];
            if (!__any(box_lb(lo, hi, q.x, q.y, q.z) * kLbShrink <= gb)) continue;
            if constexpr (LV == 0) {
                const float4* blk = ix.sorted + (int64_t)node * kKnnLeaf;
#pragma unroll
                for (int t = 0; t < kKnnLeaf / kKnnL; ++t) {
                    const float4 v = blk[sub + kKnnL * t];
                    q.consider(v.x, v.y, v.z, __float_as_uint(v.w), true);
                }
                gb = q.bound();
                qmax = wave_maxf(gb);
            } else {
                group<LV - 1>(node);
            }
        }
    }
};

template <int K>
__global__ __launch_bounds__(kKnnWG) void map_knn_kernel(const KnnSearch a, const int2* __restrict__ order) {
    __shared__ float4 tile[kKnnTile];
    constexpr int L = kKnnL, Q = 64 / L;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int qi = lane / L, sub = lane % L;
    const int64_t slot = (int64_t)blockIdx.x * kKnnQW + wave * Q + qi;  // the query's place in key order
    const bool have = slot < a.nq;
    int32_t o = 0;  // its row
    float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (have) {
        o = order ? order[slot].y : (int32_t)slot;
        qv = a.q[o];
    }
    const bool ok = have && finite_xyz(qv);  // a query with a non-finite coordinate finds nothing
    KnnLane<K> q;
    // empty slots hold (+inf, ~0): a real d² bound for the pruning tests, told from a stored point at
    // distance +inf by the index
#pragma unroll
    for (int s = 0; s < K; ++s) q.best[s] = make_key(INFINITY, 0xFFFFFFFFu);
    q.x = ok ? qv.x : 0.0f, q.y = ok ? qv.y : 0.0f, q.z = ok ? qv.z : 0.0f;
    q.md2 = ok ? a.md2 : -1.0;
    q.lim = ok ? a.bound : -INFINITY;
    q.k = a.k;

    if (a.ix.levels > 0) {
        KnnWalk<K> w = {q, a.ix, lane, sub, {}, {}, q.lim, 0.0f};
        w.qlo[0] = wave_minf(ok ? qv.x : INFINITY), w.qhi[0] = wave_maxf(ok ? qv.x : -INFINITY);
        w.qlo[1] = wave_minf(ok ? qv.y : INFINITY), w.qhi[1] = wave_maxf(ok ? qv.y : -INFINITY);
        w.qlo[2] = wave_minf(ok ? qv.z : INFINITY), w.qhi[2] = wave_maxf(ok ? qv.z : -INFINITY);
        w.qmax = wave_maxf(w.gb);
        const int top = a.ix.levels - 1;
        const int ngrp = (a.ix.cnt[top] + kKnnFan - 1) / kKnnFan;  // 1 below 2^28 points
        for (int g = 0; g < ngrp; ++g) {
            if (top == 0) w.template group<0>(g);
            else if (top == 1) w.template group<1>(g);
            else if (top == 2) w.template group<2>(g);
            else w.template group<3>(g);
        }
    }

    // what the tree does not hold: [tail0, n) through LDS, every lane of the workgroup taking part
    for (int64_t j0 = a.tail0; j0 < a.n; j0 += kKnnTile) {
        const int len = (int)min((int64_t)kKnnTile, a.n - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < len; t += kKnnWG) tile[t] = a.pts[j0 + t];
        __syncthreads();
        for (int t = sub; t < len; t += L) {
            const float4 v = tile[t];
            q.consider(v.x, v.y, v.z, (uint32_t)(j0 + t), finite_xyz(v));
        }
    }

    knn_merge_lanes<K, L>(q.best);
    if (sub != 0 || !have) return;
    int32_t found = 0;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        if (s < a.k) {
            const uint32_t idx = (uint32_t)q.best[s];
            const bool real = idx != 0xFFFFFFFFu;
            const int64_t row = (int64_t)o * a.k + s;
            if (a.pout) a.pout[row] = real ? a.pts[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.dout) a.dout[row] = real ? __uint_as_float((uint32_t)(q.best[s] >> 32)) : INFINITY;
            if (a.iout) a.iout[row] = real ? (int32_t)idx : -1;
            found += real ? 1 : 0;
        }
    }
    if (a.fout) a.fout[o] = found;
}

hipError_t launch_knn_search(const KnnSearch& s, void* scratch, hipStream_t st) {
    if (s.nq <= 0) return hipSuccess;
    const int2* order = nullptr;
    if (s.ix.levels > 0) order = knn_sorted_pairs(s.q, s.nq, s.ix.bbox, scratch, st);
    const dim3 grid((unsigned)((s.nq + kKnnQW - 1) / kKnnQW)), wg(kKnnWG);
    if (s.k <= 1)
        hipLaunchKernelGGL(map_knn_kernel<1>, grid, wg, 0, st, s, order);
    else if (s.k <= 8)
        hipLaunchKernelGGL(map_knn_kernel<8>, grid, wg, 0, st, s, order);
    else if (s.k <= 16)
        hipLaunchKernelGGL(map_knn_kernel<16>, grid, wg, 0, st, s, order);
    else
        hipLaunchKernelGGL(map_knn_kernel<32>, grid, wg, 0, st, s, order);
    return hipGetLastError();
}

}  // namespace icp4r
