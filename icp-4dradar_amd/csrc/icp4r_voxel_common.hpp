// icp4r_voxel_common.hpp — device pieces shared by the voxel-grid filter (icp4r_voxel.hip) and the
// incremental voxel grid (icp4r_voxel_acc.hip): the grid and its overflow verdict from a bounding box,
// the stable compaction of an index range, and the wave broadcast of the centroid chains.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icp4r_device.hpp"
#include "icp4r_internal.hpp"

namespace icp4r {

constexpr int kVxWG = 256;
constexpr int kVxPer = 16;                // elements per thread of a compaction block
constexpr int kVxBlock = kVxWG * kVxPer;  // elements per workgroup
constexpr int kVxShort = 16;              // voxels of at most this many members: one lane walks them

static inline int64_t vx_blocks(int64_t n) { return (n + kVxBlock - 1) / kVxBlock; }

// min_b, div and the overflow flag from the bounding box (6 order-preserving words).  The grid is
// refused (flag -1) when PCL's own check refuses it (d[k] outside [1, 2^31] or d0 d1 d2 > INT32_MAX),
// when div0 div1 div2 > INT32_MAX (PCL's int leaf index would wrap), when floorf(p * inv) of a box
// corner is no int, or when an axis has more than 2^24 cells (beyond that floorf(p * inv) -
// (float)min_b is inexact).
__device__ inline VoxelGridDev voxel_grid_from_bbox(const uint32_t* __restrict__ bbox, const VoxelArgs& a) {
    VoxelGridDev r = {};
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = float_unord(bbox[k]);
        hi[k] = float_unord(bbox[3 + k]);
    }
    if (!(lo[0] <= hi[0])) {  // (+inf, -inf): no participating point
        r.flag = 1;
        return r;
    }
    bool over = false;
    int64_t d[3] = {1, 1, 1}, dv[3] = {1, 1, 1};
    for (int k = 0; k < 3; ++k) {
        const float f = (hi[k] - lo[k]) * a.inv[k];
        if (!(f < 2147483648.0f)) over = true;  // (int64)f + 1 > 2^31; an infinite extent too
        else d[k] = (int64_t)f + 1;
        const float fl = floorf(lo[k] * a.inv[k]), fh = floorf(hi[k] * a.inv[k]);
        if (!(fl >= -2147483648.0f && fh < 2147483648.0f)) {
            over = true;
        } else {
            r.min_b[k] = (int32_t)fl;
            dv[k] = (int64_t)(int32_t)fh - (int64_t)r.min_b[k] + 1;
            if (dv[k] > ((int64_t)1 << 24)) over = true;
            r.div[k] = (int32_t)(dv[k] < INT32_MAX ? dv[k] : INT32_MAX);
        }
    }
    if (!over) {
        const int64_t d01 = d[0] * d[1], v01 = dv[0] * dv[1];  // each factor <= 2^31: no int64 overflow
        over = d01 > INT32_MAX || d01 * d[2] > INT32_MAX || v01 > INT32_MAX || v01 * dv[2] > INT32_MAX;
    }
    r.flag = over ? -1 : 0;
    return r;
}

// ---- a stable compaction of an index range [0, size()): keep(i) is the test, emit(i, rank) the
// ordered write.  Blocks of kVxBlock elements: count -> launch_block_scan -> write.
template <class Pred>
__global__ __launch_bounds__(kVxWG) void vx_count_kernel(Pred pr, int32_t* __restrict__ counts) {
    __shared__ int32_t wsum[kVxWG / 64];
    const int64_t n = pr.size();
    const int64_t base = (int64_t)blockIdx.x * kVxBlock;
    int c = 0;
    for (int k = 0; k < kVxPer; ++k) {
        const int64_t i = base + k * kVxWG + threadIdx.x;
        if (i < n && pr.keep(i)) ++c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kVxWG / 64; ++w) t += wsum[w];
        counts[blockIdx.x] = t;
    }
}

// Round k of a block covers 256 consecutive elements, wave w its 64, lane its one: ranks taken round
// by round, wave by wave, lane by lane are index order.
template <class Pred>
__global__ __launch_bounds__(kVxWG) void vx_write_kernel(Pred pr, const int32_t* __restrict__ offsets) {
    __shared__ int32_t wcnt[kVxWG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = pr.size();
    const int64_t base = (int64_t)blockIdx.x * kVxBlock;
    if (base >= n) return;  // (the whole workgroup)
    int32_t run = offsets[blockIdx.x];
    for (int k = 0; k < kVxPer; ++k) {
        const int64_t i = base + k * kVxWG + tid;
        const bool keep = i < n && pr.keep(i);
        const uint64_t m = __ballot(keep);
        if (lane == 0) wcnt[wave] = __builtin_popcountll(m);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kVxWG / 64; ++w) {
            before += w < wave ? wcnt[w] : 0;
            tot += wcnt[w];
        }
        if (keep) {
            const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            pr.emit(i, run + before + (int32_t)r);
        }
        run += tot;
        __syncthreads();
    }
}

// max_n: the host's bound on size(); counts / offsets: vx_blocks(max_n) entries; *total: the kept.
template <class Pred>
static hipError_t vx_compact(const Pred& pr, int64_t max_n, int32_t* counts, int32_t* offsets, int32_t* total,
                             hipStream_t st) {
    const unsigned nblk = (unsigned)vx_blocks(max_n);
    hipLaunchKernelGGL(vx_count_kernel<Pred>, dim3(nblk), dim3(kVxWG), 0, st, pr, counts);
    hipError_t e = launch_block_scan(counts, (int)nblk, offsets, total, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vx_write_kernel<Pred>, dim3(nblk), dim3(kVxWG), 0, st, pr, offsets);
    return hipGetLastError();
}

__device__ __forceinline__ float vx_lane(float v, int lane) {  // lane: wave-uniform
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

}  // namespace icp4r
