// icp4r_common.hpp — the base of the ICP kernel units' include chain: the includes they all need, the
// ICP4R_WG_TICKS default, and what the index build (icp4r_index.hip) shares with the other stages
// (icp4r_kernels.hip, icp4r_frame.hip): the sizes of the two orders, the Morton cell code and its quantisation, and the packing
// of a query's index and sorted position.  No kernel.
#pragma once

#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "icp4r_device.hpp"
#include "icp4r_internal.hpp"
#include "icp4r_math.hpp"

#ifndef ICP4R_WG_TICKS
#define ICP4R_WG_TICKS 0  // diagnostic builds: per-workgroup phase stamps (tools/experiments/wg_ticks.py)
#endif

namespace icp4r {

constexpr int kCellBins = 1 << 14;
constexpr int kKdMaxN = 8192;

__device__ __forceinline__ uint32_t cell_code(float x, float y, float z, const float* lo, const float* sc) {
    const int cx = min(31, max(0, (int)((x - lo[0]) * sc[0])));
    const int cy = min(31, max(0, (int)((y - lo[1]) * sc[1])));
    const int cz = min(15, max(0, (int)((z - lo[2]) * sc[2])));
    uint32_t c = 0;
#pragma unroll
    for (int b = 4; b >= 0; --b) {  // interleave, most significant level first: x y z per level
        c = (c << 1) | ((cx >> b) & 1);
        c = (c << 1) | ((cy >> b) & 1);
        if (b < 4) c = (c << 1) | ((cz >> b) & 1);
    }
    return c;
}

// The source of pair p is ordered by its target's kd tree (src_order_kernel) rather than its own.
__device__ __forceinline__ bool src_by_tgt_tree(const PairArgs& a, const WorkArgs& w, int p) {
    const int m = a.tgt_n[p];
    // (src_order_kernel places at most kKdMaxN sources; a larger source gets its own index)
    return w.src_by_tgt && w.kdn && (w.kd_index & 1) && m > 0 && m <= kKdMaxN && w.t_stride <= kKdMaxN &&
           a.src_n[p] <= kKdMaxN;
}

__device__ __forceinline__ void mo_quant(const WorkArgs& w, int p, float* lo, float* sc) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float l = w.tbb[(int64_t)p * 8 + k], h = w.tbb[(int64_t)p * 8 + 3 + k];
        lo[k] = l;
        sc[k] = h > l ? (k == 2 ? 16.0f : 32.0f) / (h - l) : 0.0f;
    }
}

// query records {index | sorted position << kNtPosShift, ...} and nn_t[i].w (nt_pack, icp4r_tile.hpp)
constexpr int kNtPosShift = 14;
constexpr int kNtIdxMask = (1 << kNtPosShift) - 1;

}  // namespace icp4r
