// icp4r_vgicp.hpp — types shared by the voxelized GICP's host code (icp4r_vgicp.cpp) and kernels
// (icp4r_vgicp.hip); include/icp4r/icp4r_vgicp.h states the algorithm.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp4r_internal.hpp"

namespace icp4r {

constexpr int kVgicpMaxOffsets = 27;

// The Gaussian voxel maps of a batch's targets.  Target point i of pair p is element p * t_stride + i of
// the per-point arrays (elements past the pair's count are padding); the voxels of all pairs share the
// per-voxel arrays, pair p's at [vbeg[p], vbeg[p + 1]) in key order.
struct VgicpArgs {
    // the build's scratch
    uint64_t* pkey;     // [npairs * t_stride] the cell key per point (all-ones: padding, or outside the range)
    int2* pa;           // [npairs * t_stride] x 2: the sort's (key word, element) pairs
    int2* pb;
    int32_t* counts;    // the radix sort's and the compaction's block counts / offsets
    int32_t* offsets;
    int32_t* total;     // [2]: the voxels of the batch; the sort's own total
    int32_t* vstart;    // [npairs * t_stride] per voxel: the sorted position of its first point
    int32_t* bad;       // [npairs] 1: a coordinate outside the key range
    // the map
    const int2* sorted; // the elements ordered by (pair, key, index): .y = the element
    uint64_t* vkey;     // [npairs * t_stride] per voxel
    int32_t* vnum;
    double* vmean;      // x 3
    double* vcov;       // x 6, the upper triangle
    int32_t* vbeg;      // [npairs + 1]
    // the registration
    int32_t* corr;      // [npairs * x_stride * noff] the voxel of (point, offset) at the last linearisation, -1: none
    int64_t t_stride;
    double resolution;
    int32_t mode, noff;  // icp4r_vgicp_neighbor_search and its number of offsets
};

struct VgicpLayout {  // byte offsets into the workspace
    size_t pkey, pa, pb, counts, offsets, total, vstart, bad, vkey, vnum, vmean, vcov, vbeg, corr, bytes;
};
// npairs * t_stride < 2^31
VgicpLayout vgicp_layout(int64_t npairs, int64_t t_stride, int64_t x_stride, int noff);
void vgicp_bind(void* work, const VgicpLayout& L, VgicpArgs& m);

// The maps of npairs targets (points tgt + off[p], cnt[p] <= t_stride of them; cov6: their covariances'
// upper triangles, pair p's at p * t_stride).  state (or nullptr): pairs already invalid are skipped, and a
// pair with a coordinate outside the key range becomes invalid with ICP4R_E_INVALID.  Sets m.sorted.
hipError_t launch_vgicp_map(const float4* tgt, const int64_t* off, const int32_t* cnt, const double* cov6,
                            PairState* state, VgicpArgs& m, int npairs, hipStream_t st);
// One iteration of every active pair: the lookup and the linearisation, then the trials and the decision.
hipError_t launch_vgicp_iter(const PairArgs& a, const WorkArgs& w, const GicpArgs& g, const VgicpArgs& m, int npairs,
                             int max_n, int it, hipStream_t st);

}  // namespace icp4r
