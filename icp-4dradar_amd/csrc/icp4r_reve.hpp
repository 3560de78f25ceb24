// icp4r_reve.hpp — what icp4r_reve.cpp hands to the kernel of icp4r_reve.hip (include/icp4r/icp4r_reve.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp4r/icp4r_reve.h"

namespace icp4r {

constexpr int kReveWG = 1024;     // threads per scan's workgroup
constexpr int kReveLdsPts = 8192; // points of a scan held in LDS (float4: 128 KB); the rest in `spill`
constexpr int kReveMaxHyp = ICP4R_REVE_MAX_ITERATIONS;
constexpr int kReveMaxBlocks = ICP4R_REVE_MAX_POINTS / 64;  // 64-point blocks of the rank index

struct ReveArgs {
    const float* rec;       // device records, 5 floats each
    const int64_t* off;     // [nscans] first record of scan s
    const int32_t* cnt;     // [nscans]
    const int32_t* bad;     // optional [nscans] (launch_gate_guard): non-zero = refuse the scan
    int32_t max_n;
    int32_t lds_pts;        // min(max_n, kReveLdsPts): the dynamic LDS holds this many points
    float4* spill;          // [nscans * spill_stride] points lds_pts.. of each scan (nullptr: none)
    int64_t spill_stride;   // max_n - lds_pts
    float4* xyzi;           // optional: the PointXYZI fill, point i of scan s at off[s] + i
    uint8_t* mask;          // optional: inlier flag per record
    icp4r_reve_result* results;
    int32_t iterations;     // hypotheses (icp4r_reve_ransac_iterations)
    int32_t use_z;
    uint64_t seed;
    double min_dist, max_dist, min_db, az_lim, el_lim, zmin, zmax, factor;
    double zero_thresh, keep;  // keep = 1 - allowed_outlier_percentage
    double sig_zero[3], sig_off[3], sig_max[3];
    double max_cond, inlier_thresh;
};

hipError_t launch_reve(const ReveArgs& a, int nscans, hipStream_t st);

}  // namespace icp4r
