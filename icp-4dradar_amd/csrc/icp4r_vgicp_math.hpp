// icp4r_vgicp_math.hpp — the arithmetic of the voxelized GICP that host and device share and that
// tests/vgicp_twin.py states in numpy (include/icp4r/icp4r_vgicp.h gives every operation order): the
// transformed source point, the cell of a point, the cell key and the neighbour offsets.  Plain C++ with
// no HIP call; only + * / floor, compiled unfused.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// (always inlined on the device: a call would pass its small arrays through scratch memory)
#define ICP4R_VGICP_HD __host__ __device__ __forceinline__
#else
#define ICP4R_VGICP_HD inline
#endif

namespace icp4r_vgicp {

constexpr int kAxisBits = 21;                   // a cell coordinate per axis, biased
constexpr int32_t kBias = 1 << (kAxisBits - 1);  // cells -2^20 .. 2^20 - 1
constexpr uint64_t kNoKey = ~0ull;              // no cell (above every key: the top bit is never set)

// Ta = ((R[r][0] a0 + R[r][1] a1) + R[r][2] a2) + t[r], R row-major
ICP4R_VGICP_HD void transform(const double* R, const double* t, const double* a, double* ta) {
    for (int r = 0; r < 3; ++r) ta[r] = ((R[3 * r] * a[0] + R[3 * r + 1] * a[1]) + R[3 * r + 2] * a[2]) + t[r];
}

// floor(p / resolution) of one axis as a double (the caller tests the range before it converts)
ICP4R_VGICP_HD double cell_of(double p, double resolution) { return floor(p / resolution); }

ICP4R_VGICP_HD bool cell_in_range(double c) { return c >= -(double)kBias && c < (double)kBias; }

// (cx, cy, cz) -> the key whose unsigned order is the lexicographic order of the cells; every
// coordinate inside [-2^20, 2^20)
ICP4R_VGICP_HD uint64_t cell_key(int32_t cx, int32_t cy, int32_t cz) {
    return ((uint64_t)(uint32_t)(cx + kBias) << (2 * kAxisBits)) | ((uint64_t)(uint32_t)(cy + kBias) << kAxisBits) |
           (uint64_t)(uint32_t)(cz + kBias);
}
ICP4R_VGICP_HD void key_cell(uint64_t key, int32_t* c) {
    const uint32_t mask = (1u << kAxisBits) - 1;
    c[0] = (int32_t)((key >> (2 * kAxisBits)) & mask) - kBias;
    c[1] = (int32_t)((key >> kAxisBits) & mask) - kBias;
    c[2] = (int32_t)(key & mask) - kBias;
}

// fast_gicp::NeighborSearchMethod DIRECT1 / DIRECT7 / DIRECT27: the number of offsets and offset q
ICP4R_VGICP_HD int offset_count(int mode) { return mode == 0 ? 1 : mode == 1 ? 7 : 27; }
ICP4R_VGICP_HD void offset_of(int mode, int q, int32_t* d) {
    if (mode == 2) {  // i, j, k in {-1, 0, 1}, x outermost, z innermost
        d[0] = q / 9 - 1;
        d[1] = q / 3 % 3 - 1;
        d[2] = q % 3 - 1;
    } else {  // (0,0,0), (+1,0,0), (-1,0,0), (0,+1,0), (0,-1,0), (0,0,+1), (0,0,-1)
        const int axis = q > 0 ? (q - 1) / 2 : -1, s = (q & 1) ? 1 : -1;
        d[0] = axis == 0 ? s : 0;  // (selects, no indexed store: the device keeps d in registers)
        d[1] = axis == 1 ? s : 0;
        d[2] = axis == 2 ? s : 0;
    }
}

}  // namespace icp4r_vgicp
