/*
 * icp4r_voxel_acc.h — the incremental voxel grid: a device-resident accumulator that is handed each
 * scan once and gives back the downsampled map, where the radar_odometry node runs pcl::VoxelGrid over
 * its whole accumulated RadarCloudMap on every frame (radar_odometry.cpp:426-429).
 *
 *   Contract    After any sequence of adds, a filter returns exactly what icp4r_voxel_filter
 *               (icp4r_voxel.h) returns for the concatenation of all added clouds in add order under
 *               the same params: count, order, every bit, and the grid-overflow answer.  Two facts of
 *               that contract make it so: ascending leaf index is lexicographic
 *               order of the absolute cell (cz, cy, cx) whatever the bounding box is, so a voxel list
 *               sorted by absolute cell is always in output order; and a voxel's centroid chain runs in
 *               arrival order from +0.0f, so stored partial sums and a count continue the same float
 *               additions when a later scan adds members, and one division by (float)m at output
 *               gives the same bits.
 *   Params      fixed at create for the accumulator's life; checked as icp4r_voxel.h checks them.
 *   Points      as icp4r_voxel.h: a point takes part iff x, y and z are finite; a 12-byte host point has
 *               intensity 0; an add of n = 0 points or of no participating point changes nothing.
 *   Overflow    the verdict comes from the accumulated min_p / max_p by icp4r_voxel.h's rule.  The
 *               host filter returns ICP4R_E_TOO_LARGE with *out_n = -1, the device filter stores -1 in
 *               *d_count; nothing is written.  Overflow does not damage the state (size still answers,
 *               adds still merge); it lasts until clear only because the box never shrinks.
 *   Range       the one deviation.  Cells are stored as offsets from an origin, the minimum cell of the
 *               first add with a participating point; each axis offset must lie in [-2^20, 2^20) (at
 *               leaf 0.5: +-524 km) and the cell itself must be an int.  A host add (add, add_map) whose
 *               own box would leave the range returns ICP4R_E_TOO_LARGE and leaves the accumulator
 *               untouched.  A device add cannot return the status: it skips the whole add and sets a
 *               sticky flag, with which the device filter stores -2 and the host filter returns
 *               ICP4R_E_TOO_LARGE with *out_n = -2, until clear.  Overflow (-1) is answered first.
 *   Limits      n >= 2^31, 2^31 or more voxels (by the host's bound, below), or 2^32 or more points
 *               added in total: ICP4R_E_TOO_LARGE.  A stride below 12 or no multiple of 4, a NULL
 *               pointer with n > 0, a NULL accumulator: ICP4R_E_INVALID.  An accumulator whose context
 *               was destroyed: ICP4R_E_INVALID without a HIP call (destroy still frees it).  More
 *               voxels than out_cap: ICP4R_E_TOO_LARGE with *out_n = the number needed, nothing
 *               written.
 *   filter      does not modify the state: twice in a row gives identical bytes, and adds may follow.
 *               The device filter needs room at d_out for as many float4 as there are voxels (size);
 *               the number of points added is always enough.
 *   size        voxels: the stored voxels, whatever min_points_per_voxel says; points: the sum of n
 *               over the accepted adds (non-finite points included, and a device add that the range
 *               rule skipped, which the host cannot know).
 *   Growth      the buffers only grow.  The host keeps an upper bound on the voxel count: the count it
 *               last read back plus the points added since.  When that bound exceeds the capacity the
 *               entry synchronises its stream, reads the count back and, if it still must, grows
 *               geometrically (at least to 4096 voxels, else doubling) and copies the state.  The add
 *               workspace grows with the largest scan the same way.  Otherwise the device entries
 *               never synchronise; reserve (voxels) up front — and a first add no smaller than the
 *               later ones — keeps them so.  The host entries and size synchronise and read the count
 *               back.
 *   Streams     the host entries, add_map and clear run on the context's stream and are synchronous;
 *               the device entries are asynchronous on hip_stream (NULL = the context's stream) and
 *               read n float4 points.  Calls on one accumulator must not overlap: the caller orders
 *               work it puts on different streams.  add_map takes a map of the same context.
 *
 * Out of scope: deleting points (float sums cannot subtract exactly; after icp4r_map_delete_boxes,
 * clear and add_map), an update in place for adds that bring no new cell.
 */
#ifndef ICP4R_VOXEL_ACC_H
#define ICP4R_VOXEL_ACC_H

#include "icp4r/icp4r_voxel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct icp4r_voxel_acc icp4r_voxel_acc;

int icp4r_voxel_acc_create(icp4r_ctx* ctx, const icp4r_voxel_params* params, icp4r_voxel_acc** out);
int icp4r_voxel_acc_destroy(icp4r_voxel_acc* acc);
/* empty again (origin, box and range flag too); keeps its buffers */
int icp4r_voxel_acc_clear(icp4r_voxel_acc* acc);
int icp4r_voxel_acc_reserve(icp4r_voxel_acc* acc, int64_t voxels);
int icp4r_voxel_acc_add(icp4r_voxel_acc* acc, const float* pts, int64_t n, int32_t stride_bytes);
int icp4r_voxel_acc_add_device(icp4r_voxel_acc* acc, const float* d_pts, int64_t n, void* hip_stream);
/* the store's points, in insertion order, as one add */
int icp4r_voxel_acc_add_map(icp4r_voxel_acc* acc, icp4r_map* map);
int icp4r_voxel_acc_filter(icp4r_voxel_acc* acc, float* out, int64_t out_cap, int64_t* out_n);
int icp4r_voxel_acc_filter_device(icp4r_voxel_acc* acc, float* d_out, int32_t* d_count, void* hip_stream);
int icp4r_voxel_acc_size(icp4r_voxel_acc* acc, int64_t* voxels, int64_t* points);

#ifdef __cplusplus
}
#endif

#endif /* ICP4R_VOXEL_ACC_H */
