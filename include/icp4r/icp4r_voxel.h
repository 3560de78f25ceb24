/*
 * icp4r_voxel.h — voxel-grid downsampling on the device: pcl::VoxelGrid<PointT>::applyFilter of PCL
 * 1.8.1, the last per-frame step of the radar_odometry node (radar_odometry.cpp:426-429):
 *
 *   pcl::VoxelGrid<pcl::PointXYZI> sor;  sor.setInputCloud(RadarCloudMap);
 *   sor.setLeafSize(0.5f, 0.5f, 0.5f);   sor.filter(*downSizeFilterMap);
 *
 * The rule, restated from PCL 1.8.1's filters/impl/voxel_grid.hpp (applyFilter),
 * common/impl/common.hpp (getMinMax3D) and common/impl/accumulators.hpp / centroid.hpp (the
 * per-voxel average).  Everything is float and unfused unless it says otherwise.
 *
 *   Parameters  leaf[3] (setLeafSize; finite and > 0, else ICP4R_E_INVALID), downsample_all_data
 *               (setDownsampleAllData, default 1), min_points_per_voxel
 *               (setMinimumPointsNumberPerVoxel, default 0).  inv[k] = 1.0f / leaf[k], a correctly
 *               rounded division.
 *   Points      a point takes part iff x, y and z are finite (PCL on a cloud with is_dense = false;
 *               a dense-labelled cloud has no other point).  A 12-byte point has intensity 0.  No
 *               participating point: 0 output points.
 *   Box         min_p, max_p: per-axis min and max of the participating points.
 *               d[k] = (int64)((max_p[k] - min_p[k]) * inv[k]) + 1; any d[k] outside [1, 2^31] or
 *               d0 d1 d2 > INT32_MAX is grid overflow (PCL: "Leaf size is too small for the input
 *               dataset", the output is a copy of the input).
 *               min_b[k] = (int)floorf(min_p[k] * inv[k]), max_b[k] likewise, div[k] = max_b[k] -
 *               min_b[k] + 1 (it can exceed d[k] by one).
 *   Deviations  where PCL's int arithmetic is undefined, the grid is refused as overflow too:
 *               div0 div1 div2 > INT32_MAX (PCL's leaf index wraps: leaf 1, points (0.9, 0.9, 0.9)
 *               and (1290.1, 1290.1, 1290.1) give d = 1290^3 but div = 1291^3); floorf(min_p[k] *
 *               inv[k]) or floorf(max_p[k] * inv[k]) outside [-2^31, 2^31) (the cast to int);
 *               div[k] > 2^24 (beyond it the float subtraction below is inexact and a cell index
 *               could leave the grid).
 *   Leaf index  ijk[k] = (int)(floorf(p[k] * inv[k]) - (float)min_b[k]);
 *               idx = ijk0 + ijk1 * div0 + ijk2 * div0 * div1.
 *   Voxels      a voxel is the set of participating points with one idx; one with fewer than
 *               min_points_per_voxel members gives no output; the output is in ascending idx.
 *   Centroid    of a voxel with m members, for each of x, y, z and intensity: s = +0.0f; s += value,
 *               member by member in ASCENDING INPUT INDEX; then s / (float)m (a division, not a
 *               reciprocal multiply).  With downsample_all_data = 0 the output intensity is 0.0f
 *               (PCL averages only the coordinate block into a default-constructed point).
 *
 * PCL orders a voxel's members by std::sort on idx alone, so its within-voxel order — and with it
 * the last bits of a centroid of three or more members — is whatever libstdc++'s introsort leaves;
 * this contract fixes the stable order.  Out of scope: filter-field limits,
 * setSaveLeafLayout, ApproximateVoxelGrid.
 *
 * Status: n = 0 or no finite point: ICP4R_OK, count 0.  Grid overflow: the host entries return
 * ICP4R_E_TOO_LARGE with *out_n = -1 and write nothing; the device entries return ICP4R_OK and store
 * -1 in *d_count.  More voxels than out_cap: ICP4R_E_TOO_LARGE with *out_n = the number needed,
 * nothing written.  n >= 2^31: ICP4R_E_TOO_LARGE.  A stride below 12, a NULL pointer with n > 0, a
 * leaf that is not finite and > 0: ICP4R_E_INVALID.  A map whose context was destroyed:
 * ICP4R_E_INVALID without a HIP call.
 *
 * Output points are float4 (x, y, z, intensity).  The workspace belongs to the context and only
 * grows.  The host entries are synchronous; the device entries are asynchronous on hip_stream (NULL =
 * the context's stream), read n float4 points, and need room for n points at d_out.  The map entries
 * filter the store as it stands and change nothing in it (the k-NN index stays valid).
 */
#ifndef ICP4R_VOXEL_H
#define ICP4R_VOXEL_H

#include "icp4r/icp4r_map.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct icp4r_voxel_params {
    float leaf[3];
    int32_t downsample_all_data;
    uint32_t min_points_per_voxel;
} icp4r_voxel_params;

/* leaf 0 (must be set), downsample_all_data 1, min_points_per_voxel 0 */
int icp4r_voxel_params_default(icp4r_voxel_params* params);

int icp4r_voxel_filter(icp4r_ctx* ctx, const float* pts, int64_t n, int32_t stride_bytes,
                       const icp4r_voxel_params* params, float* out, int64_t out_cap, int64_t* out_n);
int icp4r_voxel_filter_device(icp4r_ctx* ctx, const float* d_pts, int64_t n, const icp4r_voxel_params* params,
                              float* d_out, int32_t* d_count, void* hip_stream);
int icp4r_map_voxel_filter(icp4r_map* map, const icp4r_voxel_params* params, float* out, int64_t out_cap,
                           int64_t* out_n);
int icp4r_map_voxel_filter_device(icp4r_map* map, const icp4r_voxel_params* params, float* d_out, int32_t* d_count,
                                  void* hip_stream);

/* HIP-event time of the filter launches since the last reset: their mean and number. */
int icp4r_voxel_time_ms(icp4r_ctx* ctx, double* avg_ms, int32_t* calls);
int icp4r_voxel_time_reset(icp4r_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* ICP4R_VOXEL_H */
