// voxel_acc_compat.hpp — header-only C++ facade of the incremental voxel grid
// (include/icp4r/icp4r_voxel_acc.h states the contract): icp4r::IncrementalVoxelGrid<PointT>.
//
// Where the reference node filters its whole accumulated map every frame (radar_odometry.cpp:426-429),
//     pcl::VoxelGrid<pcl::PointXYZI> sor;  sor.setInputCloud(RadarCloudMap);
//     sor.setLeafSize(0.5f, 0.5f, 0.5f);   sor.filter(*downSizeFilterMap);
// a maintainer keeps one IncrementalVoxelGrid beside the map, hands it each scan as it is appended, and
// filters:
//     static icp4r::IncrementalVoxelGrid<pcl::PointXYZI> grid;   // setLeafSize(0.5f, 0.5f, 0.5f) once
//     grid.addCloud(scan_in_map_frame);
//     grid.filter(*downSizeFilterMap);
// The output equals pcl::VoxelGrid (voxel_compat.hpp) over the concatenation of the added clouds, bit
// for bit.  Point handling and the PCL / stand-in switch are voxel_compat.hpp's.
//
// The leaf and the two flags are fixed at the first addCloud; setters called later take effect after
// clear().  On grid overflow filter prints PCL's warning and returns an EMPTY cloud: PCL copies its
// input there, and an accumulator has no input cloud to copy.  A scan that leaves the accumulator's
// range (+-2^20 cells around the first scan) throws std::runtime_error from addCloud and is not added.
#pragma once

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "icp4r/icp4r_voxel_acc.h"
#include "icp4r/voxel_compat.hpp"

namespace icp4r {

template <typename PointT>
class IncrementalVoxelGrid {
  public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;

    IncrementalVoxelGrid() { icp4r_voxel_params_default(&params_); }
    ~IncrementalVoxelGrid() { icp4r_voxel_acc_destroy(acc_); }
    IncrementalVoxelGrid(const IncrementalVoxelGrid&) = delete;
    IncrementalVoxelGrid& operator=(const IncrementalVoxelGrid&) = delete;

    void setLeafSize(float lx, float ly, float lz) {
        params_.leaf[0] = lx;
        params_.leaf[1] = ly;
        params_.leaf[2] = lz;
    }
    void setDownsampleAllData(bool downsample) { params_.downsample_all_data = downsample ? 1 : 0; }
    void setMinimumPointsNumberPerVoxel(unsigned int min_points_per_voxel) {
        params_.min_points_per_voxel = min_points_per_voxel;
    }

    // One scan; the first call fixes the leaf and the flags.
    void addCloud(const PointCloudConstPtr& cloud) {
        if (!cloud) {
            std::fprintf(stderr, "[icp4r::IncrementalVoxelGrid::addCloud] No input dataset given!\n");
            return;
        }
        if (!acc_ && icp4r_voxel_acc_create(thread_context(), &params_, &acc_) != ICP4R_OK)
            throw std::runtime_error(std::string("icp4r_voxel_acc_create: ") + icp4r_last_error());
        const size_t n = cloud->points.size();
        std::vector<float> in(4 * n + 4);
        for (size_t i = 0; i < n; ++i) {
            const PointT& p = cloud->points[i];
            in[4 * i + 0] = p.x;
            in[4 * i + 1] = p.y;
            in[4 * i + 2] = p.z;
            in[4 * i + 3] = voxel_detail::intensity_of(p, 0);
        }
        if (icp4r_voxel_acc_add(acc_, in.data(), (int64_t)n, 16) != ICP4R_OK)
            throw std::runtime_error(std::string("icp4r_voxel_acc_add: ") + icp4r_last_error());
    }

    // The downsampled concatenation of the added clouds; nothing added yet: an empty cloud.
    void filter(PointCloud& output) {
        output.points.clear();
        int64_t k = 0, voxels = 0;
        std::vector<float> out(4);
        if (acc_) {
            if (icp4r_voxel_acc_size(acc_, &voxels, nullptr) != ICP4R_OK)
                throw std::runtime_error(std::string("icp4r_voxel_acc_size: ") + icp4r_last_error());
            out.resize(4 * (size_t)voxels + 4);
            const int rc = icp4r_voxel_acc_filter(acc_, out.data(), voxels, &k);
            if (rc == ICP4R_E_TOO_LARGE && k == -1) {
                std::fprintf(stderr, "[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. "
                                     "Integer indices would overflow.\n");
                k = 0;  // (no input cloud to copy: an empty output)
            } else if (rc != ICP4R_OK) {
                throw std::runtime_error(std::string("icp4r_voxel_acc_filter: ") + icp4r_last_error());
            }
        }
        output.points.resize((size_t)k);  // default-constructed points (PointXYZI: data[3] = 1)
        for (size_t i = 0; i < (size_t)k; ++i) {
            PointT& p = output.points[i];
            p.x = out[4 * i + 0];
            p.y = out[4 * i + 1];
            p.z = out[4 * i + 2];
            voxel_detail::set_intensity(p, out[4 * i + 3], 0);
        }
#ifdef ICP4R_HAVE_PCL
        output.width = static_cast<uint32_t>(output.points.size());
        output.height = 1;
        output.is_dense = true;
#endif
    }

    // Empty again; the next addCloud takes the leaf and the flags as they are then.
    void clear() {
        icp4r_voxel_acc_destroy(acc_);
        acc_ = nullptr;
    }

  private:
    icp4r_voxel_params params_;
    icp4r_voxel_acc* acc_ = nullptr;
};

}  // namespace icp4r
