// voxel_compat.hpp — header-only C++ facade: pcl::VoxelGrid over the icp4r C ABI
// (include/icp4r/icp4r_voxel.h states the contract).
//
// Drop-in for the reference node's surround-map step (radar_odometry.cpp:426-429).  A maintainer replaces
//     #include <pcl/filters/voxel_grid.h>
// by
//     #include <icp4r/voxel_compat.hpp>
// and links libicp4r.so; the call sites stay textually unchanged.
//
// As pcl_compat.hpp: with real PCL and Eigen on the include path their PointCloud types are used
// (ICP4R_HAVE_PCL; tests/cpp/pcl18 is a PCL-1.8-shaped include tree), otherwise that header's stand-ins
// (ICP4R_STANDALONE).  Points are repacked to float4 (x, y, z, intensity) on the way in, so PCL's 32-byte
// PointXYZI keeps its intensity; a point type without an intensity member is filtered with intensity 0.
// Define ICP4R_NO_PCL_ALIAS to get icp4r::VoxelGrid without the pcl:: alias.
#pragma once

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "icp4r/icp4r_voxel.h"
#include "icp4r/pcl_compat.hpp"

namespace icp4r {

namespace voxel_detail {
template <typename P>
auto intensity_of(const P& p, int) -> decltype(static_cast<float>(p.intensity)) {
    return p.intensity;
}
template <typename P>
float intensity_of(const P&, long) {
    return 0.0f;
}
template <typename P>
auto set_intensity(P& p, float v, int) -> decltype(void(p.intensity)) {
    p.intensity = v;
}
template <typename P>
void set_intensity(P&, float, long) {}
}  // namespace voxel_detail

// pcl::VoxelGrid<PointT> with PCL 1.8.1's defaults (no filter-field limits, no leaf layout).
template <typename PointT>
class VoxelGrid {
  public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;

    VoxelGrid() { icp4r_voxel_params_default(&params_); }

    void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
    PointCloudConstPtr const getInputCloud() { return input_; }
    void setLeafSize(float lx, float ly, float lz) {
        params_.leaf[0] = lx;
        params_.leaf[1] = ly;
        params_.leaf[2] = lz;
    }
    void setDownsampleAllData(bool downsample) { params_.downsample_all_data = downsample ? 1 : 0; }
    bool getDownsampleAllData() { return params_.downsample_all_data != 0; }
    void setMinimumPointsNumberPerVoxel(unsigned int min_points_per_voxel) {
        params_.min_points_per_voxel = min_points_per_voxel;
    }
    unsigned int getMinimumPointsNumberPerVoxel() { return params_.min_points_per_voxel; }

    // Filter::filter(PointCloud& output)
    void filter(PointCloud& output) {
        if (!input_) {
            std::fprintf(stderr, "[pcl::VoxelGrid::filter] No input dataset given!\n");
            output.points.clear();
            finish(output);
            return;
        }
        if (params_.leaf[0] == 0.0f && params_.leaf[1] == 0.0f && params_.leaf[2] == 0.0f) {  // PCL: leaf size not set
            std::fprintf(stderr, "[pcl::VoxelGrid::applyFilter] No leaf size given!\n");
            output.points.clear();
            finish(output);
            return;
        }
        const size_t n = input_->points.size();
        std::vector<float> in(4 * n + 4), out(4 * n + 4);
        for (size_t i = 0; i < n; ++i) {
            const PointT& p = input_->points[i];
            in[4 * i + 0] = p.x;
            in[4 * i + 1] = p.y;
            in[4 * i + 2] = p.z;
            in[4 * i + 3] = voxel_detail::intensity_of(p, 0);
        }
        int64_t k = 0;
        const int rc = icp4r_voxel_filter(thread_context(), in.data(), (int64_t)n, 16, &params_, out.data(), (int64_t)n, &k);
        if (rc == ICP4R_E_TOO_LARGE && k == -1) {
            std::fprintf(stderr, "[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. "
                                 "Integer indices would overflow.\n");
            if (&output != input_.get()) output = *input_;  // PCL: output = *input_
            return;
        }
        if (rc != ICP4R_OK) throw std::runtime_error(std::string("icp4r_voxel_filter: ") + icp4r_last_error());
        output.points.clear();
        output.points.resize((size_t)k);  // default-constructed points (PointXYZI: data[3] = 1)
        for (size_t i = 0; i < (size_t)k; ++i) {
            PointT& p = output.points[i];
            p.x = out[4 * i + 0];
            p.y = out[4 * i + 1];
            p.z = out[4 * i + 2];
            voxel_detail::set_intensity(p, out[4 * i + 3], 0);
        }
        finish(output);
    }

  private:
    // PCL: the output is unorganised and dense (applyFilter: height 1, is_dense true)
    static void finish(PointCloud& output) {
#ifdef ICP4R_HAVE_PCL
        output.width = static_cast<uint32_t>(output.points.size());
        output.height = 1;
        output.is_dense = true;
#else
        (void)output;
#endif
    }

    PointCloudConstPtr input_;
    icp4r_voxel_params params_;
};

}  // namespace icp4r

#ifndef ICP4R_NO_PCL_ALIAS
namespace pcl {
template <typename PointT>
using VoxelGrid = icp4r::VoxelGrid<PointT>;
}
#endif
