// ikd_ref_pcl.h — TEST INFRASTRUCTURE ONLY.  Force-included (-include) in front of every translation
// unit of the `ref` target of oracle/Makefile, which compiles the reference's own ikd-Tree against
// the project's PCL-1.8-shaped include tree (tests/cpp/pcl18).  ikd_Tree.h includes only
// <pcl/point_types.h> and relies on real PCL for the rest; this header supplies what that stand-in
// tree leaves out:
//   - <cstring> (memset / memcpy), <vector> and <memory>, which real PCL drags in;
//   - Eigen::aligned_allocator (Eigen/Core) and pcl::PointCloud for the call-site programs;
//   - pcl::PointXYZ and pcl::PointXYZINormal, which ikd_Tree.cpp instantiates its tree for.
#pragma once
#include <cstring>
#include <memory>
#include <vector>

#include <Eigen/Core>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

namespace pcl {
struct alignas(16) PointXYZ {
    float x = 0.f, y = 0.f, z = 0.f, w = 1.f;
};
struct alignas(16) PointXYZINormal {
    float x = 0.f, y = 0.f, z = 0.f, w = 1.f;
    float normal_x = 0.f, normal_y = 0.f, normal_z = 0.f, normal_w = 0.f;
    float intensity = 0.f, curvature = 0.f, pad[2] = {0.f, 0.f};
};
}  // namespace pcl
