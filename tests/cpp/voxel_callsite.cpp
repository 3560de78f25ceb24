// The reference node's surround-map step (radar_odometry.cpp:426-429) compiled against
// include/icp4r/voxel_compat.hpp instead of <pcl/filters/voxel_grid.h> (tests/test_voxel*.py compile
// this themselves, with and without tests/cpp/pcl18).  Reads n x 4 float32 (x, y, z, intensity) from
// in.bin into RadarCloudMap, filters, and writes downSizeFilterMap to out.bin: int64 K, K x 4 float32.
#include <cstdint>
#include <cstdio>
#include <vector>

#ifdef ICP4R_CALLSITE_REFERENCE_PCL
#include <pcl/filters/voxel_grid.h>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#else
#include "icp4r/voxel_compat.hpp"
#endif

pcl::PointCloud<pcl::PointXYZI>::Ptr RadarCloudMap(new pcl::PointCloud<pcl::PointXYZI>);
pcl::PointCloud<pcl::PointXYZI>::Ptr downSizeFilterMap(new pcl::PointCloud<pcl::PointXYZI>);

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    float v[4];
    while (std::fread(v, sizeof(float), 4, f) == 4) {
        pcl::PointXYZI p_sel;
        p_sel.x = v[0];
        p_sel.y = v[1];
        p_sel.z = v[2];
        p_sel.intensity = v[3];
        RadarCloudMap->push_back(p_sel);
    }
    std::fclose(f);

    pcl::VoxelGrid<pcl::PointXYZI> sor;
    sor.setInputCloud(RadarCloudMap);
    sor.setLeafSize(0.5f, 0.5f, 0.5f);
    sor.filter(*downSizeFilterMap);

    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) {
        std::perror(argv[2]);
        return 2;
    }
    const int64_t k = (int64_t)downSizeFilterMap->points.size();
    std::fwrite(&k, sizeof(k), 1, o);
    for (size_t i = 0; i < downSizeFilterMap->points.size(); ++i) {
        const pcl::PointXYZI& p = downSizeFilterMap->points[i];
        const float w[4] = {p.x, p.y, p.z, p.intensity};
        std::fwrite(w, sizeof(float), 4, o);
    }
    std::fclose(o);
    return 0;
}
