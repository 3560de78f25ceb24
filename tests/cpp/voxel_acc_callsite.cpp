// The node's surround-map step in its incremental form, compiled against
// include/icp4r/voxel_acc_compat.hpp (tests/test_voxel_acc*.py compile this themselves, with and without
// tests/cpp/pcl18).  Each scanK.bin holds n x 4 float32 (x, y, z, intensity); every scan is handed to
// the grid once, the grid is filtered after each, and the last downSizeFilterMap goes to out.bin:
// int64 K, K x 4 float32.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "icp4r/voxel_acc_compat.hpp"

pcl::PointCloud<pcl::PointXYZI>::Ptr downSizeFilterMap(new pcl::PointCloud<pcl::PointXYZI>);

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s out.bin scan0.bin [scan1.bin ...]\n", argv[0]);
        return 2;
    }
    icp4r::IncrementalVoxelGrid<pcl::PointXYZI> grid;
    grid.setLeafSize(0.5f, 0.5f, 0.5f);
    grid.setDownsampleAllData(true);
    grid.setMinimumPointsNumberPerVoxel(0);
    for (int s = 2; s < argc; ++s) {
        std::FILE* f = std::fopen(argv[s], "rb");
        if (!f) {
            std::perror(argv[s]);
            return 2;
        }
        pcl::PointCloud<pcl::PointXYZI>::Ptr scan(new pcl::PointCloud<pcl::PointXYZI>);
        float v[4];
        while (std::fread(v, sizeof(float), 4, f) == 4) {
            pcl::PointXYZI p_sel;
            p_sel.x = v[0];
            p_sel.y = v[1];
            p_sel.z = v[2];
            p_sel.intensity = v[3];
            scan->push_back(p_sel);
        }
        std::fclose(f);
        grid.addCloud(scan);
        grid.filter(*downSizeFilterMap);
    }

    std::FILE* o = std::fopen(argv[1], "wb");
    if (!o) {
        std::perror(argv[1]);
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
