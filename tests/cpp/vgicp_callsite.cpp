// A fast_gicp program's FastVGICP block compiled against include/icp4r/fast_gicp_compat.hpp instead of
// fast_gicp: the scan-to-map registration of tests/cpp/gicp_callsite.cpp with the voxelized class.  The
// scan and the submap come from two .bin files in the node's record format; the third argument picks
// the neighbour search (1, 7, 27; "radius": a mode the device path refuses).  Prints converged, score,
// iterations, output size and the final transformation for tests/test_vgicp_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "icp4r/fast_gicp_compat.hpp"

static pcl::PointCloud<pcl::PointXYZI>::Ptr read_scan(const char* path) {
    pcl::PointCloud<pcl::PointXYZI>::Ptr c(new pcl::PointCloud<pcl::PointXYZI>);
    std::ifstream f(path, std::ios::binary);
    float rec[5];
    while (f.read(reinterpret_cast<char*>(rec), sizeof(rec))) {
        pcl::PointXYZI p;
        p.x = rec[0];
        p.y = rec[1];
        p.z = rec[2];
        p.intensity = rec[3];
        c->push_back(p);
    }
    return c;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s scan_map.bin submap.bin 1|7|27|radius [resolution]\n", argv[0]);
        return 2;
    }
    pcl::PointCloud<pcl::PointXYZI>::Ptr scan_map = read_scan(argv[1]);
    pcl::PointCloud<pcl::PointXYZI>::Ptr SubMap = read_scan(argv[2]);
    pcl::PointCloud<pcl::PointXYZI>::Ptr Final(new pcl::PointCloud<pcl::PointXYZI>);
    const fast_gicp::NeighborSearchMethod method = !std::strcmp(argv[3], "1")    ? fast_gicp::NeighborSearchMethod::DIRECT1
                                                   : !std::strcmp(argv[3], "7")  ? fast_gicp::NeighborSearchMethod::DIRECT7
                                                   : !std::strcmp(argv[3], "27") ? fast_gicp::NeighborSearchMethod::DIRECT27
                                                                                 : fast_gicp::NeighborSearchMethod::DIRECT_RADIUS;

    fast_gicp::FastVGICP<pcl::PointXYZI, pcl::PointXYZI> vgicp;
    vgicp.clearTarget();
    vgicp.clearSource();
    vgicp.setResolution(argc > 4 ? std::atof(argv[4]) : 1.0);
    vgicp.setNeighborSearchMethod(method);
    vgicp.setVoxelAccumulationMode(fast_gicp::VoxelAccumulationMode::ADDITIVE);
    vgicp.setInputTarget(SubMap);
    vgicp.setInputSource(scan_map);
    vgicp.setCorrespondenceRandomness(5);
    vgicp.align(*Final);
    double score = vgicp.getFitnessScore();

    std::printf("%d %.17g %d %zu\n", (int)vgicp.hasConverged(), score, vgicp.getNrIterations(), Final->size());
    const Eigen::Matrix<float, 4, 4> T = vgicp.getFinalTransformation();
    for (int k = 0; k < 16; ++k) std::printf("%.9g%c", T.data()[k], k == 15 ? '\n' : ' ');
    return 0;
}
