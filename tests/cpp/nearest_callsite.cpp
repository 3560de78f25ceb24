// ikd-Tree's Nearest_Search as a LIO-style consumer calls it, compiled against
// include/icp4r/ikd_compat.hpp instead of ikd_Tree.h (tests/test_map_nearest*.py compile this
// themselves, with and without tests/cpp/pcl18).  Reads one case from a text file —
//     n_build n_add n_query k max_dist        (max_dist < 0: the call's default)
//     n_build + n_add + n_query lines "x y z"
// — gives every stored point its index as intensity, and prints per query the indices and the bits of
// the distances the call returns.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#ifdef ICP4R_CALLSITE_REFERENCE_IKD_TREE
#include "ikd_Tree.h"
#else
#include "icp4r/ikd_compat.hpp"
#endif

typedef pcl::PointXYZI PointType;
typedef KD_TREE<PointType>::PointVector PointVector;

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s case.txt\n", argv[0]);
        return 2;
    }
    std::ifstream f(argv[1]);
    int nb, na, nq, k;
    double max_dist;
    f >> nb >> na >> nq >> k >> max_dist;
    PointVector build, add, query;
    for (int i = 0; i < nb + na + nq; ++i) {
        PointType p;
        f >> p.x >> p.y >> p.z;
        p.intensity = (float)i;
        (i < nb ? build : i < nb + na ? add : query).push_back(p);
    }
    if (!f) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    static KD_TREE<PointType> ikdtree(0.5, 0.6, 0.2);  // static: the reference's tree is about 64 MB by value
    ikdtree.Build(build);
    ikdtree.Add_Points(add, false);
    for (int i = 0; i < nq; ++i) {
        PointType point_world = query[i];
        PointVector points_near;
        std::vector<float> pointSearchSqDis;
        if (max_dist < 0)
            ikdtree.Nearest_Search(point_world, k, points_near, pointSearchSqDis);
        else
            ikdtree.Nearest_Search(point_world, k, points_near, pointSearchSqDis, max_dist);
        std::printf("q%d:", i);
        for (size_t t = 0; t < points_near.size(); ++t) {
            unsigned bits;
            std::memcpy(&bits, &pointSearchSqDis[t], 4);
            std::printf(" %d/%08x", (int)points_near[t].intensity, bits);
        }
        std::printf("\n");
    }
    return 0;
}
