// ikd-Tree's map-maintenance calls compiled against include/icp4r/ikd_compat.hpp instead of
// ikd_Tree.h: Build, Add_Points(.., true), Box_Search, Radius_Search, Delete_Point_Boxes, with
// BoxPointType.  Reads one case from a text file —
//     ds n_build n_add n_boxes
//     cx cy cz radius
//     n_build + n_add lines "x y z", then n_boxes lines "min xyz max xyz"
// — gives every point its index as intensity, and prints the counter and the indices each call
// returns, for tests/test_map_edit_gpu.py to compare with the recorded reference outputs.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <limits>
#include <vector>

#ifdef ICP4R_CALLSITE_REFERENCE_IKD_TREE  // oracle/Makefile, target ref: the reference's own header
#include "ikd_Tree.h"
#else
#include "icp4r/ikd_compat.hpp"
#endif

typedef pcl::PointXYZI PointType;
typedef KD_TREE<PointType>::PointVector PointVector;

static void print_ids(const char* name, const PointVector& v) {
    std::printf("%s:", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf(" %d", (int)v[i].intensity);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s case.txt\n", argv[0]);
        return 2;
    }
    std::ifstream f(argv[1]);
    float ds, radius;
    int nb, na, nboxes;
    PointType center;
    f >> ds >> nb >> na >> nboxes >> center.x >> center.y >> center.z >> radius;
    PointVector build, add;
    for (int i = 0; i < nb + na; ++i) {
        PointType p;
        f >> p.x >> p.y >> p.z;
        p.intensity = (float)i;
        (i < nb ? build : add).push_back(p);
    }
    std::vector<BoxPointType> boxes((size_t)nboxes);
    for (BoxPointType& b : boxes) {
        for (float& v : b.vertex_min) f >> v;
        for (float& v : b.vertex_max) f >> v;
    }
    if (!f) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    static KD_TREE<PointType> tree(0.5, 0.6, 0.2);  // static: the reference's tree is about 64 MB by value
    tree.Build(build);
    tree.set_downsample_param(ds);
    const int counter = tree.Add_Points(add, true);
    BoxPointType all;
    for (int k = 0; k < 3; ++k) {
        all.vertex_min[k] = -std::numeric_limits<float>::infinity();
        all.vertex_max[k] = std::numeric_limits<float>::infinity();
    }
    PointVector found;
    std::printf("counter: %d\n", counter);
    tree.Box_Search(all, found);
    print_ids("survivors", found);
    tree.Radius_Search(center, radius, found);
    print_ids("radius", found);
    std::printf("deleted: %d\n", tree.Delete_Point_Boxes(boxes));
    tree.Box_Search(all, found);
    print_ids("after_delete", found);
    std::printf("size: %d\n", tree.size());
    return 0;
}
