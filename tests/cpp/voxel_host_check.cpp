// voxel_host_check — PCL 1.8.1's VoxelGrid<PointT>::applyFilter loop restated on the host, written
// independently of the library and of tests/voxel_grid_twin.py (tests/test_voxel.py compiles it with
// g++ -O2 -ffp-contract=off: x86-64 SSE float arithmetic, the node's own).  As in PCL: getMinMax3D
// over the finite points, the division counts and the overflow check, a std::vector of (leaf index,
// point index) records, a sort by leaf index, the first / last pass with the minimum-points test and
// float accumulators per voxel.  PCL's std::sort leaves the members of a voxel in an unspecified
// order; this restatement uses std::stable_sort, the order the contract fixes
// (include/icp4r/icp4r_voxel.h, which also lists the three cases refused beyond PCL's own check).
//
//   voxel_host_check in.bin out.bin lx ly lz downsample_all_data min_points_per_voxel
//
// in.bin: n x 4 float32 (x, y, z, intensity).  out.bin: int64 K, then K x 4 float32; K = -1 on grid
// overflow.  Prints the filter's wall time in ms (without file I/O) on stdout.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <utility>
#include <vector>

struct PointXYZI {
    float x, y, z, intensity;
};

struct cloud_point_index_idx {
    unsigned int idx;
    unsigned int cloud_point_index;
    cloud_point_index_idx(unsigned int idx_, unsigned int cloud_point_index_) : idx(idx_), cloud_point_index(cloud_point_index_) {}
    bool operator<(const cloud_point_index_idx& p) const { return idx < p.idx; }
};

static bool finite3(const PointXYZI& p) { return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z); }

// -> false on grid overflow
static bool apply_filter(const std::vector<PointXYZI>& input, const float leaf_size[3], bool downsample_all_data,
                         unsigned int min_points_per_voxel, std::vector<PointXYZI>& output) {
    output.clear();
    const float inverse_leaf_size[3] = {1.0f / leaf_size[0], 1.0f / leaf_size[1], 1.0f / leaf_size[2]};

    // getMinMax3D (is_dense = false branch)
    float min_p[3] = {std::numeric_limits<float>::max(), std::numeric_limits<float>::max(), std::numeric_limits<float>::max()};
    float max_p[3] = {-std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(), -std::numeric_limits<float>::max()};
    size_t taking_part = 0;
    for (size_t i = 0; i < input.size(); ++i) {
        if (!finite3(input[i])) continue;
        const float v[3] = {input[i].x, input[i].y, input[i].z};
        for (int k = 0; k < 3; ++k) {
            min_p[k] = std::min(min_p[k], v[k]);
            max_p[k] = std::max(max_p[k], v[k]);
        }
        ++taking_part;
    }
    if (taking_part == 0) return true;

    // the overflow check
    int64_t d[3];
    for (int k = 0; k < 3; ++k) {
        const float e = (max_p[k] - min_p[k]) * inverse_leaf_size[k];
        if (!(e < 2147483648.0f)) return false;  // (int64)e + 1 would leave [1, 2^31]
        d[k] = static_cast<int64_t>(e) + 1;
    }
    if (d[0] * d[1] > std::numeric_limits<int32_t>::max() || d[0] * d[1] * d[2] > std::numeric_limits<int32_t>::max())
        return false;

    // the bounding box in leaf units
    int min_b[3], max_b[3];
    int64_t div_b[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = std::floor(min_p[k] * inverse_leaf_size[k]), hi = std::floor(max_p[k] * inverse_leaf_size[k]);
        if (lo < -2147483648.0f || hi >= 2147483648.0f) return false;  // refused here: the cast to int is undefined
        min_b[k] = static_cast<int>(lo);
        max_b[k] = static_cast<int>(hi);
        div_b[k] = static_cast<int64_t>(max_b[k]) - min_b[k] + 1;
        if (div_b[k] > (1 << 24)) return false;  // refused here: the float subtraction below turns inexact
    }
    if (div_b[0] * div_b[1] > std::numeric_limits<int32_t>::max() ||
        div_b[0] * div_b[1] * div_b[2] > std::numeric_limits<int32_t>::max())
        return false;  // refused here: PCL's int leaf index would wrap
    const int divb_mul[3] = {1, static_cast<int>(div_b[0]), static_cast<int>(div_b[0] * div_b[1])};

    // first pass: a record per point
    std::vector<cloud_point_index_idx> index_vector;
    index_vector.reserve(input.size());
    for (size_t i = 0; i < input.size(); ++i) {
        if (!finite3(input[i])) continue;
        const int ijk0 = static_cast<int>(std::floor(input[i].x * inverse_leaf_size[0]) - static_cast<float>(min_b[0]));
        const int ijk1 = static_cast<int>(std::floor(input[i].y * inverse_leaf_size[1]) - static_cast<float>(min_b[1]));
        const int ijk2 = static_cast<int>(std::floor(input[i].z * inverse_leaf_size[2]) - static_cast<float>(min_b[2]));
        const int idx = ijk0 * divb_mul[0] + ijk1 * divb_mul[1] + ijk2 * divb_mul[2];
        index_vector.push_back(cloud_point_index_idx(static_cast<unsigned int>(idx), static_cast<unsigned int>(i)));
    }

    // second pass: sort by leaf index (stable: the contract's member order)
    std::stable_sort(index_vector.begin(), index_vector.end(), std::less<cloud_point_index_idx>());

    // third pass: the voxels with enough members
    std::vector<std::pair<unsigned int, unsigned int> > first_and_last_indices_vector;
    unsigned int index = 0;
    while (index < index_vector.size()) {
        unsigned int i = index + 1;
        while (i < index_vector.size() && index_vector[i].idx == index_vector[index].idx) ++i;
        if (i - index >= min_points_per_voxel) first_and_last_indices_vector.push_back(std::pair<unsigned int, unsigned int>(index, i));
        index = i;
    }

    // fourth pass: centroids
    output.resize(first_and_last_indices_vector.size());
    for (size_t cp = 0; cp < first_and_last_indices_vector.size(); ++cp) {
        const unsigned int first_index = first_and_last_indices_vector[cp].first;
        const unsigned int last_index = first_and_last_indices_vector[cp].second;
        float sum_x = 0.0f, sum_y = 0.0f, sum_z = 0.0f, sum_i = 0.0f;
        for (unsigned int li = first_index; li < last_index; ++li) {
            const PointXYZI& p = input[index_vector[li].cloud_point_index];
            sum_x += p.x;
            sum_y += p.y;
            sum_z += p.z;
            sum_i += p.intensity;
        }
        const float num = static_cast<float>(last_index - first_index);
        output[cp].x = sum_x / num;
        output[cp].y = sum_y / num;
        output[cp].z = sum_z / num;
        output[cp].intensity = downsample_all_data ? sum_i / num : 0.0f;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s in.bin out.bin lx ly lz downsample_all_data min_points_per_voxel\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<PointXYZI> input(static_cast<size_t>(bytes) / sizeof(PointXYZI));
    if (!input.empty() && std::fread(input.data(), sizeof(PointXYZI), input.size(), f) != input.size()) {
        std::fprintf(stderr, "short read\n");
        return 2;
    }
    std::fclose(f);
    const float leaf[3] = {std::strtof(argv[3], nullptr), std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr)};
    const bool all_data = std::atoi(argv[6]) != 0;
    const unsigned int min_points = static_cast<unsigned int>(std::strtoul(argv[7], nullptr, 10));

    std::vector<PointXYZI> output;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = apply_filter(input, leaf, all_data, min_points, output);
    const auto t1 = std::chrono::steady_clock::now();
    std::printf("%.3f\n", std::chrono::duration<double, std::milli>(t1 - t0).count());

    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) {
        std::perror(argv[2]);
        return 2;
    }
    const int64_t k = ok ? static_cast<int64_t>(output.size()) : -1;
    std::fwrite(&k, sizeof(k), 1, o);
    if (ok && !output.empty()) std::fwrite(output.data(), sizeof(PointXYZI), output.size(), o);
    std::fclose(o);
    return 0;
}
