// ikd_compat.hpp — header-only C++ facade: the ikd-Tree map of radar_odometry over icp4r_map.h.
//
// Drop-in for the ikd-Tree calls of /root/reference/src/radar_odometry.cpp (:92, :347-348, :390,
// :396).  A maintainer replaces
//     #include "ikd_Tree.h"
// by
//     #include <icp4r/ikd_compat.hpp>
// and links libicp4r.so; `KD_TREE<pcl::PointXYZI> ikd_Tree(0.3, 0.6, 0.5);` and the Build /
// set_downsample_param / Add_Points / Sector_Search calls stay textually unchanged.
// ikd-Tree's map-maintenance calls carry the reference's signatures too (ikd_Tree.h:238-245):
// Nearest_Search, Delete_Point_Boxes, Box_Search, Radius_Search, Add_Points(.., true) and BoxPointType.
// One Nearest_Search per point pays a launch and a synchronisation each: a port should hand a whole
// scan to Nearest_Search_Batch.
//
// Semantics (include/icp4r/icp4r_map.h): a dense device store in insertion order; Sector_Search,
// Box_Search and Radius_Search are full filters with the reference's keep tests, returning the same
// set as ikd-Tree in insertion order; deleting keeps the survivors' order; the downsampling insert
// keeps, per touched downsample cell, the point nearest to the cell's centre.  Points are repacked to float4
// (x, y, z, intensity) on the way in and restored on the way out, so PCL's 32-byte PointXYZI keeps
// its intensity.  Each KD_TREE owns its own icp4r context (created on first use), so a
// namespace-scope tree, as the node declares it, outlives nothing it depends on.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "icp4r/icp4r_map.h"
#include "icp4r/pcl_compat.hpp"

namespace icp4r {

struct BoxPointType {  // ikd-Tree's box: min <= p < max per axis
    float vertex_min[3];
    float vertex_max[3];
};

template <typename PointType>
class KD_TREE {  // NOLINT — the reference's class name
  public:
    // ikd-Tree's storage type: a std::vector of points (PCL's aligned vector with real PCL/Eigen).
#ifdef ICP4R_HAVE_PCL
    using PointVector = std::vector<PointType, Eigen::aligned_allocator<PointType>>;
#else
    using PointVector = std::vector<PointType>;
#endif

    // delete / balance parameters steer ikd-Tree's rebalancing (no counterpart here: icp4r_map.h);
    // box_length is the downsample box of Add_Points(.., true) (the node adds with false).
    explicit KD_TREE(float delete_param = 0.5f, float balance_param = 0.6f, float box_length = 0.2f)
        : delete_param_(delete_param), balance_param_(balance_param), downsample_size_(box_length) {}
    KD_TREE(const KD_TREE&) = delete;
    KD_TREE& operator=(const KD_TREE&) = delete;
    ~KD_TREE() {
        if (map_) icp4r_map_destroy(map_);
        if (ctx_) icp4r_destroy(ctx_);
    }

    template <typename Vec>
    void Build(const Vec& point_cloud) {  // NOLINT
        std::vector<float> buf = pack(point_cloud);
        check(icp4r_map_build(map(), buf.data(), (int64_t)point_cloud.size(), 16), "Build");
    }

    void set_downsample_param(float box_length) { downsample_size_ = box_length; }

    template <typename Vec>
    int Add_Points(Vec& PointToAdd, bool downsample_on) {  // NOLINT
        std::vector<float> buf = pack(PointToAdd);
        if (downsample_on) {
            int64_t counter = 0;
            check(icp4r_map_add_points_downsample(map(), buf.data(), (int64_t)PointToAdd.size(), 16, downsample_size_,
                                                  &counter),
                  "Add_Points");
            return (int)counter;
        }
        check(icp4r_map_add_points(map(), buf.data(), (int64_t)PointToAdd.size(), 16, 0), "Add_Points");
        return 0;  // ikd-Tree returns its downsample counter: 0 without downsampling
    }

    int Delete_Point_Boxes(std::vector<BoxPointType>& BoxPoints) {  // NOLINT
        static_assert(sizeof(BoxPointType) == 6 * sizeof(float), "BoxPointType is min xyz, max xyz");
        int64_t deleted = 0;
        check(icp4r_map_delete_boxes(map(), BoxPoints.empty() ? nullptr : BoxPoints[0].vertex_min,
                                     (int32_t)BoxPoints.size(), &deleted),
              "Delete_Point_Boxes");
        return (int)deleted;
    }

    template <typename Vec>
    void Box_Search(const BoxPointType& Box_of_Point, Vec& Storage) {  // NOLINT
        float box[6];
        for (int k = 0; k < 3; ++k) {
            box[k] = Box_of_Point.vertex_min[k];
            box[3 + k] = Box_of_Point.vertex_max[k];
        }
        search(Storage, "Box_Search", [&](float* out, int64_t cap, int64_t* k) {
            return icp4r_map_box_search(map(), box, out, cap, k);
        });
    }

    template <typename Vec>
    void Radius_Search(PointType point, const float radius, Vec& Storage) {  // NOLINT
        const float c[3] = {point.x, point.y, point.z};
        search(Storage, "Radius_Search", [&](float* out, int64_t cap, int64_t* k) {
            return icp4r_map_radius_search(map(), c, radius, out, cap, k);
        });
    }

    template <typename Vec>
    void Sector_Search(PointType point, const float radius, const float heading, Vec& Storage) {  // NOLINT
        const float c[3] = {point.x, point.y, point.z};
        search(Storage, "Sector_Search", [&](float* out, int64_t cap, int64_t* k) {
            return icp4r_map_sector_search(map(), c, radius, heading, out, cap, k);
        });
    }

    // The reference's call: the k_nearest stored points nearest to `point` within max_dist, nearest
    // first, and their squared distances (exact; ties to the earliest inserted: icp4r_map.h).
    void Nearest_Search(PointType point, int k_nearest, PointVector& Nearest_Points,  // NOLINT
                        std::vector<float>& Point_Distance, double max_dist = INFINITY) {
        std::vector<PointType> one(1, point);
        std::vector<int> found;
        Nearest_Search_Batch(one, k_nearest, Nearest_Points, Point_Distance, found, max_dist);
        Nearest_Points.resize((size_t)found[0]);
        Point_Distance.resize((size_t)found[0]);
    }

    // The same for a whole scan in one launch: row q of Nearest_Points / Point_Distance (k_nearest
    // slots each) holds found[q] answers, nearest first; the unused slots hold a zero point and +inf.
    template <typename Vec, typename OutVec>
    void Nearest_Search_Batch(const Vec& points, int k_nearest, OutVec& Nearest_Points,  // NOLINT
                              std::vector<float>& Point_Distance, std::vector<int>& found, double max_dist = INFINITY) {
        const size_t nq = points.size(), rows = nq * (size_t)(k_nearest > 0 ? k_nearest : 0);
        std::vector<float> q = pack(points), out(rows * 4 + 4);
        std::vector<int32_t> cnt(nq + 1);
        Point_Distance.assign(rows, 0.0f);
        check(icp4r_map_nearest_search(map(), q.data(), (int64_t)nq, 16, k_nearest, max_dist, 0, out.data(),
                                       rows ? Point_Distance.data() : nullptr, nullptr, cnt.data()),
              "Nearest_Search");
        Nearest_Points.resize(rows);
        for (size_t i = 0; i < rows; ++i) {
            PointType& p = Nearest_Points[i];
            p.x = out[4 * i];
            p.y = out[4 * i + 1];
            p.z = out[4 * i + 2];
            p.intensity = out[4 * i + 3];
        }
        found.assign(cnt.begin(), cnt.begin() + (std::ptrdiff_t)nq);
    }

    int size() {
        int64_t n = 0;
        check(icp4r_map_size(map(), &n), "size");
        return (int)n;
    }

    icp4r_map* handle() { return map(); }

  private:
    icp4r_map* map() {
        if (!map_) {
            check(icp4r_create(&ctx_, 0), "icp4r_create");
            check(icp4r_map_create(ctx_, &map_), "icp4r_map_create");
        }
        return map_;
    }

    // A host search into Storage: query(out, cap, &k) fills at most cap float4 rows; intensity restored.
    template <typename Vec, typename Query>
    void search(Vec& Storage, const char* what, Query query) {
        Storage.clear();
        int64_t cap = 0;
        check(icp4r_map_size(map(), &cap), what);
        std::vector<float> out((size_t)(cap > 0 ? cap : 1) * 4);
        int64_t k = 0;
        check(query(out.data(), cap, &k), what);
        Storage.resize((size_t)k);
        for (int64_t i = 0; i < k; ++i) {
            PointType& p = Storage[(size_t)i];
            p.x = out[4 * i];
            p.y = out[4 * i + 1];
            p.z = out[4 * i + 2];
            p.intensity = out[4 * i + 3];
        }
    }

    template <typename Vec>
    static std::vector<float> pack(const Vec& v) {
        std::vector<float> buf(v.size() * 4 + 4);
        for (size_t i = 0; i < v.size(); ++i) {
            buf[4 * i] = v[i].x;
            buf[4 * i + 1] = v[i].y;
            buf[4 * i + 2] = v[i].z;
            buf[4 * i + 3] = v[i].intensity;
        }
        return buf;
    }

    static void check(int rc, const char* what) {
        if (rc != ICP4R_OK) throw std::runtime_error(std::string("KD_TREE::") + what + ": " + icp4r_last_error());
    }

    float delete_param_, balance_param_, downsample_size_;
    icp4r_ctx* ctx_ = nullptr;
    icp4r_map* map_ = nullptr;
};

}  // namespace icp4r

#ifndef ICP4R_NO_IKD_ALIAS
using icp4r::BoxPointType;
using icp4r::KD_TREE;
#endif
