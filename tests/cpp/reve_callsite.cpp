// The reference node's ego-velocity step (radar_odometry.cpp:328, settings :574-611) written against
// include/icp4r/reve_compat.hpp: every setting set by name, estimate(), the inlier scan as the PointXYZI
// cloud the node fills `src` with (:329-342).  Reads n x 5 float32 (x, y, z, intensity,
// doppler) from in.bin; writes to out.bin: int32 success, int32 K, double v[3], double sigma[3],
// K x 4 float32 (x, y, z, intensity).  Optional third argument: the hypothesis seed.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "icp4r/reve_compat.hpp"

using Vector3 = std::array<double, 3>;

// the node's settings (radar_odometry.cpp:576-610), every one set by name
reve::RadarEgoVelocityEstimatorConfig node_settings() {
    reve::RadarEgoVelocityEstimatorConfig c;
    // which targets count
    c.min_dist = 0.25;
    c.max_dist = 100;
    c.min_db = 0;
    c.azimuth_thresh_deg = 60;
    c.elevation_thresh_deg = 60;
    c.filter_max_z = 3;
    c.filter_min_z = -3;
    c.doppler_velocity_correction_factor = 1.0;
    // standstill
    c.allowed_outlier_percentage = 0.25;
    c.thresh_zero_velocity = 0.05;
    c.sigma_zero_velocity_x = c.sigma_zero_velocity_y = c.sigma_zero_velocity_z = 0.025;
    // RANSAC
    c.use_ransac = true;
    c.N_ransac_points = 3;
    c.success_prob = 0.9999;
    c.outlier_prob = 0.4;
    c.inlier_thresh = 0.15;
    c.max_r_cond = 1000;
    // the least squares and its bounds
    c.use_cholesky_instead_of_bdcsvd = true;
    c.sigma_offset_radar_x = c.sigma_offset_radar_z = 0.05;
    c.sigma_offset_radar_y = 0.025;
    c.max_sigma_x = c.max_sigma_y = c.max_sigma_z = 0.2;
    // ODR (accepted, without effect)
    c.use_odr = true;
    c.min_speed_odr = 4.0;
    c.sigma_v_d = 0.125;
    c.model_noise_offset_deg = 2.0;
    c.model_noise_scale_deg = 10.0;
    return c;
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        std::fprintf(stderr, "usage: %s in.bin out.bin [seed]\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    pcl::PointCloud<reve::RadarPoint> radar_scan;
    float v[5];
    while (std::fread(v, sizeof(float), 5, f) == 5) {
        reve::RadarPoint p;
        p.x = v[0];
        p.y = v[1];
        p.z = v[2];
        p.intensity = v[3];
        p.doppler = v[4];
        radar_scan.push_back(p);
    }
    std::fclose(f);

    // the node names the type through radar_ego_velocity_estimation:: (:574)
    const radar_ego_velocity_estimation::RadarEgoVelocityEstimatorConfig config = node_settings();
    reve::RadarEgoVelocityEstimator radar_ego_velocity;
    radar_ego_velocity.configure(config);
    if (argc == 4) radar_ego_velocity.setSeed(std::strtoull(argv[3], nullptr, 0));

    // the inlier scan straight into the PointXYZI cloud the node registers (its `src`)
    Vector3 v_r, sigma_v_r;
    pcl::PointCloud<pcl::PointXYZI>::Ptr src(new pcl::PointCloud<pcl::PointXYZI>);
    const bool ok = radar_ego_velocity.estimate(radar_scan, v_r, sigma_v_r, *src);
    // and once more into a cloud of the scan's own point type: the same points, Doppler kept
    pcl::PointCloud<reve::RadarPoint> inlier_radar_scan;
    Vector3 v2, s2;
    radar_ego_velocity.estimate(radar_scan, v2, s2, inlier_radar_scan);
    if (inlier_radar_scan.size() != src->size() || v2 != v_r || s2 != sigma_v_r) {
        std::fprintf(stderr, "the two estimates differ\n");
        return 1;
    }

    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) {
        std::perror(argv[2]);
        return 2;
    }
    const int32_t head[2] = {ok ? 1 : 0, (int32_t)src->points.size()};
    std::fwrite(head, sizeof(int32_t), 2, o);
    std::fwrite(v_r.data(), sizeof(double), 3, o);
    std::fwrite(sigma_v_r.data(), sizeof(double), 3, o);
    for (size_t i = 0; i < src->points.size(); ++i) {
        const pcl::PointXYZI& p = src->points[i];
        const float w[4] = {p.x, p.y, p.z, p.intensity};
        std::fwrite(w, sizeof(float), 4, o);
    }
    std::fclose(o);
    return 0;
}
