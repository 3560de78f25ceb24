// reve_compat.hpp — header-only C++ facade: reve::RadarEgoVelocityEstimator over the icp4r C ABI
// (include/icp4r/icp4r_reve.h states the contract and its departures from reve).
//
// Drop-in for the first step of the reference node's frame (radar_odometry.cpp:328, configured at
// :574-611): a maintainer includes <icp4r/reve_compat.hpp> instead of reve's estimator header, links
// libicp4r.so, and config_init stays textually unchanged.  The estimator takes a
// point cloud instead of a ROS message: a pcl::PointCloud (points, clear(), push_back()) whose points
// have x, y, z, intensity and doppler members (the ColoRadar layout the node converts to, :540-563).  v_r and
// sigma_v_r are any type indexed with [] (Eigen::Vector3d, std::array<double, 3>).  The inlier cloud
// keeps the input's points, in input order, when it has the same point type; another point type (the
// node's PointXYZI `src`) gets x, y, z and intensity.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "icp4r/icp4r_reve.h"
#include "icp4r/pcl_compat.hpp"

namespace reve {

// The settings of config_init, same member names.
struct RadarEgoVelocityEstimatorConfig {
    double min_dist = 0.25, max_dist = 100, min_db = 0;
    double elevation_thresh_deg = 60, azimuth_thresh_deg = 60;
    double filter_min_z = -3, filter_max_z = 3;
    double doppler_velocity_correction_factor = 1.0;
    double thresh_zero_velocity = 0.05, allowed_outlier_percentage = 0.25;
    double sigma_zero_velocity_x = 0.025, sigma_zero_velocity_y = 0.025, sigma_zero_velocity_z = 0.025;
    double sigma_offset_radar_x = 0.05, sigma_offset_radar_y = 0.025, sigma_offset_radar_z = 0.05;
    double max_sigma_x = 0.2, max_sigma_y = 0.2, max_sigma_z = 0.2;
    double max_r_cond = 1000;
    bool use_cholesky_instead_of_bdcsvd = true;
    bool use_ransac = true;
    double outlier_prob = 0.4, success_prob = 0.9999;
    int N_ransac_points = 3;
    double inlier_thresh = 0.15;
    bool use_odr = true;
    double sigma_v_d = 0.125, min_speed_odr = 4.0;
    double model_noise_offset_deg = 2.0, model_noise_scale_deg = 10.0;
};

// The 5-float point the estimator reads (ColoRadar's x, y, z, intensity, doppler).
struct RadarPoint {
    float x = 0.f, y = 0.f, z = 0.f, intensity = 0.f, doppler = 0.f;
};

class RadarEgoVelocityEstimator {
  public:
    RadarEgoVelocityEstimator() { icp4r_reve_params_default(&params_); }

    // reve: configure(config) copies the settings
    bool configure(RadarEgoVelocityEstimatorConfig config) {
        config_ = config;
        const uint64_t seed = params_.seed;
        const int32_t use_z = params_.use_z_filter;
        icp4r_reve_params_default(&params_);
        params_.seed = seed;
        params_.use_z_filter = use_z;
        params_.min_dist = config.min_dist;
        params_.max_dist = config.max_dist;
        params_.min_db = config.min_db;
        params_.elevation_thresh_deg = config.elevation_thresh_deg;
        params_.azimuth_thresh_deg = config.azimuth_thresh_deg;
        params_.filter_min_z = config.filter_min_z;
        params_.filter_max_z = config.filter_max_z;
        params_.doppler_velocity_correction_factor = config.doppler_velocity_correction_factor;
        params_.thresh_zero_velocity = config.thresh_zero_velocity;
        params_.allowed_outlier_percentage = config.allowed_outlier_percentage;
        params_.sigma_zero_velocity_x = config.sigma_zero_velocity_x;
        params_.sigma_zero_velocity_y = config.sigma_zero_velocity_y;
        params_.sigma_zero_velocity_z = config.sigma_zero_velocity_z;
        params_.sigma_offset_radar_x = config.sigma_offset_radar_x;
        params_.sigma_offset_radar_y = config.sigma_offset_radar_y;
        params_.sigma_offset_radar_z = config.sigma_offset_radar_z;
        params_.max_sigma_x = config.max_sigma_x;
        params_.max_sigma_y = config.max_sigma_y;
        params_.max_sigma_z = config.max_sigma_z;
        params_.max_r_cond = config.max_r_cond;
        params_.use_cholesky_instead_of_bdcsvd = config.use_cholesky_instead_of_bdcsvd ? 1 : 0;
        params_.use_ransac = config.use_ransac ? 1 : 0;
        params_.outlier_prob = config.outlier_prob;
        params_.success_prob = config.success_prob;
        params_.N_ransac_points = config.N_ransac_points;
        params_.inlier_thresh = config.inlier_thresh;
        params_.use_odr = config.use_odr ? 1 : 0;
        params_.sigma_v_d = config.sigma_v_d;
        params_.min_speed_odr = config.min_speed_odr;
        params_.model_noise_offset_deg = config.model_noise_offset_deg;
        params_.model_noise_scale_deg = config.model_noise_scale_deg;
        return true;
    }

    // not in reve: the hypothesis stream (reve seeds from random_device) and the optional z limits
    void setSeed(uint64_t seed) { params_.seed = seed; }
    void setUseZFilter(bool on) { params_.use_z_filter = on ? 1 : 0; }
    const icp4r_reve_result& result() const { return result_; }
    const RadarEgoVelocityEstimatorConfig& config() const { return config_; }

    // estimate(radar_scan, v_r, sigma_v_r, inlier_radar_scan): true iff the estimate succeeded; the inlier
    // cloud is filled either way
    template <typename CloudIn, typename Vec3, typename CloudOut>
    bool estimate(const CloudIn& radar_scan, Vec3& v_r, Vec3& sigma_v_r, CloudOut& inlier_radar_scan) {
        const size_t n = radar_scan.points.size();
        std::vector<float> rec(5 * n + 5);
        std::vector<uint8_t> mask(n + 1);
        for (size_t i = 0; i < n; ++i) {
            const auto& p = radar_scan.points[i];
            rec[5 * i + 0] = p.x;
            rec[5 * i + 1] = p.y;
            rec[5 * i + 2] = p.z;
            rec[5 * i + 3] = p.intensity;
            rec[5 * i + 4] = p.doppler;
        }
        const int rc = icp4r_reve_estimate(icp4r::thread_context(), rec.data(), (int32_t)n, &params_, &result_, mask.data());
        if (rc != ICP4R_OK && rc != ICP4R_E_EMPTY)
            throw std::runtime_error(std::string("icp4r_reve_estimate: ") + icp4r_last_error());
        for (int k = 0; k < 3; ++k) {
            v_r[k] = result_.v[k];
            sigma_v_r[k] = result_.sigma[k];
        }
        inlier_radar_scan.clear();
        using PointIn = typename std::decay<decltype(radar_scan.points[0])>::type;
        using PointOut = typename std::decay<decltype(inlier_radar_scan.points[0])>::type;
        for (size_t i = 0; i < n; ++i) {
            if (!mask[i]) continue;
            if constexpr (std::is_same<PointIn, PointOut>::value) {
                inlier_radar_scan.push_back(radar_scan.points[i]);
            } else {
                PointOut q;
                q.x = radar_scan.points[i].x;
                q.y = radar_scan.points[i].y;
                q.z = radar_scan.points[i].z;
                q.intensity = radar_scan.points[i].intensity;
                inlier_radar_scan.push_back(q);
            }
        }
        return rc == ICP4R_OK && result_.success != 0;
    }

  private:
    RadarEgoVelocityEstimatorConfig config_;
    icp4r_reve_params params_;
    icp4r_reve_result result_ = {};
};

}  // namespace reve

// the node names the config through this namespace (radar_odometry.cpp:574)
namespace radar_ego_velocity_estimation {
using RadarEgoVelocityEstimatorConfig = reve::RadarEgoVelocityEstimatorConfig;
}
