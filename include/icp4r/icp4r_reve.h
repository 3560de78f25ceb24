/*
 * icp4r_reve.h — C ABI of the 3D Doppler ego-velocity estimator with inlier scans: the first step of
 * every radar_odometry frame, on the GPU.
 *
 * Replaces, in src/radar_odometry.cpp of the reference:
 *
 *     radar_ego_velocity.estimate(radar_data_msg, v_r, sigma_v_r, inlier_radar_scan)   // :328
 *     inlier scan -> PointXYZI cloud `src`                                             // :329-342
 *     config_init(config)                                                              // :574-611
 *
 * reve::RadarEgoVelocityEstimator is not part of the reference tree; this header restates it.  Input:
 * the 5-float record [x, y, z, intensity, doppler] (snr_db = intensity, v_doppler_mps = doppler,
 * :540-563).  All arithmetic is double on the widened float inputs, unfused.
 *
 *  1. Valid targets.  r = sqrt((x x + y y) + z z); point i is valid iff min_dist < r < max_dist,
 *     intensity > min_db, |atan2(y, x)| < azimuth_thresh_deg pi/180 and
 *     |atan2(sqrt(x x + y y), z) - pi/2| < elevation_thresh_deg pi/180 (pi/180 = (pi / 180) in double,
 *     the product thresh * (pi / 180)).  A comparison with NaN is false.  Valid targets keep input
 *     order; d_i = doppler * doppler_velocity_correction_factor; h_i = (x / r, y / r, z / r).
 *  2. Fewer than 3 valid targets: no estimate (empty inlier set, success = 0).
 *  3. Standstill.  a = ascending |d_i| over the valid targets, n = (size_t)(count (1 -
 *     allowed_outlier_percentage)), median = a[n].  median < thresh_zero_velocity: v = 0, sigma =
 *     sigma_zero_velocity_*, inliers = the valid targets with |d_i| < thresh_zero_velocity, success = 1.
 *     (a[n] < t iff more than n valid targets have |d_i| < t: the device counts, it does not sort.)
 *  4. RANSAC.  y_i = -d_i; iterations = (unsigned)(log(1 - success_prob) / log(1 - pow(1 -
 *     outlier_prob, 3))) hypotheses (icp4r_reve_ransac_iterations; 37 at the node's settings).
 *     Hypothesis k takes three distinct valid targets (icp4r_reve_draw) a, b, c:
 *         M_ij = (h_a,i h_a,j + h_b,i h_b,j) + h_c,i h_c,j,  g_i = (h_a,i y_a + h_b,i y_b) + h_c,i y_c,
 *     cond = lambda_max / lambda_min of M by 8 sweeps of cyclic Jacobi ((0,1), (0,2), (1,2); a zero
 *     off-diagonal element is skipped; theta = (M_qq - M_pp) / (2 M_pq), t = sign(theta) / (|theta| +
 *     sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c); rejected unless fabs(cond) < max_r_cond;
 *     v = M^-1 g with the cofactor inverse (first-column cofactors, det, adjugate * (1 / det)) and
 *     v_i = (R_i0 g_0 + R_i1 g_1) + R_i2 g_2.  Its inliers: the valid targets with
 *     |y_i - ((h_i,0 v_0 + h_i,1 v_1) + h_i,2 v_2)| < inlier_thresh.  A hypothesis replaces the best
 *     only with strictly more inliers (from 0): the first maximum wins.
 *     Only + - * / sqrt: a double implementation that follows this order gives equal bits.
 *  5. Refit.  A non-empty best set is solved again, M and g summed over the set (any order: the device
 *     uses a fixed-order tree), the same cond test, the same inverse; e = H v - y,
 *     C_ii = ((e.e) R_ii) / (rows - 3), sigma_i = sqrt(C_ii) + sigma_offset_radar_*.  success iff the
 *     cond test passes and every sigma_i < max_sigma_*; a failed cond test leaves v = sigma = 0.  The
 *     inlier scan is the best set either way (the node ignores the return value, :328).
 *
 * Departures from reve:
 *   - Draws.  reve shuffles with an mt19937 seeded from random_device.  Here hypothesis k's three
 *     indices are a partial Fisher-Yates over the valid list: j_i = i + SplitMix64(seed + 3 k + i) mod
 *     (n_valid - i), i = 0, 1, 2; scan s of a batch uses seed + (s << 32).  Runs are reproducible.
 *   - Non-finite Doppler.  A point whose Doppler is not finite is invalid (reve would hand it to
 *     nth_element).
 *   - Angle precision.  reve takes the two angles with the float atan2 overloads, here they are double:
 *     only a point within a float ulp of a threshold can differ.
 *   - No ODR.  use_odr, min_speed_odr, sigma_v_d and the model_noise_* settings are accepted and have
 *     no effect: v and sigma are the least squares'.  ODR refines only v and sigma, never the scan.
 *   - z limits.  filter_min_z / filter_max_z act (filter_min_z < z < filter_max_z) only when
 *     use_z_filter is 1; it defaults to 0 (it is not known whether reve's estimate() applies them).
 *   - Fixed sample size.  N_ransac_points must be 3, use_ransac non-zero: anything else is
 *     ICP4R_E_INVALID.  use_cholesky_instead_of_bdcsvd is accepted; the solve is the cofactor inverse.
 *   - allowed_outlier_percentage must lie in [0, 1]; an index n >= count (reve would read past the
 *     end) is taken as count - 1.
 *   - At most ICP4R_REVE_MAX_ITERATIONS hypotheses and ICP4R_REVE_MAX_POINTS points per scan
 *     (ICP4R_E_TOO_LARGE beyond).
 *
 * Conventions as icp4r.h: int status returns, icp4r_last_error(), one context per host thread.
 */
#ifndef ICP4R_REVE_H
#define ICP4R_REVE_H

#include <stdint.h>

#include "icp4r.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ICP4R_REVE_MAX_ITERATIONS 256
#define ICP4R_REVE_MAX_POINTS 262144

/* One field per setting of config_init (:576-610), same names; then seed and use_z_filter. */
typedef struct icp4r_reve_params {
    double min_dist, max_dist, min_db;
    double elevation_thresh_deg, azimuth_thresh_deg;
    double filter_min_z, filter_max_z;
    double doppler_velocity_correction_factor;
    double thresh_zero_velocity, allowed_outlier_percentage;
    double sigma_zero_velocity_x, sigma_zero_velocity_y, sigma_zero_velocity_z;
    double sigma_offset_radar_x, sigma_offset_radar_y, sigma_offset_radar_z;
    double max_sigma_x, max_sigma_y, max_sigma_z;
    double max_r_cond;
    double outlier_prob, success_prob;
    double inlier_thresh;
    double sigma_v_d, min_speed_odr, model_noise_offset_deg, model_noise_scale_deg;
    int32_t use_cholesky_instead_of_bdcsvd, use_ransac, N_ransac_points, use_odr;
    uint64_t seed;        /* hypothesis stream (SplitMix64 of seed + 3 k + i)                      */
    int32_t use_z_filter; /* 1: also require filter_min_z < z < filter_max_z                       */
    int32_t reserved[7];
} icp4r_reve_params; /* 272 bytes */

typedef struct icp4r_reve_result {
    double v[3];           /* sensor velocity (y = -doppler: +v_sensor)                             */
    double sigma[3];       /* its standard deviation                                                */
    int32_t n;             /* points in the scan                                                    */
    int32_t n_valid;       /* valid targets (step 1)                                                */
    int32_t n_inliers;     /* points in the inlier scan                                             */
    int32_t iterations;    /* hypotheses drawn (0: fewer than 3 valid targets, or standstill)       */
    int32_t accepted;      /* hypotheses that passed the cond test                                  */
    int32_t best;          /* index of the winning hypothesis, -1 if none                           */
    int32_t zero_velocity; /* 1: the standstill branch                                              */
    int32_t success;       /* what estimate() returns                                               */
    int32_t status;        /* icp4r_status of this scan                                             */
    int32_t reserved;
} icp4r_reve_result; /* 88 bytes */

void icp4r_reve_params_default(icp4r_reve_params* p);

/* Pure host, no device call.  The hypothesis count of step 4 (-1: params NULL or the formula's value
 * is not a number >= 0). */
int32_t icp4r_reve_ransac_iterations(const icp4r_reve_params* params);
/* Pure host, no device call.  The three valid-list indices of hypothesis k: distinct, each below
 * n_valid.  ICP4R_E_INVALID when n_valid < 3 or k < 0. */
int icp4r_reve_draw(uint64_t seed, int32_t k, int32_t n_valid, int32_t out[3]);

/* Many scans, device-resident, asynchronous on hip_stream (NULL = the context's stream): records:
 * device, concatenated 5-float records; off / cnt: device[nscans] (first record, count); max_n:
 * host-known upper bound of cnt[]; results: device[nscans]; inlier_mask: device (one byte per record,
 * same indexing as records: 1 = in the inlier scan) or NULL.  A scan with cnt < 0 or cnt > max_n gets
 * status ICP4R_E_INVALID; its records are not read and its mask bytes not written.  An empty scan gets
 * ICP4R_E_EMPTY. */
int icp4r_reve_batch_device(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt,
                            int32_t nscans, int32_t max_n, const icp4r_reve_params* params,
                            icp4r_reve_result* results, uint8_t* inlier_mask, void* hip_stream);

/* The estimator, then the gate's compaction (icp4r_gate.h) of every scan's inlier points, on one
 * stream with no host round trip: clouds (float4 x, y, z, intensity; 16-B aligned; room for the sum of
 * the counts), pair_off int64[nscans + 1], pair_n int32[nscans + 1] in the packed layout of
 * icp4r_gate.h ([s0, s0, s1, ...]).  inlier_mask: as above, or NULL (the context keeps it).  The scans
 * must lie within the first nscans * max_n records of `records`; a scan that does not is not touched:
 * it packs nothing and its status is ICP4R_E_INVALID, as is a scan with cnt < 0 or cnt > max_n. */
int icp4r_reve_inlier_clouds_batch_device(icp4r_ctx* ctx, const float* records, const int64_t* off,
                                          const int32_t* cnt, int32_t nscans, int32_t max_n,
                                          const icp4r_reve_params* params, icp4r_reve_result* results,
                                          uint8_t* inlier_mask, float* clouds, int64_t* pair_off, int32_t* pair_n,
                                          void* hip_stream);

/* One scan from host records, synchronous.  inlier_mask_out: optional, n bytes. */
int icp4r_reve_estimate(icp4r_ctx* ctx, const float* records, int32_t n, const icp4r_reve_params* params,
                        icp4r_reve_result* out, uint8_t* inlier_mask_out);

/* One scan from host records, synchronous: the result (v, sigma) and the inlier points (xyzi_out: room
 * for n x 4 floats; *n_inliers of them are written, in input order). */
int icp4r_reve_inlier_cloud(icp4r_ctx* ctx, const float* records, int32_t n, const icp4r_reve_params* params,
                            icp4r_reve_result* out, float* xyzi_out, int32_t* n_inliers);

#ifdef __cplusplus
}
#endif

#endif /* ICP4R_REVE_H */
