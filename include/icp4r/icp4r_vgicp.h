/*
 * icp4r_vgicp.h — C ABI of the voxelized generalized ICP: fast_gicp::FastVGICP, the registration
 * fast_gicp ships beside the FastGICP of icp4r_gicp.h for the cost that one pays on a scan-to-map call
 * (an index of the submap and an exact nearest-neighbour pass per iteration).  The target becomes a map
 * of Gaussian voxels; a correspondence is a voxel lookup at the transformed source point.
 *
 * Parity status: UNPINNED by the reference — fast_gicp (koide3/fast_gicp) is not vendored and not in
 * this image.  Parity is to the restatement below, pinned by the numpy twin tests/vgicp_twin.py and
 * known answers (tests/test_vgicp.py, tests/test_vgicp_gpu.py).
 *
 * The algorithm, all in double unless stated:
 *
 *   Covariances.  Source and target covariances come from the k nearest neighbours of each point in
 *   its own cloud, exactly as icp4r_gicp.h computes them (the same kernels, regularisation and n < k
 *   rule).
 *
 *   Voxel map of the target.  The cell of a point p is c = floor(double(p) / resolution) per axis (an
 *   IEEE double division and floor) as a signed integer.  A cell keeps num_points, mean = Σp /
 *   num_points and cov = ΣC_p / num_points.  Both sums run sequentially in ascending target index: the
 *   points are ordered by a stable sort on the cell key and each voxel's run is added from its first
 *   point on, starting from the first term.  Cells are ordered lexicographically by (cx, cy, cz).  A
 *   coordinate outside [-2^20, 2^20) cells does not fit the 3 x 21-bit key: the pair gets
 *   ICP4R_E_INVALID and nothing is written for it (a stated departure: fast_gicp hashes unbounded ints).
 *   Of a covariance the upper triangle is read and summed; the voxel's lower triangle mirrors it.
 *
 *   Offsets.  DIRECT1: (0,0,0).  DIRECT7: (0,0,0), (1,0,0), (-1,0,0), (0,1,0), (0,-1,0), (0,0,1),
 *   (0,0,-1).  DIRECT27: i, j, k in {-1, 0, 1}, x outermost, z innermost.
 *
 *   Per iteration at x0 = (R, t).  Ta = ((R[r][0] a0 + R[r][1] a1) + R[r][2] a2) + t[r], unfused.  Take
 *   the cell of Ta; for each offset in list order, if the neighbouring cell exists (a neighbour outside
 *   the key range does not) that is a correspondence (i, v) with M = (cov_v + R C_i Rᵀ)⁻¹ (the cofactor
 *   inverse, its upper triangle mirrored), e = mean_v - Ta, w = sqrt((double)num_points_v), J =
 *   [skew(Ta), -I].  H = Σ JᵀWJ, g = Σ JᵀWe, y = Σ eᵀWe with W = w M (each element of M times w).  The
 *   sums run per slice of the source (256 or more points, a function of the source size only) in a
 *   fixed order and the slices are added in order, so a pair's result never depends on its batch.
 *   A trial's error is Σ eᵀWe at the trial pose over the same correspondences with the same W: the
 *   linearisation stores each correspondence's voxel (4 bytes per (point, offset)) and the trial
 *   recomputes W from R0.  Everything else is LsqRegistration as icp4r_gicp.h has it: lambda from
 *   lm_init_lambda_factor max|diag H|, the factor-2 growth, at most lm_max_iterations trials, the so3
 *   exponential, the two epsilons, at most max_iterations iterations, pairs that stop individually.
 *   A pair with no correspondence behaves as the gated GICP pair: H = g = 0, ICP4R_OK, converged after
 *   0 iterations at the guess, n_correspondences 0.
 *
 *   Results.  n_correspondences is the number of (i, v) pairs of the last linearisation; the fitness is
 *   Registration::getFitnessScore() by exact nearest neighbour on the target cloud, as GICP.  With
 *   compute_fitness = 0 no nearest-neighbour pass runs (the only index of the target is the one its
 *   k-NN covariances walk).  max_correspondence_distance is accepted and has no effect: VGICP has no
 *   distance gate.
 *
 * Not offered (ICP4R_E_INVALID): NeighborSearchMethod DIRECT_RADIUS, VoxelAccumulationMode
 * ADDITIVE_WEIGHTED and MULTIPLICATIVE.
 */
#ifndef ICP4R_VGICP_H
#define ICP4R_VGICP_H

#include <stdint.h>

#include "icp4r.h"
#include "icp4r_gicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fast_gicp::NeighborSearchMethod */
typedef enum icp4r_vgicp_neighbor_search {
    ICP4R_VGICP_DIRECT1 = 0,
    ICP4R_VGICP_DIRECT7 = 1,
    ICP4R_VGICP_DIRECT27 = 2,
    ICP4R_VGICP_DIRECT_RADIUS = 3 /* refused */
} icp4r_vgicp_neighbor_search;

/* fast_gicp::VoxelAccumulationMode */
typedef enum icp4r_vgicp_accumulation {
    ICP4R_VGICP_ADDITIVE = 0,
    ICP4R_VGICP_ADDITIVE_WEIGHTED = 1, /* refused */
    ICP4R_VGICP_MULTIPLICATIVE = 2     /* refused */
} icp4r_vgicp_accumulation;

typedef struct icp4r_vgicp_params {
    icp4r_gicp_params gicp;     /* every GICP parameter (max_correspondence_distance: no effect)  */
    double voxel_resolution;    /* FastVGICP::setResolution;                      1.0, > 0        */
    int32_t neighbor_search;    /* icp4r_vgicp_neighbor_search;                   DIRECT1         */
    int32_t voxel_accumulation; /* icp4r_vgicp_accumulation;                      ADDITIVE        */
    int32_t reserved[8];
} icp4r_vgicp_params;

void icp4r_vgicp_params_default(icp4r_vgicp_params* p);

/* FastVGICP::align(output[, guess]) for one pair from host buffers; arguments and results as
 * icp4r_gicp_align. */
int icp4r_vgicp_align(icp4r_ctx* ctx, const float* src, int32_t n, int32_t src_stride_bytes, const float* tgt,
                      int32_t m, int32_t tgt_stride_bytes, const float* guess, const icp4r_vgicp_params* params,
                      icp4r_result* out, float* aligned_out, int32_t out_stride_bytes);

/* The same for a device-resident batch (icp4r_batch layout; results[npairs] in device memory), stream
 * ordered on hip_stream (NULL: the context's stream).  Per pair as icp4r_vgicp_align; a pair with a
 * target coordinate outside the key range gets status ICP4R_E_INVALID. */
int icp4r_vgicp_align_batch_device(icp4r_ctx* ctx, const icp4r_batch* batch, const icp4r_vgicp_params* params,
                                   icp4r_result* results, void* hip_stream);

/* fast_gicp's GaussianVoxelMap of one cloud (host buffers).  cov_in: n x 9 doubles (row-major 3x3, the
 * upper triangle is read), or NULL: the k-NN covariances with k and regularization.  Voxel v in
 * lexicographic cell order: coords_out[v][3], num_points_out[v], mean_out[v][3], cov_out[v][9]; any
 * output may be NULL.  *n_voxels is always set; more than cap voxels, or a coordinate outside the key
 * range (then *n_voxels = 0), returns ICP4R_E_INVALID and writes no voxel. */
int icp4r_vgicp_voxel_map(icp4r_ctx* ctx, const float* cloud, int32_t n, int32_t stride_bytes, const double* cov_in,
                          int32_t k, int32_t regularization, double resolution, int32_t cap, int32_t* coords_out,
                          int32_t* num_points_out, double* mean_out, double* cov_out, int32_t* n_voxels);

#ifdef __cplusplus
}
#endif

#endif /* ICP4R_VGICP_H */
