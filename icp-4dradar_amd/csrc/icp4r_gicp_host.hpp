// icp4r_gicp_host.hpp — the host stages of a fast_gicp LsqRegistration on the device that the generalized
// ICP (icp4r_gicp.cpp, which defines them) and the voxelized one (icp4r_vgicp.cpp) share: parameter
// checks, the start of a registration up to both clouds' covariances, the iteration loop with its
// active-pair checks, the fitness pass and results, and the single-pair entry over host buffers.
#pragma once

#include <hip/hip_runtime.h>

#include <functional>

#include "icp4r/icp4r_gicp.h"
#include "icp4r_batch.hpp"
#include "icp4r_host.hpp"
#include "icp4r_internal.hpp"

namespace icp4r_gicp_host {

int check_params(const icp4r_gicp_params* p);
// the kernels' KParams of a registration with these parameters (getFitnessScore's default range)
int kparams(const icp4r_gicp_params& gp, icp4r::KParams* kp);

// The device arrays of a batch into a (everything but a.kp); ICP4R_E_INVALID for a malformed batch.
int pair_args(const icp4r_batch* b, icp4r_result* results, icp4r::PairArgs& a);

// What a registration's stages share.
struct Work {
    icp4r_pipe::Plan pl;
    icp4r::WorkArgs w;
    icp4r::GicpArgs g;
    int mn = 1, mm = 1;  // the largest source / target, at least 1
    bool indexed = false;  // the target's index for the nearest-neighbour passes is built
    icp4r_host::EventPair* be = nullptr;
};

// Sizes the workspace, then queues: validation and X := guess * src, x0 := guess, λ := -1, the slice
// counters' reset, and the k-NN covariances of both clouds (g.cov_src / g.cov_tgt).  nn_index: the
// target's index is left built for nearest-neighbour passes even where the covariances did not need it.
int begin(icp4r_ctx* ctx, const icp4r::PairArgs& a, int npairs, int max_n, int max_m, const icp4r_gicp_params& gp,
          bool nn_index, hipStream_t st, Work& k);
// step(it) queues iteration it; every few iterations the number of pairs still iterating lands in pinned
// host memory, read one check behind, and the loop ends early at zero.
int iterate(icp4r_ctx* ctx, const Work& k, int npairs, int max_iterations, hipStream_t st,
            const std::function<int(int)>& step);
// getFitnessScore (first_nn: no nearest-neighbour pass ran before it), the result rows, the aligned clouds.
int end(icp4r_ctx* ctx, const icp4r::PairArgs& a, Work& k, int npairs, bool first_nn, hipStream_t st);

// One pair from host buffers through a batch entry: stages the clouds, calls run(batch, device result,
// stream), copies the result and the aligned cloud back.  who: the entry's name in error messages.
int align_host(icp4r_ctx* ctx, const float* src, int32_t n, int32_t src_stride_bytes, const float* tgt, int32_t m,
               int32_t tgt_stride_bytes, const float* guess, icp4r_result* out, float* aligned_out,
               int32_t out_stride_bytes, const char* who,
               const std::function<int(const icp4r_batch&, icp4r_result*, hipStream_t)>& run);

}  // namespace icp4r_gicp_host
