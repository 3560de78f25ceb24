// icp4r_gicp_dev.hpp — device pieces of fast_gicp's LsqRegistration iteration shared by the generalized
// ICP (icp4r_gicp.hip) and the voxelized one (icp4r_vgicp.hip): the slicing of a source cloud, the small
// double linear algebra, one correspondence's terms of the Gauss-Newton system, the fixed-order slice
// reductions, the Levenberg-Marquardt trial and the hand-off of a pair's slice sums to the workgroup
// that finishes last.  (The units are built without relocatable device code: each gets its own copy of
// the functions that are not inlined.)
// gicp_lin_finish / gicp_trial_finish are the last workgroup's work of the two iteration kernels.  The
// voxelized kernels call them; icp4r_gicp.hip's own kernels keep the same statements written out in
// place, because calling these changed their machine code (tools/kernel_asm_diff.py) and a change that
// only adds a registration must leave them as they were.
// !! TWO COPIES.  The λ schedule, the rho decision, the one-by-one trial fallback and the state write-back
// exist here (gicp_lin_finish, gicp_trial_finish) AND in the tails of gicp_lin_kernel / gicp_trial_kernel in
// icp4r_gicp.hip.  A fix to either must be made in both, statement for statement.  Folding GICP's kernels
// onto these functions is the follow-up for the first change that is allowed to alter
// their machine code.
#pragma once

#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icp4r_internal.hpp"

// gicp_so3_exp, gicp_ldlt6 and gicp_make_trial below are ordinary (external, not inlined) __device__
// definitions, kept so because GICP's kernels call them that way and their machine code must not change.
// Two units include this header: that links only while each unit's device code is linked on its own.
#if defined(__CLANG_RDC__)
#error "icp4r_gicp_dev.hpp defines external __device__ functions: with -fgpu-rdc mark them inline first"
#endif

namespace icp4r {

// Eigen-style cofactor inverse of a 3x3 (row-major)
__device__ __forceinline__ void gicp_inv3(const double* m, double* r) {
    const double c0 = m[4] * m[8] - m[5] * m[7];
    const double c1 = m[7] * m[2] - m[8] * m[1];
    const double c2 = m[1] * m[5] - m[2] * m[4];
    const double id = 1.0 / (c0 * m[0] + c1 * m[3] + c2 * m[6]);
    r[0] = c0 * id;
    r[1] = c1 * id;
    r[2] = c2 * id;
    r[3] = (m[5] * m[6] - m[3] * m[8]) * id;
    r[4] = (m[8] * m[0] - m[6] * m[2]) * id;
    r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    r[6] = (m[3] * m[7] - m[4] * m[6]) * id;
    r[7] = (m[6] * m[1] - m[7] * m[0]) * id;
    r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// ---- per-iteration update
constexpr int kGicpSliceWG = 256;  // threads per slice workgroup; a slice is a multiple of it
constexpr int kGicpSliceWaves = kGicpSliceWG / 64;
// (the linearisation's deciding workgroup hands out its copies by thread ranges up to thread 140)
static_assert(kGicpSliceWG >= 128 + 12 && kGicpSliceWG >= kGicpSpec * 12, "slice workgroup too small");

// points per slice and slices of an n-point source: at least one slice (an empty source still
// decides), at most kGicpMaxSlices, a slice a multiple of kGicpSliceWG points
__host__ __device__ __forceinline__ int gicp_slice_pts(int n) {
    const int m = (n + kGicpSliceWG * kGicpMaxSlices - 1) / (kGicpSliceWG * kGicpMaxSlices);
    return kGicpSliceWG * (m > 1 ? m : 1);
}
__host__ __device__ __forceinline__ int gicp_slices(int n) {
    const int s = (n + gicp_slice_pts(n) - 1) / gicp_slice_pts(n);
    return s > 1 ? s : 1;
}

__device__ __forceinline__ void sym_unpack(const double* s, double* m) {
    m[0] = s[0]; m[1] = s[1]; m[2] = s[2];
    m[3] = s[1]; m[4] = s[3]; m[5] = s[4];
    m[6] = s[2]; m[7] = s[4]; m[8] = s[5];
}

// so3_exp (fast_gicp so3.hpp) then Eigen's Quaternion::toRotationMatrix
__device__ void gicp_so3_exp(const double* w, double* R) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double imag, real;
    if (th2 < 1e-10) {
        const double th4 = th2 * th2;
        imag = 0.5 - 1.0 / 48.0 * th2 + 1.0 / 3840.0 * th4;
        real = 1.0 - 1.0 / 8.0 * th2 + 1.0 / 384.0 * th4;
    } else {
        const double th = sqrt(th2), half = 0.5 * th;
        imag = sin(half) / th;
        real = cos(half);
    }
    const double qw = real, qx = imag * w[0], qy = imag * w[1], qz = imag * w[2];
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx;
    const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// (A) x = b, A symmetric positive definite 6x6 (row-major), LDLᵀ without pivoting; L overwrites A's
// strict lower triangle (each A[i][j], i > j, is read once, just before L[i][j] replaces it: the same
// operations in the same order as with a separate L, in a third of the registers — the separate 6x6
// arrays beside the LM state had spilled the iteration kernel to scratch)
__device__ void gicp_ldlt6(double (&A)[36], const double (&b)[6], double (&x)[6]) {
    double D[6], y[6];
    for (int j = 0; j < 6; ++j) {
        double s = A[6 * j + j];
        for (int k = 0; k < j; ++k) s -= A[6 * j + k] * A[6 * j + k] * D[k];
        D[j] = s;
        for (int i = j + 1; i < 6; ++i) {
            double t = A[6 * i + j];
            for (int k = 0; k < j; ++k) t -= A[6 * i + k] * A[6 * j + k] * D[k];
            A[6 * i + j] = D[j] != 0.0 ? t / D[j] : t;  // Eigen: a zero pivot leaves its column undivided
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= A[6 * i + k] * y[k];
        y[i] = s;
    }
    for (int i = 0; i < 6; ++i) y[i] = fabs(D[i]) > DBL_MIN ? y[i] / D[i] : 0.0;  // Eigen's LDLT::solve
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s -= A[6 * k + i] * x[k];
        x[i] = s;
    }
}

__device__ __forceinline__ bool gicp_converged(const double* R, const double* t, double rot_eps, double trans_eps) {
    double m = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) m = fmax(m, 1.0 / rot_eps * fabs(R[3 * r + c] - (r == c ? 1.0 : 0.0)));
    for (int r = 0; r < 3; ++r) m = fmax(m, 1.0 / trans_eps * fabs(t[r]));
    return m < 1.0;
}

// the error eᵀMe of a correspondence with residual e at the transformed source point ta, and with LIN
// its terms of H = Σ JᵀMJ and g = Σ JᵀMe (J = [skew(ta), -I]) and the count, into acc (fast_gicp's
// linearize / compute_error).  Every term is linear in M: a weighted correspondence passes w M.
template <bool LIN>
__device__ __forceinline__ void gicp_terms(const double (&ta)[3], const double (&e)[3], const double (&M)[9],
                                           double* acc) {
    double Me[3];
    for (int r = 0; r < 3; ++r) Me[r] = M[3 * r] * e[0] + M[3 * r + 1] * e[1] + M[3 * r + 2] * e[2];
    if (!LIN) {
        acc[0] += e[0] * Me[0] + e[1] * Me[1] + e[2] * Me[2];
        return;
    }
    acc[27] += e[0] * Me[0] + e[1] * Me[1] + e[2] * Me[2];
    acc[28] += 1.0;
    // J = [skew(Ta), -I] (row k: J[k][0..2] = skew, J[k][3 + k] = -1). The terms with a zero or -1
    // factor of J are left out or reduced to a negation: the same values as the generic JᵀMJ / JᵀMe
    // sums (x + (+-0) = x), in half the operations.
    auto js = [&](int k, int c) -> double {  // skew(Ta)[k][c], k != c
        return k == 0 ? (c == 1 ? -ta[2] : ta[1]) : k == 1 ? (c == 0 ? ta[2] : -ta[0]) : (c == 0 ? -ta[1] : ta[0]);
    };
    double MS[9];  // M skew(Ta)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k0 = c == 0 ? 1 : 0, k1 = c == 2 ? 1 : 2;
            MS[3 * r + c] = M[3 * r + k0] * js(k0, c) + M[3 * r + k1] * js(k1, c);
        }
    int u = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int k0 = r == 0 ? 1 : 0, k1 = r == 2 ? 1 : 2;  // the rows k != r of column r of J
#pragma unroll
        for (int c = r; c < 3; ++c) acc[u++] += js(k0, r) * MS[3 * k0 + c] + js(k1, r) * MS[3 * k1 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[u++] += js(k0, r) * -M[3 * k0 + c] + js(k1, r) * -M[3 * k1 + c];
        acc[21 + r] += js(k0, r) * Me[k0] + js(k1, r) * Me[k1];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = r; c < 3; ++c) acc[u++] += M[3 * r + c];
        acc[24 + r] += -Me[r];
    }
}

// the same for correspondence (a, b) of two float points at transform (R, t)
template <bool LIN>
__device__ __forceinline__ void gicp_point(const float4 sa, const float4 sb, const double (&M)[9], const double* R,
                                           const double* t, double* acc) {
    const double a[3] = {sa.x, sa.y, sa.z};
    double ta[3];
    for (int r = 0; r < 3; ++r) ta[r] = R[3 * r] * a[0] + R[3 * r + 1] * a[1] + R[3 * r + 2] * a[2] + t[r];
    const double e[3] = {(double)sb.x - ta[0], (double)sb.y - ta[1], (double)sb.z - ta[2]};
    gicp_terms<LIN>(ta, e, M, acc);
}

// Σ over the workgroup of each v[k] in a fixed order (butterfly per wave, then the waves in order);
// the sum of v[k] is returned to thread k < NV. red: kGicpSliceWaves * NV doubles of LDS.
template <int NV>
__device__ __forceinline__ double gicp_slice_sum(double (&v)[NV], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    }
    if (lane == 0)
        for (int k = 0; k < NV; ++k) red[wave * NV + k] = v[k];
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < NV)
        for (int q = 0; q < kGicpSliceWaves; ++q) r += red[q * NV + threadIdx.x];
    __syncthreads();  // red is free again
    return r;
}

// The same for the 29 sums of the linearisation, as a transposing reduction: at each step a lane keeps
// half of its values and adds its partner's copy of that half (one shuffle per kept value), so the 32
// padded values take 16 + 8 + 4 + 2 + 1 + 1 shuffles instead of 29 x 6; lanes 2k and 2k + 1 end with
// the wave's sum of value k (another fixed order than the butterfly's). In place in v.
__device__ __forceinline__ double gicp_slice_sum_sys(double (&v)[kGicpSys], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        const bool hi = lane & 32;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const double lo_v = v[k], hi_v = k + 16 < kGicpSys ? v[k + 16] : 0.0;
            v[k] = (hi ? hi_v : lo_v) + __shfl_xor(hi ? lo_v : hi_v, 32, 64);
        }
    }
#pragma unroll
    for (int h = 8, o = 16; h >= 1; h >>= 1, o >>= 1) {
        const bool hi = lane & o;
#pragma unroll
        for (int k = 0; k < h; ++k) {
            const double a = v[k], b = v[k + h];
            v[k] = (hi ? b : a) + __shfl_xor(hi ? a : b, o, 64);
        }
    }
    const double r1 = v[0] + __shfl_xor(v[0], 1, 64);
    const int k = lane >> 1;  // the value this lane pair holds
    if (!(lane & 1) && k < kGicpSys) red[wave * kGicpSys + k] = r1;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < kGicpSys)
        for (int q = 0; q < kGicpSliceWaves; ++q) r += red[q * kGicpSys + threadIdx.x];
    __syncthreads();
    return r;
}

// the LM trial of damping lambda from the system sys at x0 = (R0, t0): delta from (H + λI) d = -g,
// the trial transform delta * x0 (fast_gicp LsqRegistration::step_lm)
__device__ void gicp_make_trial(const double* sys, double lambda, const double* R0, const double* t0, GicpTrial& o) {
    double A[36], nb[6];
    int u = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) A[6 * r + c] = A[6 * c + r] = sys[u++];
    for (int k = 0; k < 6; ++k) A[7 * k] += lambda;
    for (int k = 0; k < 6; ++k) nb[k] = -sys[21 + k];
    double d[6];
    gicp_ldlt6(A, nb, d);
    for (int k = 0; k < 6; ++k) o.d[k] = d[k];
    gicp_so3_exp(d, o.dR);
    o.dt[0] = d[3];
    o.dt[1] = d[4];
    o.dt[2] = d[5];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o.R[3 * r + c] = o.dR[3 * r] * R0[c] + o.dR[3 * r + 1] * R0[3 + c] + o.dR[3 * r + 2] * R0[6 + c];
        o.t[r] = o.dR[3 * r] * t0[0] + o.dR[3 * r + 1] * t0[1] + o.dR[3 * r + 2] * t0[2] + o.dt[r];
    }
    o.lambda = lambda;
}

// Workgroup j of a pair takes its slices j, j + W, j + 2W, ... (W workgroups per pair, fewer for many pairs:
// the slicing, and so every sum, depends on n only; W only spreads the slices over the chip).
// The per-slice sums of one pair reach the workgroup that finishes last (the counter form of the
// hand-off in cdna_hip_programming.md §6 Guideline 16, with write-through sum stores, gicp_publish,
// in place of a release fence in every workgroup): every workgroup waits for its stores and draws a
// ticket; the one drawing nw - 1 acquires, resets the counter for the next launch and returns true
// (in all its threads).
// This block's pair and its index j < W among the pair's workgroups: the W workgroups of a pair on one
// XCD, as blocks are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one), so a pair's
// gathered target data is fetched into one L2, not eight (a speed choice only: nothing depends on it)
__device__ __forceinline__ bool gicp_block(int npairs, int W, int& p, int& j) {
    const int b = blockIdx.x, x = b & 7, r = b >> 3;
    p = (r / W) * 8 + x;
    j = r % W;
    return p < npairs;
}

__device__ __forceinline__ void gicp_publish(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool gicp_last_slice(int32_t* cnt, int nw, int32_t* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int prev = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = prev == nw - 1;
        if (last) {
            __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

// The linearisation's last workgroup of pair p (gicp_last_slice): the ns slices' sums (part) staged in LDS
// by all threads at once (one round trip, not one per slice) and added in slice order, the first LM trials
// solved (step_lm's (H + λI) d = -g, λ, 2λ, 8λ, ...), the system and x0 (g.gs[p]) kept for the trial kernel.
// red: the kernel's reduction scratch, at least kGicpSys doubles, free.
__device__ __forceinline__ void gicp_lin_finish(const GicpArgs& g, int p, int ns, const double* part, double* red) {
    const GicpState& gs = g.gs[p];
    const double *R = gs.R, *t = gs.t;  // (read where they lie: a register copy would go through scratch
                                        // memory to reach gicp_make_trial, which is not inlined)
    __shared__ double stage[kGicpMaxSlices * kGicpSys];
    for (int e = threadIdx.x; e < ns * kGicpSys; e += kGicpSliceWG) stage[e] = part[e];
    __syncthreads();
    double* sys = red;  // (free again)
    if (threadIdx.x < kGicpSys) {
        double sum = 0.0;
        for (int q = 0; q < ns; ++q) sum += stage[q * kGicpSys + threadIdx.x];
        sys[threadIdx.x] = sum;
    }
    __syncthreads();
    GicpCand& gc = g.cand[p];
    const int nt = min(g.spec, g.lm_max_iterations);
    if (threadIdx.x < nt) {
        const int k = threadIdx.x;
        double lambda = gs.lambda, nu = 2.0;
        if (lambda < 0.0) {
            double mx = 0.0;
            const int diag[6] = {0, 6, 11, 15, 18, 20};  // (r, r) in the packed upper triangle
            for (int q = 0; q < 6; ++q) mx = fmax(mx, fabs(sys[diag[q]]));
            lambda = g.lm_init * mx;
        }
        for (int q = 0; q < k; ++q) {
            lambda = nu * lambda;
            nu = 2 * nu;
        }
        GicpTrial tr;
        gicp_make_trial(sys, lambda, R, t, tr);
        gc.c[k] = tr;
    }
    if (threadIdx.x == 63) {  // (independent of nt: gicp_spec = 0 runs every trial one by one from it)
        double lambda = gs.lambda;
        if (lambda < 0.0) {
            double mx = 0.0;
            const int diag[6] = {0, 6, 11, 15, 18, 20};
            for (int q = 0; q < 6; ++q) mx = fmax(mx, fabs(sys[diag[q]]));
            lambda = g.lm_init * mx;
        }
        gc.lambda0 = lambda;
    }
    if (threadIdx.x >= 64 && threadIdx.x < 64 + kGicpSys) gc.sys[threadIdx.x - 64] = sys[threadIdx.x - 64];
    if (threadIdx.x >= 128 && threadIdx.x < 140) {
        const int q = threadIdx.x - 128;
        if (q < 9) gc.R0[q] = R[q];
        else gc.t0[q - 9] = t[q - 9];
    }
}

// The trial kernel's last workgroup of pair p: the nt speculative trials' errors (part, ns slices) summed
// in slice order, then the decision (accept, converge on a rejected step, or raise λ); in the rare case
// every speculative trial was rejected the further trials run one by one over all slices — slice_err(q,
// R, t, e) adds this thread's share of slice q's error at (R, t) to e[0] — each summed slice by slice
// exactly as the speculative ones; then x0, λ and the pair's state are written.
template <class SliceErr>
__device__ __forceinline__ void gicp_trial_finish(const GicpArgs& g, PairState& st, int p, int ns, int nt, int it,
                                                  const double* part, double* red, SliceErr slice_err) {
    __shared__ double err[kGicpSpec];
    __shared__ double x0[12];   // the transform after this iteration
    __shared__ GicpTrial cur;   // the last trial decided on
    __shared__ double lam, nuv;
    __shared__ int32_t stop;    // 1 accepted, 2 converged on a rejected step, 0 none yet
    const GicpCand& gc = g.cand[p];
    {
        __shared__ double stage[kGicpMaxSlices * kGicpSpec];  // (as in the linearisation)
        for (int e = threadIdx.x; e < ns * kGicpSpec; e += kGicpSliceWG) stage[e] = part[e];
        __syncthreads();
        if (threadIdx.x < nt) {
            double t = 0.0;
            for (int q = 0; q < ns; ++q) t += stage[q * kGicpSpec + threadIdx.x];
            err[threadIdx.x] = t;
        }
    }
    __syncthreads();
    const double y0 = gc.sys[27];
    // rho = (y0 - yi) / dᵀ(λd - g)
    auto decide = [&](double yi) {
        const double lambda = cur.lambda;
        double den = 0.0;
        for (int k = 0; k < 6; ++k) den += cur.d[k] * (lambda * cur.d[k] - gc.sys[21 + k]);
        const double rho = (y0 - yi) / den;
        if (rho < 0) {
            if (gicp_converged(cur.dR, cur.dt, g.rot_eps, g.trans_eps)) {
                stop = 2;
            } else {
                lam = nuv * lambda;
                nuv = 2 * nuv;
            }
        } else {
            for (int k = 0; k < 9; ++k) x0[k] = cur.R[k];
            for (int k = 0; k < 3; ++k) x0[9 + k] = cur.t[k];
            lam = lambda * fmax(1.0 / 3.0, 1 - pow(2 * rho - 1, 3));
            stop = 1;
        }
    };
    if (threadIdx.x == 0) {
        for (int k = 0; k < 9; ++k) x0[k] = gc.R0[k];
        for (int k = 0; k < 3; ++k) x0[9 + k] = gc.t0[k];
        stop = 0;
        nuv = 2.0;
        lam = gc.lambda0;  // (== gc.c[0].lambda when trials were solved up front)
        for (int k = 0; k < nt && !stop; ++k) {
            cur = gc.c[k];
            decide(err[k]);
        }
    }
    __syncthreads();
    for (int k = nt; k < g.lm_max_iterations; ++k) {
        if (stop) break;
        __syncthreads();  // every thread read stop
        if (threadIdx.x == 0) gicp_make_trial(gc.sys, lam, gc.R0, gc.t0, cur);
        __syncthreads();
        double tot = 0.0;
        for (int q = 0; q < ns; ++q) {
            double e[1] = {0.0};
            slice_err(q, cur.R, cur.t, e);
            tot += gicp_slice_sum(e, red);
        }
        if (threadIdx.x == 0) decide(tot);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    GicpState& gs = g.gs[p];
    st.ncorr = (int)gc.sys[28];
    st.iterations = it;  // nr_iterations_ = i
    gs.lambda = lam;
    for (int k = 0; k < 9; ++k) gs.R[k] = x0[k];
    for (int k = 0; k < 3; ++k) gs.t[k] = x0[9 + k];
    // final_transformation_ = x0.cast<float>() (column-major)
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) st.final_T[4 * c + r] = (float)x0[3 * r + c];
        st.final_T[12 + r] = (float)x0[9 + r];
        st.final_T[4 * r + 3] = 0.0f;
    }
    st.final_T[15] = 1.0f;
    if (!stop) {
        st.phase = kPhaseFailed;  // step_lm returned false: "lm not converged!!", break
    } else if (gicp_converged(cur.dR, cur.dt, g.rot_eps, g.trans_eps)) {
        st.phase = kPhaseConverged;
        st.conv_state = 2;
    } else if (it + 1 >= g.max_iterations) {
        st.conv_state = 1;
    }
}

// the grid of an iteration kernel: W workgroups per pair (about `grid` in all; a single pair: one per
// slice) for pairs of at most max_n source points, pairs padded to whole rounds of the 8 XCDs
__host__ __forceinline__ void gicp_iter_grid(int npairs, int max_n, int grid, int& W, unsigned& blocks) {
    const int ns = gicp_slices(max_n);
    const int per = grid / npairs;
    W = per < 1 ? 1 : per > ns ? ns : per;
    blocks = (unsigned)W * ((npairs + 7) / 8 * 8);
}

}  // namespace icp4r
