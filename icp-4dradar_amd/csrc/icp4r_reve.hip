// icp4r_reve.hip — the 3D Doppler ego-velocity estimator for gfx950 (include/icp4r/icp4r_reve.h states
// the algorithm and every operation order).
//
// The work per scan is small (37 hypotheses x n tests at the node's settings) and the path is bound by
// passes over the records, so one launch does everything and reads each record from HBM once:
//
//   reve_kernel   one workgroup of kReveWG threads per scan.
//     pass 1  the scan's records -> the valid test -> (x, y, z, doppler) as float4 in LDS (an invalid
//             point's w := NaN), points past kReveLdsPts to a workspace that stays in L2; per 64-point
//             block the number of valid points (one ballot), the standstill count, the xyzi copy the
//             packing reads
//     index   inclusive scan of the block counts: the rank of every valid point, n_valid
//     draw    3 x iterations threads: Fisher-Yates index -> rank -> point (binary search over the
//             blocks, then at most 64 LDS reads)
//     solve   one thread per hypothesis: M, g, Jacobi cond, cofactor solve
//     pass 2  every point against all accepted hypotheses, from LDS: a wave keeps 4 x 64 points'
//             directions in registers and runs through the hypotheses (one ballot per 64 tests); lane a
//             holds hypothesis a's count, one integer LDS add per wave at the end — no float atomics
//     pass 3  the winner's inlier flags (the mask), M and g of the refit in a fixed-order reduction
//             (each thread its points in index order, xor butterfly per wave, waves in order)
//     pass 4  e.e of the refit, the same reduction; thread 0 writes the result row
//
// HBM traffic per record: 20 B read, 1 B mask written (+ 16 B xyzi written when the caller packs).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icp4r/icp4r_reve.h"
#include "icp4r_reve.hpp"
#include "icp4r_reve_math.hpp"

namespace icp4r {

constexpr double kRevePi = 3.14159265358979323846;
constexpr int kReveWaves = kReveWG / 64;
constexpr int kRevePer = 4;  // points per lane of a scoring round

struct RevePt {
    double hx, hy, hz, y, d;
    bool valid;
};

// direction, Doppler and measurement of a stored point (w = NaN: invalid)
__device__ __forceinline__ RevePt reve_point(const float4 q, double factor) {
    RevePt p;
    p.valid = q.w == q.w;
    const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
    const double r = sqrt((x * x + y * y) + z * z);
    p.hx = x / r;
    p.hy = y / r;
    p.hz = z / r;
    p.d = (double)q.w * factor;
    p.y = -p.d;
    return p;
}

__device__ __forceinline__ bool reve_inlier(const RevePt& p, const double v[3], double thresh) {
    const double e = p.y - ((p.hx * v[0] + p.hy * v[1]) + p.hz * v[2]);
    return p.valid && fabs(e) < thresh;
}

// Sums k doubles per thread over the workgroup in a fixed order; the totals are valid in thread 0 only.
template <int K>
__device__ __forceinline__ void reve_reduce(double (&m)[K], double (*red)[10]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m[k] += __shfl_xor(m[k], o, 64);
    }
    __syncthreads();  // red may still be read from the previous reduction
    if (lane == 0)
        for (int k = 0; k < K; ++k) red[wave][k] = m[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int w = 0; w < kReveWaves; ++w) t += red[w][k];
            m[k] = t;
        }
    }
}

__global__ __launch_bounds__(kReveWG) void reve_kernel(ReveArgs a) {
    extern __shared__ float4 spts[];            // a.lds_pts points
    __shared__ int bpre[kReveMaxBlocks];        // valid points per 64-point block, then their inclusive scan
    __shared__ double hv[kReveMaxHyp][3];       // each hypothesis' velocity
    __shared__ int hacc[kReveMaxHyp];           // 1: passed the cond test
    __shared__ int hcnt[kReveMaxHyp];           // its inliers
    __shared__ int pick[3 * kReveMaxHyp];       // the drawn points
    __shared__ double red[kReveWaves][10];
    __shared__ int wsum[kReveWaves];
    __shared__ int s_nzero, s_best, s_accepted, s_ninl, s_ok;
    __shared__ double s_v[3], s_rdiag[3];

    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_raw = a.cnt[s];
    icp4r_reve_result res;
    for (int k = 0; k < 3; ++k) res.v[k] = res.sigma[k] = 0.0;
    res.n = res.n_valid = res.n_inliers = res.iterations = res.accepted = 0;
    res.best = -1;
    res.zero_velocity = res.success = res.status = res.reserved = 0;
    if (n_raw < 0 || n_raw > a.max_n || (a.bad && a.bad[s])) {  // refused: nothing read, nothing written but the row
        if (tid == 0) {
            res.status = ICP4R_E_INVALID;
            a.results[s] = res;
        }
        return;
    }
    const int n = n_raw;
    const int64_t first = a.off[s];
    const int nblk = (n + 63) >> 6;
    float4* spill = a.spill ? a.spill + (int64_t)s * a.spill_stride : nullptr;
    const int lds_pts = a.lds_pts;
    auto load_pt = [&](int i) -> float4 { return i < lds_pts ? spts[i] : spill[i - lds_pts]; };

    if (tid == 0) s_nzero = 0;
    __syncthreads();
    // ---- pass 1
    for (int i0 = wave * 64; i0 < n; i0 += kReveWG) {  // wave-uniform
        const int i = i0 + lane;
        bool valid = false, zero = false;
        if (i < n) {
            const float* r = a.rec + 5 * (first + i);
            const float fx = r[0], fy = r[1], fz = r[2], fi = r[3], fd = r[4];
            const double x = (double)fx, y = (double)fy, z = (double)fz;
            const double xy = x * x + y * y;
            const double rr = sqrt(xy + z * z);
            const double d = (double)fd * a.factor;
            valid = rr > a.min_dist && rr < a.max_dist && (double)fi > a.min_db && fabs(atan2(y, x)) < a.az_lim &&
                    fabs(atan2(sqrt(xy), z) - kRevePi / 2.0) < a.el_lim && fabs((double)fd) <= 1.7976931348623157e308 &&
                    fabs(d) <= 1.7976931348623157e308 && (!a.use_z || (z > a.zmin && z < a.zmax));
            zero = valid && fabs(d) < a.zero_thresh;
            const float4 q = make_float4(fx, fy, fz, valid ? fd : __builtin_nanf(""));
            if (i < lds_pts)
                spts[i] = q;
            else
                spill[i - lds_pts] = q;
            if (a.xyzi) a.xyzi[first + i] = make_float4(fx, fy, fz, fi);
        }
        const unsigned long long bv = __ballot(valid), bz = __ballot(zero);
        if (lane == 0) {
            bpre[i0 >> 6] = __popcll(bv);
            if (bz) atomicAdd(&s_nzero, __popcll(bz));
        }
    }
    __syncthreads();
    // ---- the rank index: inclusive scan of bpre[0, nblk), 4 entries a thread (kReveMaxBlocks = 4 kReveWG)
    {
        int c[4], t = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = 4 * tid + k;
            c[k] = b < nblk ? bpre[b] : 0;
            t += c[k];
        }
        int inc = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int run = inc - t;
        for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = 4 * tid + k;
            run += c[k];
            if (b < nblk) bpre[b] = run;
        }
    }
    __syncthreads();
    const int n_valid = nblk > 0 ? bpre[nblk - 1] : 0;
    const int n_zero = s_nzero;
    res.n = n;
    res.n_valid = n_valid;
    res.status = n > 0 ? ICP4R_OK : ICP4R_E_EMPTY;

    int mode;  // 0: no estimate, 1: standstill, 2: RANSAC
    if (n_valid < 3) {
        mode = 0;
    } else {
        long long nidx = (long long)((double)n_valid * a.keep);
        if (nidx > n_valid - 1) nidx = n_valid - 1;
        mode = (long long)n_zero > nidx ? 1 : 2;
    }
    if (mode == 1) {
        if (a.mask)
            for (int i = tid; i < n; i += kReveWG) {
                const RevePt p = reve_point(load_pt(i), a.factor);
                a.mask[first + i] = p.valid && fabs(p.d) < a.zero_thresh ? 1 : 0;
            }
        if (tid == 0) {
            for (int k = 0; k < 3; ++k) res.sigma[k] = a.sig_zero[k];
            res.n_inliers = n_zero;
            res.zero_velocity = 1;
            res.success = 1;
            a.results[s] = res;
        }
        return;
    }
    const int H = mode == 2 ? a.iterations : 0;
    const uint64_t seed = a.seed + ((uint64_t)s << 32);
    // ---- draw: rank -> point
    if (tid < 3 * H) {
        int32_t out[3];
        icp4r_reve::draw(seed, tid / 3, n_valid, out);
        const int r = out[tid % 3];
        int lo = 0, hi = nblk - 1;  // the first block whose inclusive count exceeds r
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (bpre[mid] > r)
                hi = mid;
            else
                lo = mid + 1;
        }
        int left = r - (lo > 0 ? bpre[lo - 1] : 0);
        int found = lo * 64;
        const int end = min(n, lo * 64 + 64);
        for (int i = lo * 64; i < end; ++i) {
            const float4 q = load_pt(i);
            if (q.w == q.w) {
                if (left == 0) {
                    found = i;
                    break;
                }
                --left;
            }
        }
        pick[tid] = found;
    }
    __syncthreads();
    // ---- solve
    if (tid < H) {
        double m[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
        for (int j = 0; j < 3; ++j) {
            const RevePt p = reve_point(load_pt(pick[3 * tid + j]), a.factor);
            const double t[9] = {p.hx * p.hx, p.hx * p.hy, p.hx * p.hz, p.hy * p.hy, p.hy * p.hz,
                                 p.hz * p.hz, p.hx * p.y,  p.hy * p.y,  p.hz * p.y};
            if (j == 0) {
                for (int k = 0; k < 6; ++k) m[k] = t[k];
                for (int k = 0; k < 3; ++k) g[k] = t[6 + k];
            } else {
                for (int k = 0; k < 6; ++k) m[k] = m[k] + t[k];
                for (int k = 0; k < 3; ++k) g[k] = g[k] + t[6 + k];
            }
        }
        const double cond = icp4r_reve::jacobi_cond(m);
        const bool ok = fabs(cond) < a.max_cond;
        double R[9], v[3];
        icp4r_reve::solve3(m, g, R, v);
        hacc[tid] = ok ? 1 : 0;
        hcnt[tid] = 0;
        for (int k = 0; k < 3; ++k) hv[tid][k] = v[k];
    }
    __syncthreads();
    // ---- the accepted hypotheses moved to the front of hv, in order (pick[a]: hypothesis a's own index)
    if (tid == 0) {
        int na = 0;
        for (int k = 0; k < H; ++k) {
            if (!hacc[k]) continue;
            for (int q = 0; q < 3; ++q) hv[na][q] = hv[k][q];
            pick[na++] = k;
        }
        s_accepted = na;
    }
    __syncthreads();
    const int na = s_accepted;
    // ---- pass 2: every point against every accepted hypothesis.  A wave holds kRevePer x 64 points in
    // registers (an invalid point's y := NaN: never an inlier) and runs through the hypotheses; lane a
    // keeps hypothesis a's count of this wave, added to LDS once at the end.
    for (int c0 = 0; c0 < na; c0 += 64) {  // hypotheses in chunks of 64: one at the node's settings
        const int c1 = min(na, c0 + 64);
        int acc = 0;
        for (int i0 = wave * (64 * kRevePer); i0 < n; i0 += kReveWG * kRevePer) {  // wave-uniform
            double hx[kRevePer], hy[kRevePer], hz[kRevePer], yy[kRevePer];
            bool any = false;
#pragma unroll
            for (int q = 0; q < kRevePer; ++q) {
                const int i = i0 + 64 * q + lane;
                hx[q] = hy[q] = hz[q] = 0.0;
                yy[q] = __builtin_nan("");
                if (i < n) {
                    const RevePt p = reve_point(load_pt(i), a.factor);
                    hx[q] = p.hx;
                    hy[q] = p.hy;
                    hz[q] = p.hz;
                    if (p.valid) yy[q] = p.y;
                    any = any || p.valid;
                }
            }
            if (!__ballot(any)) continue;
            for (int h = c0; h < c1; ++h) {
                const double v0 = hv[h][0], v1 = hv[h][1], v2 = hv[h][2];
                int c = 0;
#pragma unroll
                for (int q = 0; q < kRevePer; ++q) {
                    const double e = yy[q] - ((hx[q] * v0 + hy[q] * v1) + hz[q] * v2);  // reve_inlier's order
                    c += __popcll(__ballot(fabs(e) < a.inlier_thresh));
                }
                acc += lane == h - c0 ? c : 0;
            }
        }
        if (c0 + lane < c1 && acc) atomicAdd(&hcnt[c0 + lane], acc);
    }
    __syncthreads();
    if (tid == 0) {  // the first strict maximum
        int best = -1, bc = 0;
        for (int h = 0; h < na; ++h) {
            if (hcnt[h] > bc) {
                bc = hcnt[h];
                best = h;
            }
        }
        s_best = best;
        s_ninl = bc;
    }
    __syncthreads();
    const int best = s_best;  // its place among the accepted
    res.iterations = H;
    res.accepted = na;
    res.best = best < 0 ? -1 : pick[best];
    res.n_inliers = s_ninl;
    if (best < 0) {
        if (a.mask)
            for (int i = tid; i < n; i += kReveWG) a.mask[first + i] = 0;
        if (tid == 0) a.results[s] = res;
        return;
    }
    // ---- pass 3: the mask, M and g over the best set
    const double vb[3] = {hv[best][0], hv[best][1], hv[best][2]};
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += kReveWG) {
        const RevePt p = reve_point(load_pt(i), a.factor);
        const bool in = reve_inlier(p, vb, a.inlier_thresh);
        if (a.mask) a.mask[first + i] = in ? 1 : 0;
        if (!in) continue;
        m[0] += p.hx * p.hx; m[1] += p.hx * p.hy; m[2] += p.hx * p.hz;
        m[3] += p.hy * p.hy; m[4] += p.hy * p.hz; m[5] += p.hz * p.hz;
        m[6] += p.hx * p.y;  m[7] += p.hy * p.y;  m[8] += p.hz * p.y;
    }
    reve_reduce<9>(m, red);
    if (tid == 0) {
        const double cond = icp4r_reve::jacobi_cond(m);
        double R[9], v[3];
        icp4r_reve::solve3(m, m + 6, R, v);
        s_ok = fabs(cond) < a.max_cond ? 1 : 0;
        for (int k = 0; k < 3; ++k) {
            s_v[k] = v[k];
            s_rdiag[k] = R[4 * k];
        }
    }
    __syncthreads();
    if (!s_ok) {  // workgroup-uniform
        if (tid == 0) a.results[s] = res;
        return;
    }
    // ---- pass 4: e.e
    const double v[3] = {s_v[0], s_v[1], s_v[2]};
    double ee[1] = {0.0};
    for (int i = tid; i < n; i += kReveWG) {
        const RevePt p = reve_point(load_pt(i), a.factor);
        if (!reve_inlier(p, vb, a.inlier_thresh)) continue;
        const double e = ((p.hx * v[0] + p.hy * v[1]) + p.hz * v[2]) - p.y;
        ee[0] += e * e;
    }
    reve_reduce<1>(ee, red);
    if (tid == 0) {
        const double rows3 = (double)(s_ninl - 3);
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            res.v[k] = v[k];
            res.sigma[k] = sqrt((ee[0] * s_rdiag[k]) / rows3) + a.sig_off[k];
            ok = ok && res.sigma[k] < a.sig_max[k];
        }
        res.success = ok ? 1 : 0;
        a.results[s] = res;
    }
}

hipError_t launch_reve(const ReveArgs& a, int nscans, hipStream_t st) {
    if (nscans <= 0) return hipSuccess;
    const size_t lds = (size_t)(a.lds_pts > 0 ? a.lds_pts : 1) * sizeof(float4);
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(reve_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(reve_kernel, dim3(nscans), dim3(kReveWG), lds, st, a);
    return hipGetLastError();
}

}  // namespace icp4r
