// icp4r_reve_math.hpp — the arithmetic of the 3D Doppler ego-velocity estimator that host and device
// share (include/icp4r/icp4r_reve.h states every operation order): the hypothesis draw, the hypothesis
// count, the Jacobi condition number and the cofactor solve.  Plain C++ with no HIP call: the library's
// two pure-host entries wrap the first two, tests/cpp/reve_host_check.cpp runs all of it under the host
// sanitizers.  Only + - * / sqrt (and log / pow in the count): compiled unfused, host and device agree
// bit for bit.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ICP4R_REVE_HD __host__ __device__
#else
#define ICP4R_REVE_HD
#endif

namespace icp4r_reve {

constexpr int kJacobiSweeps = 8;

ICP4R_REVE_HD inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The first three steps of a Fisher-Yates shuffle of 0 .. m - 1 (m >= 3) without the array: step i swaps
// position i with j_i = i + SplitMix64(seed + 3 k + i) mod (m - i); out[i] is what lands at position i.
// The at most six positions that no longer hold their own index are kept in a list.
ICP4R_REVE_HD inline void draw(uint64_t seed, int32_t k, int32_t m, int32_t out[3]) {
    int32_t pos[6], val[6];
    int cnt = 0;
    for (int i = 0; i < 3; ++i) {
        const uint64_t r = splitmix64(seed + 3ull * (uint64_t)(int64_t)k + (uint64_t)i);
        const int32_t j = i + (int32_t)(r % (uint64_t)(m - i));
        int32_t vi = i, vj = j;
        for (int q = 0; q < cnt; ++q) {
            if (pos[q] == i) vi = val[q];
            if (pos[q] == j) vj = val[q];
        }
        out[i] = vj;
        // a[j] = vi, a[i] = vj
        int qi = -1, qj = -1;
        for (int q = 0; q < cnt; ++q) {
            if (pos[q] == i) qi = q;
            if (pos[q] == j) qj = q;
        }
        if (qj < 0) {
            qj = cnt++;
            pos[qj] = j;
        }
        val[qj] = vi;
        if (qi < 0 && i != j) {
            qi = cnt++;
            pos[qi] = i;
        }
        if (i != j) val[qi] = vj;
    }
}

// (unsigned)(log(1 - success_prob) / log(1 - pow(1 - outlier_prob, 3))); -1 where that is no count.
inline int32_t ransac_iterations(double success_prob, double outlier_prob) {
    const double t = log(1.0 - success_prob) / log(1.0 - pow(1.0 - outlier_prob, 3.0));
    if (!(t >= 0.0) || !(t < 2147483648.0)) return -1;
    return (int32_t)(unsigned)t;
}

// One Jacobi rotation that zeroes a_pq; r is the third index.
ICP4R_REVE_HD inline void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (!(apq != 0.0)) return;
    const double theta = (aqq - app) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tp = t * apq;
    app = app - tp;
    aqq = aqq + tp;
    apq = 0.0;
    const double np = c * arp - s * arq;
    const double nq = s * arp + c * arq;
    arp = np;
    arq = nq;
}

// lambda_max / lambda_min of the symmetric M = [m0 m1 m2; m1 m3 m4; m2 m4 m5]: kJacobiSweeps sweeps of
// cyclic Jacobi over (0,1), (0,2), (1,2), then the largest over the smallest diagonal element.
ICP4R_REVE_HD inline double jacobi_cond(const double m[6]) {
    double a00 = m[0], a01 = m[1], a02 = m[2], a11 = m[3], a12 = m[4], a22 = m[5];
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12);  // (p, q) = (0, 1), r = 2
        jacobi_rotate(a00, a22, a02, a01, a12);  // (0, 2), r = 1
        jacobi_rotate(a11, a22, a12, a01, a02);  // (1, 2), r = 0
    }
    double hi = a00, lo = a00;
    if (a11 > hi) hi = a11;
    if (a22 > hi) hi = a22;
    if (a11 < lo) lo = a11;
    if (a22 < lo) lo = a22;
    return hi / lo;
}

// R = M^-1 by cofactors (Eigen 3.3 compute_inverse<Matrix3d>: first-column cofactors, det, the
// adjugate times 1 / det), row-major; v_i = (R_i0 g_0 + R_i1 g_1) + R_i2 g_2.
ICP4R_REVE_HD inline void solve3(const double m[6], const double g[3], double R[9], double v[3]) {
    const double M[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]};
#define ICP4R_REVE_M(i, j) M[3 * (i) + (j)]
    const double c0 = ICP4R_REVE_M(1, 1) * ICP4R_REVE_M(2, 2) - ICP4R_REVE_M(1, 2) * ICP4R_REVE_M(2, 1);
    const double c1 = ICP4R_REVE_M(2, 1) * ICP4R_REVE_M(0, 2) - ICP4R_REVE_M(2, 2) * ICP4R_REVE_M(0, 1);
    const double c2 = ICP4R_REVE_M(0, 1) * ICP4R_REVE_M(1, 2) - ICP4R_REVE_M(0, 2) * ICP4R_REVE_M(1, 1);
    const double det = (c0 * ICP4R_REVE_M(0, 0) + c1 * ICP4R_REVE_M(1, 0)) + c2 * ICP4R_REVE_M(2, 0);
    const double inv = 1.0 / det;
    R[0] = c0 * inv;
    R[1] = c1 * inv;
    R[2] = c2 * inv;
    R[3] = (ICP4R_REVE_M(1, 2) * ICP4R_REVE_M(2, 0) - ICP4R_REVE_M(1, 0) * ICP4R_REVE_M(2, 2)) * inv;
    R[4] = (ICP4R_REVE_M(2, 2) * ICP4R_REVE_M(0, 0) - ICP4R_REVE_M(2, 0) * ICP4R_REVE_M(0, 2)) * inv;
    R[5] = (ICP4R_REVE_M(0, 2) * ICP4R_REVE_M(1, 0) - ICP4R_REVE_M(0, 0) * ICP4R_REVE_M(1, 2)) * inv;
    R[6] = (ICP4R_REVE_M(1, 0) * ICP4R_REVE_M(2, 1) - ICP4R_REVE_M(1, 1) * ICP4R_REVE_M(2, 0)) * inv;
    R[7] = (ICP4R_REVE_M(2, 0) * ICP4R_REVE_M(0, 1) - ICP4R_REVE_M(2, 1) * ICP4R_REVE_M(0, 0)) * inv;
    R[8] = (ICP4R_REVE_M(0, 0) * ICP4R_REVE_M(1, 1) - ICP4R_REVE_M(0, 1) * ICP4R_REVE_M(1, 0)) * inv;
#undef ICP4R_REVE_M
    for (int i = 0; i < 3; ++i) v[i] = (R[3 * i] * g[0] + R[3 * i + 1] * g[1]) + R[3 * i + 2] * g[2];
}

}  // namespace icp4r_reve
