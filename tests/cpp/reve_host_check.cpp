// reve_host_check — the host code behind icp4r_reve_draw and icp4r_reve_ransac_iterations
// (csrc/icp4r_reve_math.hpp, the code the library entries wrap and the kernel calls), built with
// -fsanitize=address,undefined and run as a program (tests/test_reve.py).  The draw against a literal
// three-step Fisher-Yates over a std::vector for every n_valid in [3, 48] and for 8192, 65 hypotheses
// and four seeds each; the hypothesis count at the node's settings and two others; the Jacobi condition
// number and the cofactor solve on a diagonal, a rotated and a singular matrix.  Prints
// "<draws> draws, <m> mismatches".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "icp4r_reve_math.hpp"

namespace {

int check_draw(uint64_t seed, int32_t k, int32_t m) {
    std::vector<int32_t> a((size_t)m);  // exact size: an index past the end is a heap overflow
    for (int32_t i = 0; i < m; ++i) a[(size_t)i] = i;
    int32_t want[3];
    for (int i = 0; i < 3; ++i) {
        const uint64_t r = icp4r_reve::splitmix64(seed + 3ull * (uint64_t)k + (uint64_t)i);
        const int32_t j = i + (int32_t)(r % (uint64_t)(m - i));
        std::swap(a[(size_t)i], a[(size_t)j]);
        want[i] = a[(size_t)i];
    }
    int32_t got[3] = {-1, -1, -1};
    icp4r_reve::draw(seed, k, m, got);
    int bad = 0;
    for (int i = 0; i < 3; ++i) bad += got[i] != want[i] || got[i] < 0 || got[i] >= m;
    bad += got[0] == got[1] || got[0] == got[2] || got[1] == got[2];
    return bad ? 1 : 0;
}

bool close(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fabs(b); }

}  // namespace

int main() {
    long draws = 0, mismatches = 0;
    const uint64_t seeds[4] = {0ull, 0x4E7E5EEDull, 0xFFFFFFFFFFFFFFFBull, 0x4E7E5EEDull + (7ull << 32)};
    for (int32_t m = 3; m <= 49; ++m) {
        const int32_t mm = m == 49 ? 8192 : m;
        for (uint64_t seed : seeds)
            for (int32_t k = 0; k < 65; ++k) {
                mismatches += check_draw(seed, k, mm);
                ++draws;
            }
    }
    // the count: 37 at the node's settings, and the formula elsewhere; no count where it is not a number
    if (icp4r_reve::ransac_iterations(0.9999, 0.4) != 37) ++mismatches;
    if (icp4r_reve::ransac_iterations(0.99, 0.5) != (int32_t)(unsigned)(std::log(0.01) / std::log(1.0 - 0.125))) ++mismatches;
    if (icp4r_reve::ransac_iterations(0.0, 0.4) != 0) ++mismatches;
    if (icp4r_reve::ransac_iterations(1.0, 0.4) != -1) ++mismatches;   // log(0) = -inf
    if (icp4r_reve::ransac_iterations(0.9999, 1.0) != -1) ++mismatches;  // log(1) = 0: inf or NaN
    if (icp4r_reve::ransac_iterations(NAN, 0.4) != -1) ++mismatches;
    // cond and solve
    const double diag[6] = {4.0, 0.0, 0.0, 2.0, 0.0, 0.5};
    if (icp4r_reve::jacobi_cond(diag) != 8.0) ++mismatches;
    // R diag(9, 3, 1) R^T with R a rotation about z by 30 degrees then about x by 20: cond = 9
    const double cz = std::cos(0.5235987755982988), sz = std::sin(0.5235987755982988);
    const double cx = std::cos(0.3490658503988659), sx = std::sin(0.3490658503988659);
    const double R[3][3] = {{cz, -sz, 0.0}, {cx * sz, cx * cz, -sx}, {sx * sz, sx * cz, cx}};
    const double lam[3] = {9.0, 3.0, 1.0};
    double M[3][3] = {};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int q = 0; q < 3; ++q) M[i][j] += R[i][q] * lam[q] * R[j][q];
    const double m6[6] = {M[0][0], M[0][1], M[0][2], M[1][1], M[1][2], M[2][2]};
    if (!close(icp4r_reve::jacobi_cond(m6), 9.0, 1e-12)) ++mismatches;
    const double x[3] = {1.0, -2.0, 0.5};
    double g[3], Ri[9], v[3];
    for (int i = 0; i < 3; ++i) g[i] = M[i][0] * x[0] + M[i][1] * x[1] + M[i][2] * x[2];
    icp4r_reve::solve3(m6, g, Ri, v);
    for (int i = 0; i < 3; ++i)
        if (!close(v[i], x[i], 1e-12)) ++mismatches;
    // a planar triple: lambda_min = 0 exactly on a diagonal matrix -> cond = inf, never accepted
    const double planar[6] = {2.0, 0.0, 0.0, 1.0, 0.0, 0.0};
    if (std::fabs(icp4r_reve::jacobi_cond(planar)) < 1000.0) ++mismatches;
    std::printf("%ld draws, %ld mismatches\n", draws, mismatches);
    return mismatches ? 1 : 0;
}
