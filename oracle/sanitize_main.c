/* Host-only sanitizer driver for the oracles (TEST INFRASTRUCTURE): ASan + UBSan over the ICP
 * oracle's kd-tree build/search, both Umeyama paths, the error paths and the fitness pass; the GICP
 * oracle's covariances and alignments; the ego-velocity and map oracles. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "ego_oracle.h"
#include "gicp_oracle.h"
#include "icp_oracle.h"
#include "map_oracle.h"

static float frand(unsigned* s) {
    *s = *s * 1103515245u + 12345u;
    return ((*s >> 8) & 0xFFFF) / 65535.0f;
}

/* GICP oracle: the covariances under every regularisation at n = 1 (one point), 12 (fewer than k) and
 * 300, and small alignments: plain, a gate that rejects every correspondence, no LM trial, no
 * iteration. */
static int gicp_checks(void) {
    enum { N = 300 };
    float* tgt = malloc(sizeof(float) * 4 * N);
    float* src = malloc(sizeof(float) * 4 * N);
    double* cov = malloc(sizeof(double) * 9 * N);
    unsigned s = 7;
    for (int i = 0; i < N; ++i) { /* a floor and a wall, 1 cm noise */
        const float u = 10.0f * frand(&s), v = 10.0f * frand(&s), e = 0.01f * (frand(&s) - 0.5f);
        tgt[4 * i] = u;
        tgt[4 * i + 1] = i % 2 ? v : e;
        tgt[4 * i + 2] = i % 2 ? e : v;
        tgt[4 * i + 3] = 0.0f;
        src[4 * i] = tgt[4 * i] + 0.05f;
        src[4 * i + 1] = tgt[4 * i + 1] - 0.03f;
        src[4 * i + 2] = tgt[4 * i + 2] + 0.02f;
        src[4 * i + 3] = 0.0f;
    }
    const int ns[3] = {1, 12, N};
    for (int reg = 0; reg <= 4; ++reg)
        for (int q = 0; q < 3; ++q) {
            gicp_oracle_covariances(tgt, ns[q], 20, reg, cov);
            /* (one point: a zero scatter matrix, which no regularisation may turn into NaN) */
            for (int t = 0; t < 9 * ns[q]; ++t)
                if (isnan(cov[t])) return 20 + reg;
        }
    free(cov);
    gicp_oracle_params p;
    gicp_oracle_result r;
    gicp_oracle_params_default(&p);
    p.k = 5;
    if (gicp_oracle_align(src, N, tgt, N, NULL, &p, &r) != 0 || !r.converged || r.n_valid != N) return 30;
    if (gicp_oracle_align(src, 12, tgt, 15, NULL, &p, &r) != 0) return 31; /* fewer points than k = 20 next */
    p.k = 20;
    if (gicp_oracle_align(src, 12, tgt, 15, NULL, &p, &r) != 0) return 32;
    p.k = 5;
    p.max_correspondence_distance = 1e-4; /* shorter than every correspondence */
    if (gicp_oracle_align(src, N, tgt, N, NULL, &p, &r) != 0 || r.n_valid != 0 || r.iterations != 0) return 33;
    gicp_oracle_params_default(&p);
    p.k = 5;
    p.lm_max_iterations = 0;
    if (gicp_oracle_align(src, N, tgt, N, NULL, &p, &r) != 0 || !r.lm_failed || r.converged || r.iterations != 0) return 34;
    gicp_oracle_params_default(&p);
    p.k = 5;
    p.max_iterations = 0;
    if (gicp_oracle_align(src, N, tgt, N, NULL, &p, &r) != 0 || r.n_valid != 0 || r.converged) return 35;
    if (gicp_oracle_align(src, N, tgt, 0, NULL, &p, &r) != -2) return 36;
    free(src);
    free(tgt);
    return 0;
}

/* ego and map oracles: the parse, the sine RANSAC and the split of a small scan; a sector query and
 * pointAssociateToMap over a small map */
static int ego_map_checks(void) {
    enum { N = 200 };
    float* rec = malloc(sizeof(float) * 5 * N);
    float* feat = malloc(sizeof(float) * 4 * N);
    unsigned s = 11;
    for (int i = 0; i < N; ++i) {
        const float x = 5.0f + 60.0f * frand(&s), y = 40.0f * (frand(&s) - 0.5f), z = 6.0f * (frand(&s) - 0.5f);
        const float d = sqrtf(x * x + y * y + z * z);
        rec[5 * i] = x;
        rec[5 * i + 1] = y;
        rec[5 * i + 2] = z;
        rec[5 * i + 3] = frand(&s);
        rec[5 * i + 4] = -(3.0f * x + 0.5f * y) / d + 0.02f * (frand(&s) - 0.5f); /* ego velocity (3, 0.5, 0) */
    }
    ego_features(rec, N, feat);
    if (ego_hyp_index(1234u, 3, N) < 0 || ego_hyp_index(1234u, 3, N) >= N) return 40;
    const int it = (int)(0.2 * N);
    double A = 0.0, b = 0.0, V[3];
    double* scores = malloc(sizeof(double) * it);
    int32_t best_h = -1;
    const double best = ego_fit_sine_ransac(feat, N, it, 0.5, 0x1CB4D12A5EEDull, &A, &b, scores, &best_h);
    if (!(best > 0.0) || best_h < 0 || best_h >= it) return 41;
    uint8_t* mask = malloc(N);
    const int32_t nst = ego_split_lsq(feat, N, A, b, 0.2, mask, V);
    if (nst <= 0 || nst > N) return 42;
    if (ego_split_lsq(feat, N, A, b, 0.2, NULL, V) != nst) return 43;
    free(scores);
    free(mask);

    float* map = malloc(sizeof(float) * 4 * N);
    float* moved = malloc(sizeof(float) * 4 * N);
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < 4; ++k) map[4 * i + k] = rec[5 * i + k];
    const double R[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {1.0, 2.0, 3.0};
    oracle_associate_to_map(map, N, R, t, moved);
    const float center[3] = {0.0f, 0.0f, 0.0f}, ahead[3] = {1.0f, 0.0f, 0.0f};
    const float heading = oracle_calc_heading(center, ahead);
    int64_t* kept = malloc(sizeof(int64_t) * N);
    const int64_t nk = oracle_sector_search(map, N, 4, center, 80.0f, heading, kept);
    if (nk < 0 || nk > N) return 44;
    for (int64_t i = 0; i < nk; ++i)
        if (!oracle_sector_keep(map + 4 * kept[i], center, 80.0f, heading)) return 45;
    if (!(oracle_calc_dist(map, moved) >= 0.0f)) return 46;
    if (oracle_sector_search(map, 0, 4, center, 80.0f, heading, kept) != 0) return 47;
    free(rec); free(feat); free(map); free(moved); free(kept);
    return 0;
}

int main(void) {
    enum { N = 700, M = 650 };
    float* src = malloc(sizeof(float) * 4 * N);
    float* tgt = malloc(sizeof(float) * 4 * M);
    unsigned s = 1;
    for (int i = 0; i < M; ++i)
        for (int k = 0; k < 4; ++k) tgt[4 * i + k] = 80.0f * frand(&s) - 40.0f;
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < 4; ++k) src[4 * i + k] = tgt[4 * (i % M) + k] + 0.05f * (frand(&s) - 0.5f);
    oracle_params p;
    oracle_result r;
    float* out = malloc(sizeof(float) * 4 * N);
    for (int num = 0; num < 2; ++num)
        for (int nn = 0; nn < 2; ++nn) {
            oracle_params_default(&p);
            p.numerics = num;
            p.nn = nn;
            p.max_iterations = 5;
            if (oracle_align(src, N, 4, tgt, M, 4, NULL, &p, &r, out, NULL) != 0) return 1;
        }
    oracle_params_default(&p);
    p.huber_delta = 0.5;
    p.numerics = 1;
    if (oracle_align(src, N, 4, tgt, M, 4, NULL, &p, &r, NULL, NULL) != 0) return 2;
    if (oracle_align(src, N, 4, tgt, 0, 4, NULL, &p, &r, NULL, NULL) != -2) return 3;
    if (oracle_align(src, 2, 4, tgt, M, 4, NULL, &p, &r, NULL, NULL) != -3) return 4;
    /* reciprocal correspondences: the scan of the moved source for every candidate's target (the
     * source wraps round the target, so sources i and i + M compete and the rule rejects some) */
    oracle_params_default(&p);
    p.use_reciprocal_correspondences = 1;
    p.max_iterations = 5;
    if (oracle_align(src, N, 4, tgt, M, 4, NULL, &p, &r, out, NULL) != 0) return 7;
    if (r.n_correspondences <= 0 || r.n_correspondences >= N) return 8;
    if (oracle_align(src, 2, 4, tgt, M, 4, NULL, &p, &r, NULL, NULL) != -3) return 9;
    int32_t* idx = malloc(sizeof(int32_t) * N);
    float* d2 = malloc(sizeof(float) * N);
    if (oracle_nearest(src, N, 4, tgt, M, 4, 0, idx, d2) != 0) return 5;
    double f = oracle_fitness(src, N, 4, tgt, M, 4, r.T, 1e300, 0);
    if (!isfinite(f)) return 6;
    free(src); free(tgt); free(out); free(idx); free(d2);
    int rc = gicp_checks();
    if (rc) return rc;
    rc = ego_map_checks();
    if (rc) return rc;
    printf("ok\n");
    return 0;
}
