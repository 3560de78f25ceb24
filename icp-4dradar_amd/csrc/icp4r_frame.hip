// icp4r_frame.hip — the kernels around a frame's iterations: init_kernel, fitness_prep_kernel, finish_kernel and
// the test hook rot_f32_kernel, with their launches.
#include "icp4r_fold.hpp"

namespace icp4r {

// ---------------------------------------------------------------------------------------------
// init_kernel: one workgroup per pair.
// WG threads per pair: 256 for batches (HBM-bound there), 1024 for a few pairs, whose validation
// passes are latency-bound rounds of loads (C5's 65k-point map: 16 rounds of 256 x 16 -> 4)
template <int kInitWG>
__global__ __launch_bounds__(kInitWG) void init_kernel(PairArgs a, WorkArgs w) {
    __shared__ float Tg[16];
    __shared__ int ident;
    const int p = xcd_remap(blockIdx.x, gridDim.x);
    const int tid = threadIdx.x;
    const int n = a.src_n[p], m = a.tgt_n[p];
    const float4* src = a.src + a.src_off[p];
    const float4* tgt = a.tgt + a.tgt_off[p];
    PairState& st = w.state[p];
    if (tid < 16) Tg[tid] = a.guess ? a.guess[(int64_t)p * 16 + tid] : ((tid % 5 == 0) ? 1.0f : 0.0f);
    __syncthreads();
    if (tid == 0) {
        bool id = true;
        for (int k = 0; k < 16; ++k) id = id && (Tg[k] == ((k % 5 == 0) ? 1.0f : 0.0f));
        ident = id ? 1 : 0;
    }
    __syncthreads();
    // One pass over the source: validated and written transformed (transformCloud(input, guess)) in
    // the same read — X of a pair found invalid below is never read.  Counts above the workspace
    // stride are not copied (too_big below marks the pair invalid).  kInitPer points per thread in
    // flight, every load of a round before its stores.
    constexpr int kInitPer = 4;
    float4* X = w.X + (int64_t)p * w.x_stride;
    const bool id = ident != 0;
    const int nc = min(n, (int)w.x_stride);
    int bad = 0;
    // coordinates beyond 1e17 could square into an overflowing (inf) distance, which PCL rejects: such
    // a pair never skips pass A's distance check (PairState::sums_ok = -1)
    constexpr float kBig = 1e17f;
    int big = 0;
    // (the target is only validated: 16 points per thread in flight — a scan-to-map target of 65k
    // points had taken 64 dependent rounds of 1024, ~65 us of a single registration)
    // (and its bounding box, for the Morton index of a large target: w.tbb)
    constexpr int kTgtPer = 16;
    float bl[3] = {INFINITY, INFINITY, INFINITY}, bh[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i0 = 0; i0 < m; i0 += kInitWG * kTgtPer) {
        float4 t[kTgtPer];
#pragma unroll
        for (int e = 0; e < kTgtPer; ++e) t[e] = tgt[min(i0 + e * kInitWG + tid, m - 1)];
#pragma unroll
        for (int e = 0; e < kTgtPer; ++e) {  // (a clamped duplicate of point m - 1 changes no extent)
            bad |= !(isfinite(t[e].x) && isfinite(t[e].y) && isfinite(t[e].z));
            big |= fmaxf(fabsf(t[e].x), fmaxf(fabsf(t[e].y), fabsf(t[e].z))) > kBig;
            bl[0] = fminf(bl[0], t[e].x); bl[1] = fminf(bl[1], t[e].y); bl[2] = fminf(bl[2], t[e].z);
            bh[0] = fmaxf(bh[0], t[e].x); bh[1] = fmaxf(bh[1], t[e].y); bh[2] = fmaxf(bh[2], t[e].z);
        }
    }
    if (w.tbb) {
        __shared__ float bred[kInitWG / 64][6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // (DPP)
            bl[k] = wave_minf(bl[k]);
            bh[k] = wave_maxf(bh[k]);
        }
        if ((tid & 63) == 0)
            for (int k = 0; k < 3; ++k) {
                bred[tid >> 6][k] = bl[k];
                bred[tid >> 6][3 + k] = bh[k];
            }
        __syncthreads();
        if (tid < 6) {
            float v = bred[0][tid];
            for (int q = 1; q < kInitWG / 64; ++q) v = tid < 3 ? fminf(v, bred[q][tid]) : fmaxf(v, bred[q][tid]);
            w.tbb[(int64_t)p * 8 + tid] = v;
        }
    }
    for (int i0 = 0; i0 < n; i0 += kInitWG * kInitPer) {
        float4 v[kInitPer];
#pragma unroll
        for (int e = 0; e < kInitPer; ++e) v[e] = src[min(i0 + e * kInitWG + tid, n - 1)];
#pragma unroll
        for (int e = 0; e < kInitPer; ++e) {
            const int i = i0 + e * kInitWG + tid;
            bad |= !(isfinite(v[e].x) && isfinite(v[e].y) && isfinite(v[e].z));
            float4 o = v[e];
            if (!id) xform_pt(Tg, v[e].x, v[e].y, v[e].z, o.x, o.y, o.z);
            big |= fmaxf(fabsf(o.x), fmaxf(fabsf(o.y), fabsf(o.z))) > kBig;
            if (i < nc) X[i] = o;
        }
    }
    // the pass-scoped state this registration starts from: the pair's miss bitmap and count (cached-
    // neighbour plans) and, by the group's first pair, its work-list counters (plist_n[0..3]: items,
    // queue, part size, the fused order's arrival counter)
    if (w.need) {
        uint32_t* gneed = w.need + (int64_t)p * w.need_stride;
        for (int k = tid; k < w.need_stride; k += kInitWG) gneed[k] = 0u;
    }
    if (tid == 0 && w.miss_cnt) w.miss_cnt[p] = 0;
    if (tid < 4 && p == 0 && w.plist_n) w.plist_n[tid] = 0;
    bad = __syncthreads_or(bad);
    big = __syncthreads_or(big);
    if (tid == 0) {
        mat4_identity(st.T_inc);
        st.prev_mse = DBL_MAX;
        st.similar = 0;
        st.conv_state = 0;
        st.iterations = 0;
        st.ncorr = 0;
        st.sums_ok = big ? -1 : 0;
        st.pending = 0;
        // counts above the batch's declared max_src_n / max_tgt_n would overrun the workspace strides
        const bool too_big = n > w.x_stride || (w.leaf > 0 && m > w.t_stride);
        if (m <= 0 || bad || too_big) {
            // Registration::initCompute fails (no target) -> align returns; final stays identity.
            mat4_identity(st.final_T);
            st.phase = kPhaseInvalid;
            st.status = too_big ? kStatusInvalid : m <= 0 ? kStatusEmpty : kStatusNonFinite;
        } else {
            for (int k = 0; k < 16; ++k) st.final_T[k] = Tg[k];  // final_transformation_ = guess
            st.phase = kPhaseActive;
            st.status = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fitness_prep_kernel: X := final * input (Registration::getFitnessScore / align's output).
// test (cached-neighbour plan): the fitness pass' cached-neighbour test runs here too, by the pair's
// workgroup (pair_cache_test), instead of as nn_cache_test_kernel after it — one read of X, U, nn_t
// and the input per point, no launch of its own.
constexpr int kPrepWG = 256;
constexpr int kPrepRecs = 1024;  // the fitness test's LDS miss records (the fitness pass misses ~1 %)
__global__ __launch_bounds__(kPrepWG) void fitness_prep_kernel(PairArgs a, WorkArgs w, int test) {
    const int p = xcd_remap(blockIdx.x, gridDim.x);
    const PairState& st = w.state[p];
    if (st.phase == kPhaseInvalid) return;
    __shared__ float Tf[16];
    __shared__ uint32_t need[kNeedWords];
    __shared__ int32_t pre[kNeedWords];
    __shared__ float4 lv[kPrepRecs];
    __shared__ uint2 lm[kPrepRecs];
    __shared__ int32_t mcount, wcnt[kPrepWG / 64];
    const int n = a.src_n[p];
    if (threadIdx.x < 16) Tf[threadIdx.x] = st.final_T[threadIdx.x];
    if (test && w.nn_u) {
        for (int k = threadIdx.x; k < (n + 31) >> 5; k += kPrepWG) need[k] = 0u;
        if (threadIdx.x == 0) mcount = 0;
        __syncthreads();
        float T[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) T[q] = Tf[q];
        pair_cache_test<kPrepWG, 4, true>(a, w, p, n, T, need, pre, lv, lm, kPrepRecs, &mcount, wcnt, true);
        return;
    }
    __syncthreads();
    const float4* src = a.src + a.src_off[p];
    float4* X = w.X + (int64_t)p * w.x_stride;
    float* uu = w.nn_u ? w.nn_u + (int64_t)p * w.x_stride : nullptr;
    // (w.seed_next: the fitness pass's seed keys too — see transform_pair)
    const bool seed = w.seed_next && w.corr && a.kp.compute_fitness;
    NNKey* key = w.nn_key + (int64_t)p * w.x_stride;
    const float4* C = w.corr ? w.corr + (int64_t)p * w.x_stride * 2 : nullptr;
    for (int i = threadIdx.x; i < n; i += kPrepWG) {
        const float4 s = src[i];
        float4 o = s;
        xform_pt(Tf, s.x, s.y, s.z, o.x, o.y, o.z);
        if (seed) {
            const float4 t = C[2 * i + 1];
            key[i] = make_key(l2_simple(o.x, o.y, o.z, t.x, t.y, t.z), (uint32_t)key_idx(key[i]));
        }
        if (uu) {  // X still holds the last NN pass's points (a deferred transform never ran), .w = L
            const float4 old = X[i];
            const float2 Lm = move_lu(make_float2(fabsf(old.w), uu[i]), old.x, old.y, old.z, o.x, o.y, o.z);
            o.w = Lm.x;
            uu[i] = Lm.y;
        }
        X[i] = o;
    }
}

// finish_kernel: fitness = mean of d² over d² <= max_range (double), results, aligned output.
constexpr int kFinWG = 256;
__global__ __launch_bounds__(kFinWG) void finish_kernel(PairArgs a, WorkArgs w) {
    const int p = xcd_remap(blockIdx.x, gridDim.x);
    const PairState& st = w.state[p];
    const int n = a.src_n[p];
    const int64_t slot0 = (int64_t)p * w.x_stride;
    const bool have = st.phase != kPhaseInvalid && a.kp.compute_fitness && n > 0;
    // Registration::getFitnessScore: sequential double sum over points with d² <= max_range, in
    // index order, by wave 0 lane 0 over LDS chunks that waves 1..3 stage (double buffer); points
    // beyond max_range contribute +0 (a no-op on the non-negative running sum); the count is an
    // exact integer reduction.  Bit-identical to the reference loop.
    __shared__ double chunk[2][kFoldChunkP];  // (doubles: the fold lane only adds, fold_seq_d)
    __shared__ int32_t fcnt_w[kFinWG / 64];
    __shared__ uint64_t fsum_w[kFinWG / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double fsum = 0.0;
    int fcnt = 0;
    // Exact parallel form of the same sum.  Every term is a float widened to double, so every term is
    // an integer multiple of 2^e, e = the lowest set bit's exponent over the nonzero terms.  When the
    // exact total S is below 2^(e + 53), every partial sum of the non-negative terms is a multiple of
    // 2^e below 2^(e + 53), i.e. a double: the sequential loop never rounds and returns S itself.  S is
    // then an integer sum in units of 2^e (associative), saturated at 2^53; otherwise (a span of more
    // than 53 bits between the smallest term's last bit and the total) the sequential fold below runs.
    // Batches of at least kFinExactMaxPairs pairs keep the sequential fold only: their chains overlap
    // across the pairs, and the exact attempt measured slower there (C3: 43 -> 63 us per batch; a
    // pair whose span test fails pays both forms).
    constexpr int kFinExactMaxPairs = 256;
    bool exact = false;
    if (have && (int)gridDim.x < kFinExactMaxPairs) {
        constexpr uint64_t kSat = 1ull << 53;
        // the values: in registers for clouds of at most kFinWG * kFinPer points (every load in flight
        // at once, one read of the keys), else re-read per pass; NaN = no point (never in range)
        constexpr int kFinPer = 32;
        const bool reg = n <= kFinWG * kFinPer;
        float v[kFinPer];
        if (reg) {
#pragma unroll
            for (int k = 0; k < kFinPer; ++k) {
                const int i = threadIdx.x + k * kFinWG;
                v[k] = i < n ? key_d2(w.nn_key[slot0 + i]) : __int_as_float(0x7fc00000);
            }
        }
        auto each = [&](auto&& f) {
            if (reg) {
#pragma unroll
                for (int k = 0; k < kFinPer; ++k) f(v[k]);
            } else {
                for (int i = threadIdx.x; i < n; i += kFinWG) f(key_d2(w.nn_key[slot0 + i]));
            }
        };
        int emin = INT_MAX;
        each([&](float d2) {
            const double x = (double)d2;
            if (x <= a.kp.fit_max_range) {
                ++fcnt;
                if (x > 0.0) {
                    const uint64_t b = (uint64_t)__double_as_longlong(x);
                    const int ex = (int)((b >> 52) & 0x7ff);
                    const uint64_t mant = (b & ((1ull << 52) - 1)) | (1ull << 52);
                    emin = min(emin, ex - 1075 + (int)__builtin_ctzll(mant));
                }
            }
        });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            emin = min(emin, __shfl_xor(emin, off, 64));
            fcnt += __shfl_xor(fcnt, off, 64);
        }
        if (lane == 0) {
            fcnt_w[wave] = fcnt;
            fsum_w[wave] = (uint64_t)(uint32_t)emin;
        }
        __syncthreads();
        fcnt = 0;
        emin = INT_MAX;
        for (int k = 0; k < kFinWG / 64; ++k) {
            fcnt += fcnt_w[k];
            emin = min(emin, (int)(uint32_t)fsum_w[k]);
        }
        __syncthreads();  // (fsum_w reused below)
        uint64_t S = 0;
        if (emin != INT_MAX) {
            each([&](float d2) {
                const double x = (double)d2;
                if (x <= a.kp.fit_max_range && x > 0.0) {
                    const uint64_t b = (uint64_t)__double_as_longlong(x);
                    const int ex = (int)((b >> 52) & 0x7ff);
                    const uint64_t mant = (b & ((1ull << 52) - 1)) | (1ull << 52);
                    // x = mant * 2^(ex - 1075); below 2^(emin + 53) iff ex - 1023 - emin <= 52, and then
                    // x / 2^emin = mant >> (emin + 1075 - ex), a shift by at most ctz(mant): exact
                    const uint64_t t = (ex - 1023 - emin <= 52) ? (mant >> (emin + 1075 - ex)) : kSat;
                    S = (S + t < kSat) ? S + t : kSat;
                }
            });
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) S = min(S + __shfl_xor(S, off, 64), kSat);
            if (lane == 0) fsum_w[wave] = S;
            __syncthreads();
            S = 0;
            for (int k = 0; k < kFinWG / 64; ++k) S = min(S + fsum_w[k], kSat);
        }
        if (S < kSat) {
            exact = true;
            fsum = emin == INT_MAX ? 0.0 : ldexp((double)S, emin);
        }
    }
    if (have && !exact) {
        fcnt = 0;
        __syncthreads();  // (fcnt_w reused)
        const int nch = (n + kFoldChunkP - 1) / kFoldChunkP;
        auto fill = [&](int c) {
            const int base = c * kFoldChunkP, len = min(kFoldChunkP, n - base);
            for (int o = threadIdx.x - 64; o < len; o += kFinWG - 64) {
                const float d2 = key_d2(w.nn_key[slot0 + base + o]);  // (d² only: see WorkArgs::nn_key)
                const bool in = (double)d2 <= a.kp.fit_max_range;
                chunk[c & 1][o] = in ? (double)d2 : 0.0;
                fcnt += in ? 1 : 0;
            }
        };
        if (wave >= 1) fill(0);
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            if (wave == 0) {
                if (lane == 0) fsum = fold_seq_d(chunk[c & 1], min(kFoldChunkP, n - c * kFoldChunkP), fsum);
            } else if (c + 1 < nch) {
                fill(c + 1);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) fcnt += __shfl_xor(fcnt, off, 64);
        if (lane == 0) fcnt_w[wave] = fcnt;
        __syncthreads();
        fcnt = 0;
        for (int k = 0; k < kFinWG / 64; ++k) fcnt += fcnt_w[k];
    }
    if (a.aligned && st.phase != kPhaseInvalid) {
        const float4* src = a.src + a.src_off[p];
        const float4* X = w.X + (int64_t)p * w.x_stride;
        float4* out = a.aligned + a.src_off[p];
        for (int i = threadIdx.x; i < n; i += kFinWG) {
            float4 v = X[i];
            v.w = src[i].w;  // intensity copied through
            out[i] = v;
        }
    }
    if (threadIdx.x == 0) {
        Result r;
        for (int k = 0; k < 16; ++k) r.T[k] = st.final_T[k];
        r.fitness = (have && fcnt > 0) ? fsum / fcnt : DBL_MAX;
        r.iterations = st.iterations;
        r.converged = st.phase == kPhaseConverged ? 1 : 0;
        r.status = st.status;
        r.convergence_state = st.conv_state;
        r.n_correspondences = st.ncorr;
        r.reserved = 0;
        a.results[p] = r;
    }
}

// Test hook: the device float Umeyama rotation for k sigma matrices (one thread each).
__global__ void rot_f32_kernel(const float* sigma, float* R, int k) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= k) return;
    float sg[9], Ri[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) sg[e] = sigma[9 * i + e];
    umeyama_rotation_f32_reg(sg, Ri);
#pragma unroll
    for (int e = 0; e < 9; ++e) R[9 * i + e] = Ri[e];
}

hipError_t launch_rot_f32(const float* sigma, float* R, int k, hipStream_t st) {
    hipLaunchKernelGGL(rot_f32_kernel, dim3((k + 63) / 64), dim3(64), 0, st, sigma, R, k);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
hipError_t launch_init(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st) {
    if (npairs < 64)
        hipLaunchKernelGGL(init_kernel<1024>, dim3(npairs), dim3(1024), 0, st, a, w);
    else
        hipLaunchKernelGGL(init_kernel<256>, dim3(npairs), dim3(256), 0, st, a, w);
    return hipGetLastError();
}

hipError_t launch_fitness_prep(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st, int test) {
    if (test && (!w.nn_u || !w.need || !w.miss_cnt || !w.nn_t || !w.sq || !w.tsort || w.x_stride > kCacheMaxN))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fitness_prep_kernel, dim3(npairs), dim3(kPrepWG), 0, st, a, w, test);
    return hipGetLastError();
}

hipError_t launch_finish(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st) {
    hipLaunchKernelGGL(finish_kernel, dim3(npairs), dim3(kFinWG), 0, st, a, w);
    return hipGetLastError();
}

}  // namespace icp4r
