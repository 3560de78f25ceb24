// icp4r_nn.hpp — what the searches and the updates share (and with them solo_kernel and the fitness prep): the wave
// reduction, the correspondence record, the query / miss / cache records with the bounds L and U, and the
// work-list builder that nn_order_kernel runs and fold_update_kernel / fold_update_res_kernel fuse.  Device-inline
// helpers, structs and constants only: no kernel, no launch.
#pragma once

#include "icp4r_common.hpp"

namespace icp4r {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double huber_w(float d2, double delta) {
    const double r = sqrt((double)d2);
    return r <= delta ? 1.0 : delta / r;
}

// Correspondence records (PCL numerics): per source point, in source-index order (the fold order),
// two float4 at corr + (p*x_stride + i)*2: {s.xyz (the transformed source point searched with),
// w (Huber weight, 1 unweighted)}, {d.xyz (its nearest target), d² (float, as FLANN returned it)}.
// Written by the pruned NN kernel's tail, or by corr_kernel after a brute-force pass.
__device__ __forceinline__ void write_corr(const WorkArgs& w, const PairArgs& a, int p, int i, float sx, float sy,
                                           float sz, NNKey k, const float4* tgt) {
    float4* C = w.corr + ((int64_t)p * w.x_stride + i) * 2;
    const float d2 = key_d2(k);
    const float4 t = tgt[key_idx(k)];
    const float wt = a.kp.huber_delta < INFINITY ? (float)huber_w(d2, a.kp.huber_delta) : 1.0f;
    C[0] = make_float4(sx, sy, sz, wt);
    C[1] = make_float4(t.x, t.y, t.z, d2);
}

constexpr float kCacheMargin = 1.0e-4f;
constexpr int kNeedWords = kCacheMaxN / 32;  // bitmap words per pair (one bit per Morton position)
// miss_cnt[p]: the pass' misses, | kMissUnranked when the test left them unplaced (the pair's miss list
// sq / sm and bitmap, for the search to place) instead of in rank order in qv / qm
constexpr int32_t kMissUnranked = 1 << 30;
constexpr int32_t kMissCount = kMissUnranked - 1;

// nn_t[i].w packs the NN's sorted target position (bits 0..13) and the query's sorted source position
// (bits 14..27): the test reads one record for the miss bitmap's bit and for the search record it
// writes (sq / sm: the next search's seed is that target position, no index lookup).  Sizes:
// <= kCacheMaxN = 2^14 sources, <= 8192 targets on the batched plan.
__device__ __forceinline__ uint32_t nt_tpos(float w) { return __float_as_uint(w) & kNtIdxMask; }
__device__ __forceinline__ uint32_t nt_pos(float w) { return __float_as_uint(w) >> kNtPosShift; }

// A missed query's search record, appended to its pair's miss list at slot k (in the order the
// test found them): {X.xyz, U} and {its index | its NN's sorted target position << 14, its sorted
// position}.  The search stages these by rank instead of gathering X, U and a seed per query.
__device__ __forceinline__ void put_miss(const WorkArgs& w, int p, int k, uint32_t sp, int i, float x, float y,
                                         float z, float U, uint32_t tpos) {
    const int64_t slot = (int64_t)p * w.x_stride + k;
    w.sq[slot] = make_float4(x, y, z, U);
    // (one 8-B store: stored as two dwords, the second was merged with the LDS record's into a flat
    // store that every miss of the fused test paid)
    *reinterpret_cast<uint64_t*>(&w.sm[slot]) = (uint64_t)((uint32_t)i | (tpos << kNtPosShift)) | ((uint64_t)sp << 32);
}

// Slot of this lane's record in an append list shared by the workgroup (ctr: an LDS counter): one
// LDS atomic per wave.  Every lane of the wave must call it.
__device__ __forceinline__ int wave_append(bool flag, int32_t* ctr) {
    const uint64_t mask = __ballot(flag);
    if (mask == 0) return -1;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(ctr, __builtin_popcountll(mask));
    base = __builtin_amdgcn_readfirstlane(base);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    return flag ? base + (int)rank : -1;
}

// Bounds on the second-nearest distance of X_i (L in X_i.w, U in nn_u[i]):
//  L (.x): lower bound on |X_i - t_k| for every target k other than the NN — the cache test's;
//  U (.y): upper bound on the second-nearest distance — the next search's initial pruning bound.
// From the second-smallest d² a search saw (every other target has float d² >= sec; the true
// distance is within sqrt(d²)(1 -/+ 3u)), rounded outwards by 1e-6 (>> the sqrt's own rounding).
__device__ __forceinline__ float2 lu_from_sec(float sec_d2) {
    const float r = sqrtf(sec_d2);
    return make_float2(r * 0.999999f, r * 1.000001f);
}

// The bounds after X_i moved from o to v (float points): L - |v - o|, U + |v - o|, roundings covered.
__device__ __forceinline__ float2 move_lu(float2 lu, float ox, float oy, float oz, float vx, float vy, float vz) {
    const float dx = vx - ox, dy = vy - oy, dz = vz - oz;
    const float d = sqrtf(dx * dx + dy * dy + dz * dz) * 1.00001f;
    return make_float2(fmaxf((lu.x - d) * 0.999999f, 0.0f), (lu.y + d) * 1.000001f);
}

// Lazy source cloud (WorkArgs::lazy_x, PairState::pending): L is never negative (move_lu clamps at 0,
// lu_from_sec scales a square root), so the sign bit of a stored L marks a point that the search
// re-wrote after a silent tail — it is at the newer state already.  Every reader of a stored L takes
// fabsf.
constexpr uint32_t kLazyFlag = 0x80000000u;
__device__ __forceinline__ bool l_flagged(float L) { return (__float_as_uint(L) & kLazyFlag) != 0u; }

__device__ __forceinline__ bool cache_hit(float L, float dj2) {
    return L * L * (1.0f - kCacheMargin) > dj2 * (1.0f + kCacheMargin);
}

__device__ __forceinline__ bool pass_wants(int phase, int fitness_pass) {
    return fitness_pass ? (phase != kPhaseInvalid) : (phase == kPhaseActive);
}

constexpr int kOrderBuckets = 32;
constexpr int kPartBits = 10;  // work item = pair << kPartBits | part (parts of >= 64 misses)
static_assert(kCacheMaxN / 64 <= (1 << kPartBits), "part field");

struct OrderShared {
    int32_t bcnt[kOrderBuckets], boff[kOrderBuckets];
    unsigned long long tot;
};

// The work list of a pass, built by WG threads of one workgroup: by nn_order_kernel, or (FUSED) by
// the last workgroup of the fold_update_kernel launch that ran the pass's cached-neighbour test,
// from the per-pair work words (owork) the other workgroups published — written and read with
// agent-scope (L1-bypassing, write-through) accesses only, so no cache can hold a stale copy.
template <int WG, bool FUSED>
__device__ __forceinline__ void order_items_body(const PairArgs& a, const WorkArgs& w, int npairs, int fitness_pass,
                                                 int all, int ncu, OrderShared& sh) {
    const int tid = threadIdx.x;
    if (tid < kOrderBuckets) sh.bcnt[tid] = 0;
    if (tid == 0) sh.tot = 0;
    __syncthreads();
    auto work_load = [&](int p) -> int {
        if (FUSED) return __hip_atomic_load(w.owork + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kMissCount;
        return !pass_wants(w.state[p].phase, fitness_pass) ? 0 : all ? a.src_n[p] : (w.miss_cnt[p] & kMissCount);
    };
    // the thread's first kOrderReg pairs' work loaded once, all in flight (the three passes below
    // had each waited out their loads: one dependent round trip per pass)
    constexpr int kOrderReg = 4;
    int wreg[kOrderReg];
#pragma unroll
    for (int k = 0; k < kOrderReg; ++k) wreg[k] = tid + k * WG < npairs ? work_load(tid + k * WG) : 0;
    auto work = [&](int p) -> int {
        const int k = (p - tid) / WG;
        return k < kOrderReg ? wreg[k] : work_load(p);
    };
    if (!all && w.part_size > 0) {  // the pass' total work, for the part size below
        unsigned long long t = 0;
        for (int p = tid; p < npairs; p += WG) t += (unsigned long long)work(p);
        t = wave_sum(t);
        if ((tid & 63) == 0) atomicAdd(&sh.tot, t);
    }
    __syncthreads();
    int32_t* bcnt = sh.bcnt;
    int32_t* boff = sh.boff;
    const unsigned long long tot_s = sh.tot;
    // a heavy pair's misses are cut into parts of part_size (first pass: one part, all queries), so
    // the few slowly converging pairs with thousands of misses spread over several CUs
    // (at least part_size, and large enough that the pass has about 2 items per CU: a part costs a
    // target staging, so only the heavy tail of a light pass is worth cutting)
    constexpr unsigned long long kIpc = 1;  // the work list's target items per CU (round 6: 1 +0.6 % over 2; 3, 4 slower)
    const int ps = (!all && w.part_size > 0) ? max(w.part_size, (int)((tot_s + kIpc * ncu - 1) / (kIpc * ncu))) : (1 << 30);
    auto heavy_parts = [&](int c) { return (c + ps - 1) / ps; };
    auto heavy_size = [&](int c, int k) { return min(ps, c - k * ps); };
    for (int p = tid; p < npairs; p += WG) {
        const int c = work(p);
        if (w.ticks) w.ticks[32 + p] = (uint64_t)c;  // debug: this pass' work per pair (tools/experiments/miss_hist.py)
        if (c <= 0) continue;
        for (int k = 0, np = heavy_parts(c); k < np; ++k) atomicAdd(&bcnt[31 - __builtin_clz((uint32_t)heavy_size(c, k))], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int b = kOrderBuckets - 1; b >= 0; --b) {
            boff[b] = run;
            run += bcnt[b];
        }
        *w.plist_n = run;
        *w.queue = 0;
        w.plist_n[2] = ps == (1 << 30) ? 0 : ps;  // nn_lds_kernel: misses per part (0: whole pairs)
    }
    __syncthreads();
    for (int p = tid; p < npairs; p += WG) {
        const int c = work(p);
        if (c > 0)
            for (int k = 0, np = heavy_parts(c); k < np; ++k)
                w.plist[atomicAdd(&boff[31 - __builtin_clz((uint32_t)heavy_size(c, k))], 1)] = (p << kPartBits) | k;
    }
}
// (order_items_body: inlined where a call would spill the caller's live registers — fold_update_res_kernel
// takes its kernel arguments' addresses otherwise)
template <int WG, bool FUSED>
__device__ void order_items(const PairArgs& a, const WorkArgs& w, int npairs, int fitness_pass, int all, int ncu,
                            OrderShared& sh) {
    order_items_body<WG, FUSED>(a, w, npairs, fitness_pass, all, ncu, sh);
}

}  // namespace icp4r
