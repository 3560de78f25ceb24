// icp4r_fold.hpp — the sequential fold chains and the fused cached-neighbour test of one pair: what the updates
// and solo_kernel (icp4r_kernels.hip) share with the fitness prep and finish kernels (icp4r_frame.hip).
// Device-inline helpers, structs and constants only: no kernel, no launch.
#pragma once

#include "icp4r_nn.hpp"

namespace icp4r {

// ---------------------------------------------------------------------------------------------
// Sequential folds over an LDS chunk, one lane per chain: acc = acc + f[k] for k in [0, len), in
// that order — exactly the reference loop.  Groups of 32 floats are read 32 elements ahead in two
// explicit register sets (a/b ping-pong) so the chain runs at the dependent-add latency instead of
// waiting on each LDS round trip.  TAcc = float (the float chains) or double (MSE / fitness: the
// float values are widened, as PCL's double accumulators do).
template <typename TAcc>
__device__ __forceinline__ void add_group(TAcc& acc, const float4 (&g)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        acc = acc + (TAcc)g[u].x;
        acc = acc + (TAcc)g[u].y;
        acc = acc + (TAcc)g[u].z;
        acc = acc + (TAcc)g[u].w;
    }
}

__device__ __forceinline__ void load_group(float4 (&g)[8], const float* f) {
#pragma unroll
    for (int u = 0; u < 8; ++u) g[u] = *reinterpret_cast<const float4*>(f + 4 * u);
}

// The last < 32 elements of a chain segment: groups of 8 loaded one group ahead, then up to 7 loaded
// together (a dependent scalar loop would wait out one LDS round trip per element — the panel ends of
// pass B cut segments at arbitrary positions).  f needs no alignment.
template <typename TAcc>
__device__ __forceinline__ TAcc fold_tail(const float* f, int len, TAcc acc) {
    int k = 0;
    if (len >= 4) {
        float a0 = f[0], a1 = f[1], a2 = f[2], a3 = f[3];
        for (; k + 4 <= len; k += 4) {
            const int nx = (k + 8 <= len) ? k + 4 : k;  // the next group, or a harmless re-read
            const float b0 = f[nx], b1 = f[nx + 1], b2 = f[nx + 2], b3 = f[nx + 3];
            __builtin_amdgcn_sched_barrier(0);
            acc = acc + (TAcc)a0;
            acc = acc + (TAcc)a1;
            acc = acc + (TAcc)a2;
            acc = acc + (TAcc)a3;
            a0 = b0;
            a1 = b1;
            a2 = b2;
            a3 = b3;
        }
    }
    const int r = len - k;  // 0..3, loaded together
    const float v0 = f[k], v1 = f[k + (r > 1 ? 1 : 0)], v2 = f[k + (r > 2 ? 2 : 0)];
    if (r > 0) acc = acc + (TAcc)v0;
    if (r > 1) acc = acc + (TAcc)v1;
    if (r > 2) acc = acc + (TAcc)v2;
    return acc;
}

// acc + x.x + x.y + x.z + x.w in that order, each IEEE add as v_add_f32 does it, with acc kept in one
// register (the tied operand): the allocator had used a consumed group register as the running sum,
// then copied the next group into place with 16 v_mov per round.
__device__ __forceinline__ float chain_add4(float acc, const float4& x) {
    asm("v_add_f32 %0, %1, %0\n\t"
        "v_add_f32 %0, %2, %0\n\t"
        "v_add_f32 %0, %3, %0\n\t"
        "v_add_f32 %0, %4, %0"
        : "+v"(acc)
        : "v"(x.x), "v"(x.y), "v"(x.z), "v"(x.w));
    return acc;
}

// A panel chain's step over one chunk row (len <= T floats, T a multiple of 8; 16-B aligned): groups
// of 16 floats in two register sets that trade roles (the next group's four ds_read_b128 issued before
// this group's 16 dependent adds, as long as the LDS round trip; no register copies: one set carried
// into the next round had cost 16 v_mov and a full lgkmcnt wait per 16 adds, ~15 cycles per add
// against ~7), the rest through fold_tail — half fold_seq's registers: the panel fold lanes share
// their waves' allocation with the fillers.
__device__ __forceinline__ float fold_row(const float* f, int len, float acc) {
    int k = 0;
    if (len >= 32) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const float4*>(f + 4 * u);
        for (; k + 32 <= len; k += 32) {
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = *reinterpret_cast<const float4*>(f + k + 16 + 4 * u);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc = chain_add4(acc, a[u]);
            }
            const int nx = (k + 48 <= len) ? k + 32 : k;  // the next group, or a harmless re-read
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const float4*>(f + nx + 4 * u);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc = chain_add4(acc, b[u]);
            }
        }
        if (k + 16 <= len) {  // a holds f[k, k + 16)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc = chain_add4(acc, a[u]);
            }
            k += 16;
        }
    }
    return k < len ? fold_tail<float>(f + k, len - k, acc) : acc;
}

constexpr int kFoldAhead = 2;  // groups of 32 floats in flight ahead of the adds (1 or 2)
template <typename TAcc>
__device__ __forceinline__ TAcc fold_seq(const float* f, int len, TAcc acc) {
    int k = 0;
    if (kFoldAhead >= 2 && len >= 96) {
        // three register groups in rotation, two loads in flight while a group is summed: 6.4-6.7
        // cycles per dependent add on gfx950 vs 7.6-9.0 with one group ahead (tools/experiments/chain_bench.hip)
        float4 a[8], b[8], c[8];
        load_group(a, f);
        load_group(b, f + 32);
        for (; k + 96 <= len; k += 96) {
            // the loads past this round re-read group 0 harmlessly when nothing follows
            const int n1 = (k + 128 <= len) ? k + 96 : 0, n2 = (k + 160 <= len) ? k + 128 : 0;
            load_group(c, f + k + 64);
            __builtin_amdgcn_sched_barrier(0);
            add_group(acc, a);
            load_group(a, f + n1);
            __builtin_amdgcn_sched_barrier(0);
            add_group(acc, b);
            load_group(b, f + n2);
            __builtin_amdgcn_sched_barrier(0);
            add_group(acc, c);
        }
        // a, b hold [k, k + 32) and [k + 32, k + 64) when they exist
        if (k + 32 <= len) {
            add_group(acc, a);
            k += 32;
            if (k + 32 <= len) {
                add_group(acc, b);
                k += 32;
            }
        }
        return k < len ? fold_tail<TAcc>(f + k, len - k, acc) : acc;
    }
    if (len >= 32) {
        float4 a[8], b[8];
        load_group(a, f);
        int apos = 0;  // where `a` was loaded from
        // sched_barrier: keep each prefetch ahead of the adds it overlaps (the scheduler would
        // otherwise sink the loads down to their first use and expose the LDS latency again)
        for (; k + 64 <= len; k += 64) {
            load_group(b, f + k + 32);
            __builtin_amdgcn_sched_barrier(0);
            add_group(acc, a);
            apos = (k + 96 <= len) ? k + 64 : k;  // next group, or a harmless re-read
            load_group(a, f + apos);
            __builtin_amdgcn_sched_barrier(0);
            add_group(acc, b);
        }
        if (k + 32 <= len) {
            if (apos != k) load_group(a, f + k);
            add_group(acc, a);
            k += 32;
        }
    }
    return k < len ? fold_tail<TAcc>(f + k, len - k, acc) : acc;
}

// fold_seq with the chain switched at element xa (a wave-uniform multiple of 32): groups before it go
// to acc, the rest to acc2 — a panel end of pass B inside a chunk (the fillers padded the ending
// panel to xa with +0).  One three-group rotation over the whole row: the loads stay in flight across
// the switch, which is a scalar branch per group.
template <typename TAcc>
__device__ __forceinline__ void fold_seq_switch(const float* f, int len, int xa, TAcc& acc, TAcc& acc2) {
    xa = __builtin_amdgcn_readfirstlane(xa);
    auto add = [&](int k, const float4 (&g)[8]) __attribute__((always_inline)) {
        if (k < xa)
            add_group(acc, g);
        else
            add_group(acc2, g);
    };
    int k = 0;
    if (len >= 96) {
        float4 a[8], b[8], c[8];
        load_group(a, f);
        load_group(b, f + 32);
        for (; k + 96 <= len; k += 96) {
            const int n1 = (k + 128 <= len) ? k + 96 : 0, n2 = (k + 160 <= len) ? k + 128 : 0;
            load_group(c, f + k + 64);
            __builtin_amdgcn_sched_barrier(0);
            add(k, a);
            load_group(a, f + n1);
            __builtin_amdgcn_sched_barrier(0);
            add(k + 32, b);
            load_group(b, f + n2);
            __builtin_amdgcn_sched_barrier(0);
            add(k + 64, c);
        }
        if (k + 32 <= len) {
            add(k, a);
            k += 32;
            if (k + 32 <= len) {
                add(k, b);
                k += 32;
            }
        }
    } else {
        for (; k + 32 <= len; k += 32) {
            float4 a[8];
            load_group(a, f + k);
            add(k, a);
        }
    }
    if (k < len) {  // the last < 32 elements belong to the second chain (xa <= the last group's start)
        if (k < xa)
            acc = fold_tail<TAcc>(f + k, len - k, acc);
        else
            acc2 = fold_tail<TAcc>(f + k, len - k, acc2);
    }
}

// fold_seq over row[a, b) of a 16-B aligned LDS row (a, b wave-uniform): up to 3 leading elements
// until row + a is aligned, then fold_seq.
template <typename TAcc>
__device__ __forceinline__ TAcc fold_span(const float* row, int a, int b, TAcc acc) {
    const int a4 = min(b, (a + 3) & ~3);
    if (a < a4) acc = fold_tail<TAcc>(row + a, a4 - a, acc);
    return a4 < b ? fold_seq<TAcc>(row + a4, b - a4, acc) : acc;
}

// The double chains (PCL's MSE sum and getFitnessScore) over values the fillers stored as doubles:
// the widening (exact) is done by the filler waves, so the fold lane only adds — a v_cvt_f64_f32 in
// front of every dependent v_add_f64 had put the chain at ~13.5 cycles per element.  Groups of 16
// doubles (8 x b128), three in rotation as in fold_seq.
__device__ __forceinline__ void load_group_d(double2 (&g)[8], const double* f) {
#pragma unroll
    for (int u = 0; u < 8; ++u) g[u] = *reinterpret_cast<const double2*>(f + 2 * u);
}
__device__ __forceinline__ void add_group_d(double& acc, const double2 (&g)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        acc = acc + g[u].x;
        acc = acc + g[u].y;
    }
}
__device__ __forceinline__ double fold_seq_d(const double* f, int len, double acc) {
    int k = 0;
    if (len >= 48) {
        double2 a[8], b[8], c[8];
        load_group_d(a, f);
        load_group_d(b, f + 16);
        for (; k + 48 <= len; k += 48) {
            // the loads past this round re-read group 0 harmlessly when nothing follows
            const int n1 = (k + 64 <= len) ? k + 48 : 0, n2 = (k + 80 <= len) ? k + 64 : 0;
            load_group_d(c, f + k + 32);
            __builtin_amdgcn_sched_barrier(0);
            add_group_d(acc, a);
            load_group_d(a, f + n1);
            __builtin_amdgcn_sched_barrier(0);
            add_group_d(acc, b);
            load_group_d(b, f + n2);
            __builtin_amdgcn_sched_barrier(0);
            add_group_d(acc, c);
        }
        // a, b hold [k, k + 16) and [k + 16, k + 32) when they exist
        if (k + 16 <= len) {
            add_group_d(acc, a);
            k += 16;
            if (k + 16 <= len) {
                add_group_d(acc, b);
                k += 16;
            }
        }
    }
    for (; k < len; ++k) acc = acc + f[k];
    return acc;
}

// ---------------------------------------------------------------------------------------------
// The cached-neighbour test of one pair by one workgroup of WG threads (the update's fused tail, and
// the fitness pass inside fitness_prep_kernel): the same work as nn_cache_test_kernel for the pair —
// X_i's new position (FROM_SRC: T·input_i, the fitness pass' final·input; else T·X_i, the deferred
// transformCloud(T_inc)), the bounds moved by |new − old|, the test against the cached NN; a miss
// sets its bit in the pair's bitmap (built in LDS: `need`, zeroed by the caller) and appends its
// search record; the fitness pass also writes a hit's key (finish_kernel's fitness reads them).
// kPer points per thread per group, software-pipelined: the next group's loads are issued before
// this group's stores, so the stores drain while the loads are in flight (a load issued after a store
// would wait behind it on vmcnt).
// Per point: X (.w = L) and nn_t (.w = target position | sorted position) read, U read (and the
// input point, FROM_SRC); X and U written (the fitness pass: neither bounds nor X, unless the aligned
// cloud is asked for).  The iteration passes write no key: nothing reads one before the fitness pass
// — the update folds recompute d² from X and nn_t, and the next search seeds from the record.
// The miss records stay in LDS (lv / lm, the first lcap of them) and are placed at their ranks in the
// pair's query list (qv / qm) at the end; a pair with more misses than lcap leaves its whole list in
// sq / sm with its bitmap, flagged kMissUnranked, for the search to place.
// The first point group's loads (kPer points per thread: X, the NN record, U) — issued by the update
// before its solve, so their latency hides behind thread 0's SVD (they do not depend on T_inc).
template <int kPer>
struct TailFirst {
    float4 v[kPer], t[kPer];
    float U[kPer];
};

// A fold wave's issue priority: its sequential chain is one dependent add after
// another, and the SIMD's other waves (fillers, the fused test's workers) otherwise take the issue
// slots between them.
__device__ __forceinline__ void fold_prio(bool hi) {
    if (hi)
        __builtin_amdgcn_s_setprio(3);
    else
        __builtin_amdgcn_s_setprio(0);
}

// SUMS (the update's tail, eligible pairs): the next pass A's Σs folded here, in index order, over the X
// the test writes — wave 0 lanes 0..2 fold, waves 1.. test (groups of (WG - 64) * kPer points, first
// to last, each group's new coordinates staged in `stg`: two buffers of 3 rows of kSumRow floats); the sums go to
// sums_out[0..2] (the pair state) with *sums_ok = 1.
constexpr int kSumPer = 2;  // the Σs tail's points per worker and group (4: 185 vs 179.5 us per update)
constexpr int kSumRow = 192 * kSumPer + 4;  // staged points per group (192 workers x kSumPer) + pad
constexpr int kSumBuf = 3 * kSumRow;        // one group's staging; two alternate (double buffer)
// The end of a pair's cached-neighbour test (pair_cache_test; res_update_pair's tail): the per-wave
// counts and work counters, then the miss records — lv / lm in LDS (the first lcap; beyond, sq / sm)
// — placed at their ranks in the pair's query list, or the whole list left unranked in sq / sm with
// the bitmap when it overflowed.  Returns the pair's misses.
template <int WG>
__device__ __forceinline__ int test_place(const WorkArgs& w, int p, int n, int hits, int misses, uint32_t* need,
                                          int32_t* pre, float4* lv, uint2* lm, int lcap, int32_t* wcnt, bool fitness,
                                          uint64_t* stamp) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t xs = (int64_t)p * w.x_stride;
    hits = wave_sumi(hits);
    misses = wave_sumi(misses);
    if (lane == 0) {
        wcnt[wave] = misses;
        count_add(w.evals, 0, (unsigned long long)hits);
        count_add(w.evals, 2, (unsigned long long)hits);
        count_add(w.evals, 3, (unsigned long long)(hits + misses));
        if (!fitness) {  // ... of which in an update's tail
            count_add(w.evals, 5, (unsigned long long)(hits + misses));
            count_add(w.evals, 6, (unsigned long long)hits);
        }
    }
    __syncthreads();
    if (stamp && tid == 0) *stamp = __builtin_amdgcn_s_memrealtime();  // diagnostic: the test's end
    int tot = 0;
    for (int k = 0; k < WG / 64; ++k) tot += wcnt[k];
    if (tot == 0) {
        if (tid == 0) w.miss_cnt[p] = 0;
        return 0;
    }
    const int nwords = (n + 31) >> 5;
    if (tot > lcap) {
        // more misses than LDS records (the few slowly converging pairs): the whole list goes to
        // sq / sm and the bitmap to global memory, and the search places it — a read-back of the
        // overflow here sat on this workgroup's end, which sets the update's launch time
        for (int k = tid; k < lcap; k += WG) {
            w.sq[xs + k] = lv[k];
            w.sm[xs + k] = lm[k];
        }
        uint32_t* gneed = w.need + (int64_t)p * w.need_stride;
        for (int k = tid; k < nwords; k += WG) gneed[k] = need[k];
        if (tid == 0) w.miss_cnt[p] = tot | kMissUnranked;
        return tot;
    }
    // Rank placement: the search reads its item's queries in sorted-position order (a run of 64
    // consecutive ones is a compact box), so every miss record goes to its rank in the bitmap — the
    // word's prefix + the set bits below it.  Done here, where the workgroup owns the whole bitmap,
    // instead of in the search, where it put two barriers and three dependent global round trips in
    // front of every work item.  Word prefixes: wave 0, kNeedWords / 64 words per lane.
    if (wave == 0) {
        constexpr int kW = kNeedWords / 64;
        int c[kW], sum = 0;
#pragma unroll
        for (int j = 0; j < kW; ++j) {
            const int wd = lane * kW + j;
            c[j] = wd < nwords ? __builtin_popcount(need[wd]) : 0;
            sum += c[j];
        }
        int incl = sum;
        incl = (int)wave_scan_incl((uint32_t)incl);  // (DPP)
        int run = incl - sum;
#pragma unroll
        for (int j = 0; j < kW; ++j) {
            pre[lane * kW + j] = run;
            run += c[j];
        }
    }
    if (tid == 0) w.miss_cnt[p] = tot;
    __syncthreads();
    float4* qv = w.qv + xs;
    uint2* qm = w.qm + xs;
    auto get = [&](int k, float4& r, uint2& m) {  // (tot <= lcap: every record is in LDS)
        k = min(k, tot - 1);
        r = lv[k];
        m = lm[k];
    };
    // (unconditional: a slot past the list re-read record tot - 1 and writes its very bytes to its
    // very rank again)
    auto put = [&](const float4 r, const uint2& m) {
        const uint32_t sp = min(m.y, (uint32_t)(n - 1));
        const int rk = pre[sp >> 5] + __builtin_popcount(need[sp >> 5] & ((1u << (sp & 31)) - 1u));
        qv[rk] = r;
        const uint2 mm = make_uint2((m.x & kNtIdxMask) | (sp << kNtPosShift), m.x >> kNtPosShift);
        uint64_t* const qmk = reinterpret_cast<uint64_t*>(&qm[rk]);
        *qmk = (uint64_t)mm.x | ((uint64_t)mm.y << 32);
    };
    for (int k0 = tid; k0 < tot; k0 += 4 * WG) {
        float4 r0, r1, r2, r3;  // (named, not an array: an array went to scratch)
        uint2 m0, m1, m2, m3;
        get(k0, r0, m0);  // all loads of the round first
        get(k0 + WG, r1, m1);
        get(k0 + 2 * WG, r2, m2);
        get(k0 + 3 * WG, r3, m3);
        put(r0, m0);
        put(r1, m1);
        put(r2, m2);
        put(r3, m3);
    }
    return tot;
}

template <int WG, int kPer, bool FROM_SRC, bool SUMS = false>
__device__ __forceinline__ int pair_cache_test(const PairArgs& a, const WorkArgs& w, int p, int n, const float (&T)[16],
                                                uint32_t* need, int32_t* pre, float4* lv, uint2* lm, int lcap,
                                                int32_t* mcount, int32_t* wcnt, bool fitness, uint64_t* stamp = nullptr,
                                                const TailFirst<kPer>* first = nullptr, float* stg = nullptr,
                                                float* sums_out = nullptr, int32_t* sums_ok = nullptr,
                                                const float* Tp = nullptr, bool silent = false) {
    // Lazy source cloud (WorkArgs::lazy_x; both workgroup-uniform, the update's tail only):
    //  silent: X', L', U' are formed and tested as ever but not stored — the caller records T as the
    //          pair's T_pend; the stored triple of every point stays consistent at the older state.
    //  Tp:     the pair is pending (the previous tail was silent, Tp = its T): an unflagged point is first
    //          brought to the state that tail would have stored — Tp * X, the bounds moved by that step, the
    //          very expressions it evaluated — a flagged one (re-written by the search since) is there
    //          already; then this tail's own step, stored with a positive L.
    static_assert(!SUMS || (WG - 64) * kPer <= kSumRow - 4, "staging rows");
    static_assert(!(FROM_SRC && SUMS), "the fitness pass folds no sums");
    float Tq[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) Tq[q] = (!FROM_SRC && !SUMS && Tp) ? uload(Tp + q) : 0.0f;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int WW = SUMS ? WG - 64 : WG;  // threads that test
    const bool worker = !SUMS || wave >= 1;
    const int wt = SUMS ? tid - 64 : tid;
    const int64_t xs = (int64_t)p * w.x_stride;
    float4* X = w.X + xs;
    float* uu = w.nn_u + xs;
    const float4* nt = w.nn_t + xs;
    const float4* src = FROM_SRC ? a.src + a.src_off[p] : nullptr;
    NNKey* key = w.nn_key + xs;
    constexpr int kStep = WW * kPer;
    int hits = 0, misses = 0;
    float fs = -0.0f;  // SUMS: wave 0 lane k's Σs chain (Eigen's rowwise().sum(): from the first element)
    float4 v[kPer], t[kPer], sv[kPer];
    float U[kPer];
    auto load = [&](int i0, float4 (&vv)[kPer], float4 (&tt)[kPer], float (&UU)[kPer], float4 (&ss)[kPer]) {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int i = min(i0 + e * WW + wt, n - 1);
            vv[e] = X[i];
            tt[e] = nt[i];
            UU[e] = uu[i];
            if (FROM_SRC) ss[e] = src[i];
        }
    };
    // Groups are visited last to first: the update's pass B has just streamed the
    // pair's X and nn_t front to back, so its most recently fetched lines — the ones still in the
    // L2 / MALL — are the pair's last ones.  (The folds must run in index order; the test may run in
    // any.)
    const int ngrp = (n + kStep - 1) / kStep;
    auto grp0 = [&](int g) { return (!SUMS ? ngrp - 1 - g : g) * kStep; };
    if (ngrp > 0 && worker) {
        if (first && !FROM_SRC) {
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                v[e] = first->v[e];
                t[e] = first->t[e];
                U[e] = first->U[e];
            }
        } else {
            load(grp0(0), v, t, U, sv);
        }
    }
    for (int g = 0; g < ngrp; ++g) {
        const int i0 = grp0(g);
        // SUMS: group g is staged in buffer g & 1 while the fold wave folds group g - 1 from the other;
        // the fold wave reaches barrier g only after folding g - 2, whose buffer group g reuses
        float* sg = stg + (g & 1) * kSumBuf;
        if (SUMS && !worker) {  // the fold wave: the group's staged coordinates, in index order
            __syncthreads();    // group g staged
            fold_prio(true);
            if (lane < 3) fs = fold_row(sg + lane * kSumRow, min(kStep, n - i0), fs);
            fold_prio(false);
            continue;
        }
        float4 vn[kPer], tn[kPer], sn[kPer];
        float Un[kPer];
        if (g + 1 < ngrp) load(grp0(g + 1), vn, tn, Un, sn);
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int i = i0 + e * WW + wt;
            const bool valid = i < n;
            float4 o = v[e];
            float4 b = v[e];  // the point and its bounds before this step (.w = L)
            b.w = fabsf(v[e].w);
            float Ub = U[e];
            if (!FROM_SRC && !SUMS && Tp) {
                float qx, qy, qz;
                xform_pt(Tq, b.x, b.y, b.z, qx, qy, qz);
                const float2 Lq = move_lu(make_float2(b.w, Ub), b.x, b.y, b.z, qx, qy, qz);
                const bool newer = l_flagged(v[e].w);
                b.x = newer ? b.x : qx;
                b.y = newer ? b.y : qy;
                b.z = newer ? b.z : qz;
                b.w = newer ? b.w : Lq.x;
                Ub = newer ? Ub : Lq.y;
            }
            if (FROM_SRC)
                xform_pt(T, sv[e].x, sv[e].y, sv[e].z, o.x, o.y, o.z);  // final * input
            else
                xform_pt(T, b.x, b.y, b.z, o.x, o.y, o.z);  // PCL transformCloud, in place
            const float2 Lm = move_lu(make_float2(b.w, Ub), b.x, b.y, b.z, o.x, o.y, o.z);
            o.w = Lm.x;
            const float d2 = l2_simple(o.x, o.y, o.z, t[e].x, t[e].y, t[e].z);
            const bool hit = valid & cache_hit(Lm.x, d2);
            // (the fitness pass: no later pass reads the bounds, and X only for the aligned output —
            // the misses' search records carry their own coordinates)
            if (valid && (!fitness || a.aligned) && !silent) X[i] = o;
            if (valid && !fitness && !silent) uu[i] = Lm.y;
            if (SUMS && valid) {
                sg[e * WW + wt] = o.x;
                sg[kSumRow + e * WW + wt] = o.y;
                sg[2 * kSumRow + e * WW + wt] = o.z;
            }
            const int k = wave_append(valid && !hit, mcount);
            if (hit) {
                // the fitness pass' keys are read for their d² only (finish_kernel): a hit's index
                // bits carry its NN's sorted position, no gather of the original index
                if (fitness) key[i] = make_key(d2, nt_tpos(t[e].w));
                ++hits;
            } else if (valid) {
                const uint32_t sp = nt_pos(t[e].w);
                atomicOr(&need[sp >> 5], 1u << (sp & 31));
                if (k < lcap) {
                    lv[k] = make_float4(o.x, o.y, o.z, Lm.y);
                    *reinterpret_cast<uint64_t*>(&lm[k]) =
                        (uint64_t)((uint32_t)i | (nt_tpos(t[e].w) << kNtPosShift)) | ((uint64_t)sp << 32);
                } else {
                    put_miss(w, p, k, sp, i, o.x, o.y, o.z, Lm.y, nt_tpos(t[e].w));
                }
                ++misses;
            }
        }
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            v[e] = vn[e];
            t[e] = tn[e];
            U[e] = Un[e];
            if (FROM_SRC) sv[e] = sn[e];
        }
        if (SUMS) __syncthreads();  // group g staged
    }
    if (SUMS && wave == 0 && lane < 3) {
        sums_out[lane] = fs;
        if (lane == 0 && *sums_ok != -1) *sums_ok = 1;
    }
    return test_place<WG>(w, p, n, hits, misses, need, pre, lv, lm, lcap, wcnt, fitness, stamp);
}

constexpr int kFoldChunkP = 512;  // points per LDS chunk of the fold passes

// Each fold chain's row is padded by kFoldPad floats: unpadded, rows 2 KB apart start on the same
// LDS bank, and the 7-9 fold lanes' ds_read_b128 of one column were a 7-9-way bank conflict on every
// read.  Padded by 16 B they take distinct banks.
constexpr int kFoldPad = 4;

}  // namespace icp4r
