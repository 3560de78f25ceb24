// icp4r_tile.hpp — the LDS-tile search machinery that nn_lds_kernel, nn_tile_kernel and solo_kernel
// (icp4r_kernels.hip) share: the tile's constants and slot / key packing, the box bounds, the staging of a
// pair's sorted targets and boxes, the superblock reach masks and the exact search of a query list (lds_runs).
// Device-inline helpers, structs and constants only: no kernel, no launch.
#pragma once

#include "icp4r_nn.hpp"

namespace icp4r {

// ---------------------------------------------------------------------------------------------
// The batched exact 1-NN (many pairs, targets <= kLdsTargets): three launches per NN pass.
//
//  nn_cache_test_kernel  (passes after the first, CACHE only) the cached-neighbour test of every
//                        query, elementwise at full occupancy: hits get their key / correspondence
//                        record; misses are flagged by Morton position in the pair's bitmap (w.need)
//                        and counted per pair (w.miss_cnt).
//  nn_order_kernel       one workgroup: the pairs that need a search, heaviest first (pair work list
//                        w.plist, w.plist_n), and the search's work-queue counter reset.
//  nn_lds_kernel<CACHE>  persistent (one workgroup per CU): takes pairs from the work list; per
//                        pair it stages the Morton-sorted target set in LDS and searches the queries
//                        that need it (all of them in the first pass / without CACHE).
//
// Search (per pair, one 1024-thread workgroup, the target set in LDS — 128 KB; block / superblock
// boxes stream through the scalar cache).  Each wave owns a Morton-contiguous run of queries and,
// instead of sweeping every block that ANY of its queries might need (nn_pruned_kernel), tests
// blocks per query and appends the (query, block) pairs that pass to a per-wave ring of work items;
// every 64 items are evaluated one per lane (16 targets from LDS each) and merged with an LDS
// atomicMin on the (d², index) key.  The answer is the same exact minimum (PCL semantics, lowest
// index among ties).
//
// CACHE (cached-neighbour test, exact): a search also returns L_i, a lower bound on the distance
// from X_i to every target other than its nearest one j (the exact second-nearest distance: the
// search prunes against the second-best key instead of the best, and an LDS atomicMin keeps the
// smallest key that lost a comparison).  Every kernel that moves X_i by δ_i lowers L_i by δ_i
// (triangle inequality, move_lb).  The next pass first evaluates d_j only: if
// L_i² (1 − m) > d_j² (1 + m) every other target is strictly farther in float too, so (d_j², j)
// IS the brute-force answer — no tie is possible — and the query needs no search.  ICP's increments
// shrink geometrically, so after the first few iterations most queries pass.  The margin m = 1e-4
// is ~500x the float rounding of the test (l2_simple: <= 5 ulp; the bounds are rounded down).
//
// Why persistent + a work list: a late pass leaves most pairs with no miss at all and a few (slowly
// converging) pairs with thousands; one workgroup per pair paid a dispatch gap per pair and let
// the heavy pairs that happened to share a CU set the launch time.
constexpr int kLdsTargets = 8192;
constexpr int kLdsLeaf = 16;
constexpr int kLdsWG = 1024;
constexpr int kLdsWaves = kLdsWG / 64;
constexpr int kLdsQ = 1;  // queries per lane (2 measured no faster: smaller runs prune better)
constexpr int kRing = 128;  // work items per wave (<= 63 pending + 64 appended per query slot)
static_assert(kNeedWords <= kLdsWG, "compaction: one bitmap word per thread");

// An LDS address held in a VGPR: a wave-uniform LDS address otherwise sits in an SGPR and every
// ds_read of a row pays its own v_mov; from a VGPR base the row's reads take immediate offsets.
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(3))) T* lds_vbase(const T* p) {
    const auto* l = (const __attribute__((address_space(3))) T*)p;
    uint32_t a = (uint32_t)(uintptr_t)l, v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(a));
    return (const __attribute__((address_space(3))) T*)(uintptr_t)v;
}

// Per lane: bit `lane` of the wave mask m set ? if1 : if0 (one v_cndmask on the mask itself)
__device__ __forceinline__ uint32_t lane_select(uint64_t m, uint32_t if0, uint32_t if1) {
    uint32_t r;
    asm volatile("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if0), "v"(if1), "s"(m));
    return r;
}

// The 16 targets of LDS block b (lds_swz order) into cs: slot t sits at byte A ^ (t << 4) with
// A = the block's base | (b & 15) << 4 — one v_xor per read instead of an xor, shift and or.
__device__ __forceinline__ void lds_block(const v4f* tl, int b, v4f (&cs)[16]) {
    const uint32_t base = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) v4f*)tl;
    const uint32_t A = (base + ((uint32_t)b << 8)) | (((uint32_t)b & 15u) << 4);
#pragma unroll
    for (int t = 0; t < 16; ++t) cs[t] = *(const __attribute__((address_space(3))) v4f*)(uintptr_t)(A ^ ((uint32_t)t << 4));
}

// An LDS target slot is {key, x, y, z}: the key (original index << 13 | LDS position) first, so a
// drain's (d², key) pair forms in the aligned register pair of the slot's first two words (d²
// overwrites x, dead once dx is formed) — with the key last, every evaluation paid a v_mov to pair
// them (a 64-bit VGPR operand must start on an even register).
__device__ __forceinline__ v4f tl_slot(const v4f t, uint32_t k) { return (v4f){__uint_as_float(k), t.x, t.y, t.z}; }
__device__ __forceinline__ float tl_x(const v4f c) { return c.y; }
__device__ __forceinline__ float tl_y(const v4f c) { return c.z; }
__device__ __forceinline__ float tl_z(const v4f c) { return c.w; }
__device__ __forceinline__ uint32_t tl_key(const v4f c) { return __float_as_uint(c.x); }

// The second-smallest d² of a block after one more evaluation: s2 ≥ b (the current best's d²)
// holds throughout, so min(s2, max(b, d)) — "d below the best: the old best; else min(s2, d)" —
// is the median of the three (one v_med3_u32; d² bits order as unsigned: never negative).
__device__ __forceinline__ uint32_t second_d2(uint32_t b, uint32_t d, uint32_t s2) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(d), "v"(s2));
    return r;
}

// The batched search's box tests against a bound pre-multiplied by kLbGrow (> 1 / kLbShrink with
// margin): lb <= bnd·kLbGrow rejects only what lb·kLbShrink <= bnd rejects, one multiply fewer per
// test.  The per-axis gap v - clamp(v, lo, hi) (a med3) has the magnitude of max(lo - v, v - hi, 0)
// bit for bit (IEEE subtraction is sign-symmetric); a box staged as FLT_MAX (empty) gives +inf.
constexpr float kLbGrow = 1.00002f;
template <typename P>
__device__ __forceinline__ float pt_lb(const P b, float x, float y, float z) {
    const float gx = x - __builtin_amdgcn_fmed3f(x, b[0], b[3]);
    const float gy = y - __builtin_amdgcn_fmed3f(y, b[1], b[4]);
    const float gz = z - __builtin_amdgcn_fmed3f(z, b[2], b[5]);
    return __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx));
}
// lower bound of the distance between boxes [lo, hi] and [qlo, qhi] (squared; empty: +inf)
__device__ __forceinline__ float box_lb(const v4f lo, const v4f hi, const float (&qlo)[3], const float (&qhi)[3]) {
    const float gx = fmaxf(fmaxf(lo.x - qhi[0], qlo[0] - hi.x), 0.0f);
    const float gy = fmaxf(fmaxf(lo.y - qhi[1], qlo[1] - hi.y), 0.0f);
    const float gz = fmaxf(fmaxf(lo.z - qhi[2], qlo[2] - hi.z), 0.0f);
    return __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx));
}

constexpr int kSbBatch = 1;  // candidate superblocks tested together per traversal step

static_assert(kSbBatch >= 1 && kSbBatch <= 5, "six bits per superblock in a 32-bit pack");

// LDS slot of sorted target position p: the slot inside its 16-target block XOR the block's low
// bits — an involution per block (bank spreading for the drain, see nn_lds_kernel)
__device__ __forceinline__ int lds_swz(int p) { return p ^ ((p >> 4) & (kLdsLeaf - 1)); }

// (nn_t[i].w and the query records: nt_tpos / nt_pos, icp4r_nn.hpp)
static_assert(kCacheMaxN <= (1 << kNtPosShift) && kLdsTargets <= (1 << kNtPosShift) && kLdsMaxSources == (1 << kNtPosShift),
              "nn_t.w / query record packing");
__device__ __forceinline__ float nt_pack(int tpos, int pos) {
    return __uint_as_float((uint32_t)tpos | ((uint32_t)pos << kNtPosShift));
}

// LDS target record .w during the batched search: original index << 13 | sorted position.  Keys
// compare (d², original index) exactly as before (the index is unique and the position follows
// it), and the winner's slot in LDS comes back with its key.
constexpr int kLdsPosBits = 13;
static_assert(kLdsTargets <= (1 << kLdsPosBits), "LDS key packing");
__device__ __forceinline__ uint32_t lk_idx(NNKey k) { return (uint32_t)k >> kLdsPosBits; }
__device__ __forceinline__ uint32_t lk_pos(NNKey k) { return (uint32_t)k & ((1u << kLdsPosBits) - 1); }

__device__ __forceinline__ void write_corr_t(const WorkArgs& w, const PairArgs& a, int p, int i, float sx, float sy,
                                             float sz, float d2, const float4 t) {
    float4* C = w.corr + ((int64_t)p * w.x_stride + i) * 2;
    const float wt = a.kp.huber_delta < INFINITY ? (float)huber_w(d2, a.kp.huber_delta) : 1.0f;
    C[0] = make_float4(sx, sy, sz, wt);
    C[1] = make_float4(t.x, t.y, t.z, d2);
}

// With the cached-neighbour state a pass's keys are read only by the finish kernel's fitness (the
// fitness pass) and by the F64 update (load_nn); the PCL-numerics update folds X and nn_t.
__device__ __forceinline__ bool keys_read(const PairArgs& a, int fitness_pass) {
    return fitness_pass || a.kp.numerics != kNumericsPCL;
}

// Counters of the LDS search runs (device work counts; per-wave events and clocks for
// plan option phase_ticks = 1 — tools/experiments/nn_events.py)
struct RunStats {
    unsigned long long evals = 0, tests = 0;
    uint32_t ev_runs = 0, ev_q = 0, ev_sbv = 0, ev_sbp = 0, ev_blk = 0, ev_push = 0, ev_drain = 0, ev_items = 0;
    uint64_t ck_setup = 0, ck_trav = 0, ck_write = 0;
};
// The LDS arrays a search reads: one pair's staged targets (.w = original index << 13 | position)
// and block / superblock boxes (empty: FLT_MAX).
struct LdsTile {
    v4f* tl;
    float (*bx)[6];
    float (*sbx)[6];
};

// Stage pair p's sorted targets and boxes for an LDS search (every superblock of the pair: nsb <= 64)
// and load lane l's superblock box into isl / ish (kept in registers for every run).  Every load is
// issued before the first store: a load-store loop waited out one global round trip per target (8
// per thread, ~10-20 us per item under load).  The caller's barrier makes the LDS visible.
// A pair's tile in registers (every load issued, nothing waited for): tile_load, then tile_store.
template <int WG>
struct TileRegs {
    v4f tv[kLdsTargets / WG];
    v4f blo, bhi, isl, ish;
};
template <int WG>
__device__ __forceinline__ void tile_load(const WorkArgs& w, int p, int nsb, TileRegs<WG>& r, uint64_t M = ~0ull) {
    const int tid = threadIdx.x, lane = tid & 63;
    const v4f* tsg = reinterpret_cast<const v4f*>(w.tsort + (int64_t)p * w.t_stride);
    const int nt = nsb * kSuper * kLdsLeaf;
    constexpr int kPerT = kLdsTargets / WG;
    static_assert(kLdsTargets % WG == 0, "targets per thread");
    // M: the superblocks to stage; the others load target 0 (one line for the whole wave) into slots
    // no search reads.  A wave's 64 positions lie in one superblock: the test is scalar.
    static_assert(kLdsLeaf * kSuper % 64 == 0 && WG % (kLdsLeaf * kSuper) == 0, "wave-uniform superblock");
    const int wsb = __builtin_amdgcn_readfirstlane(tid / (kLdsLeaf * kSuper));
#pragma unroll
    for (int k = 0; k < kPerT; ++k) {
        const bool on = M == ~0ull || ((M >> (wsb + k * (WG / (kLdsLeaf * kSuper)))) & 1ull);
        r.tv[k] = tsg[on ? min(tid + k * WG, nt - 1) : 0];
    }
    const v4f* tb = reinterpret_cast<const v4f*>(w.tbox + (int64_t)p * 2 * w.b_stride);
    const v4f* sbg = reinterpret_cast<const v4f*>(w.sbox + (int64_t)p * 2 * w.sb_stride);
    static_assert(kLdsTargets / kLdsLeaf / kSuper * (kSuper + 1) <= WG, "one box per thread");
    const int nbx = nsb * (kSuper + 1);
    const int bq = min(tid, nbx - 1);
    const bool blk = bq < nsb * kSuper;
    const int kb = blk ? bq : bq - nsb * kSuper;
    r.blo = blk ? tb[2 * kb] : sbg[2 * kb];
    r.bhi = blk ? tb[2 * kb + 1] : sbg[2 * kb + 1];
    const int sbl = min(lane, nsb - 1);  // (in flight across the caller's barrier)
    r.isl = sbg[2 * sbl];
    r.ish = sbg[2 * sbl + 1];
}
template <int WG>
__device__ __forceinline__ void tile_store(const LdsTile& sh, int nsb, const TileRegs<WG>& r) {
    const int tid = threadIdx.x;
    const int nt = nsb * kSuper * kLdsLeaf;
    constexpr int kPerT = kLdsTargets / WG;
#pragma unroll
    for (int k = 0; k < kPerT; ++k) {
        int i = tid + k * WG;
        // (opaque: the slot addresses are formed here, not hoisted out of a caller's item loop as
        // invariants — kept live across the search they pushed its other values into scratch)
        asm volatile("" : "+v"(i));
        if (i < nt) sh.tl[lds_swz(i)] = tl_slot(r.tv[k], (__float_as_uint(r.tv[k].w) << kLdsPosBits) | (uint32_t)i);
    }
    const int nbx = nsb * (kSuper + 1);
    if (tid < nbx) {
        const bool blk = tid < nsb * kSuper;
        const int kb = blk ? tid : tid - nsb * kSuper;
        const bool empty = !(r.blo.x <= r.bhi.x);  // (+inf, -inf): a box no point reaches
        float* d = blk ? sh.bx[kb] : sh.sbx[kb];
        d[0] = empty ? FLT_MAX : r.blo.x; d[1] = empty ? FLT_MAX : r.blo.y; d[2] = empty ? FLT_MAX : r.blo.z;
        d[3] = empty ? FLT_MAX : r.bhi.x; d[4] = empty ? FLT_MAX : r.bhi.y; d[5] = empty ? FLT_MAX : r.bhi.z;
    }
}

// Stage pair p's sorted targets and boxes for an LDS search (every superblock of the pair: nsb <= 64)
// and load lane l's superblock box into isl / ish (kept in registers for every run).  Every load is
// issued before the first store: a load-store loop waited out one global round trip per target (8
// per thread, ~10-20 us per item under load).  The caller's barrier makes the LDS visible.
template <int WG>
__device__ __forceinline__ void stage_tile(const LdsTile& sh, const WorkArgs& w, int p, int nsb, v4f& isl, v4f& ish,
                                           uint64_t M = ~0ull) {
    TileRegs<WG> r;
    tile_load<WG>(w, p, nsb, r, M);
    tile_store<WG>(sh, nsb, r);
    isl = r.isl;
    ish = r.ish;
}

// The superblocks an item's queries can reach (plan option stage_sel): a lane-per-superblock test of
// each query against lds_runs' initial pruning bound.  lds_runs reads a target only (a) in a query's
// seed block, or (b) in a block it queued, whose superblock passed pt_lb(superblock, q) <= bnd_q for
// that query; and bnd_q = min(seed block's second-smallest d², U²·1.00001) · kLbGrow never exceeds
// B_q = (U²·1.00001) · kLbGrow (the same float expressions: rounding is monotone), nor grows.  So
// every target the search reads lies in a superblock with pt_lb <= B_q for some query of the item,
// or in a seed's superblock — the mask below holds both (idle lanes shadow a run's first query, so
// they read its seed).  A U that is not finite stages everything.  Wave w tests queries w, w + NW, …
// (uniform loads); the caller ORs the waves' masks.  Items of more than kSelExact queries: per run of 64.
constexpr int kSelExact = 64;
template <int WG>
__device__ __forceinline__ uint64_t reach_mask(const float4* qv, const uint2* qm, int nlist, int m, int nsb,
                                               const v4f isl, const v4f ish) {
    constexpr int NW = WG / 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const float b[6] = {isl.x, isl.y, isl.z, ish.x, ish.y, ish.z};  // (an empty box passes: a superset)
    const bool mine = lane < nsb;
    uint64_t mk = 0;
    if (nlist > kSelExact) {
        // larger items: 64 consecutive queries (a compact run of sorted positions) at a time, tested as
        // their bounding box against their largest bound — box_lb(sb, box) <= pt_lb(sb, q) <= B_q <= max B
        // for every query q in the box (the same per-axis gaps, monotone float arithmetic): a superset
        const v4f lo4 = isl, hi4 = ish;
        for (int j0 = wave * 64; j0 < nlist; j0 += NW * 64) {
            const int j = min(j0 + lane, nlist - 1);
            const float4 q = qv[j];
            const uint32_t sd = qm[j].y;
            const float B = __uint_as_float(__float_as_uint(q.w * q.w * 1.00001f)) * kLbGrow;
            if (__ballot(!(B < INFINITY)) != 0ull) return ~0ull;
            float qlo[3] = {q.x, q.y, q.z}, qhi[3] = {q.x, q.y, q.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                qlo[k] = wave_minf(qlo[k]);
                qhi[k] = wave_maxf(qhi[k]);
            }
            const float bmax = wave_maxf(B);
            mk |= __ballot(mine && box_lb(lo4, hi4, qlo, qhi) <= bmax);
            unsigned long long s = 1ull << (min(sd, (uint32_t)(m - 1)) / (uint32_t)(kLdsLeaf * kSuper));
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s |= __shfl_xor(s, off, 64);
            mk |= s;
        }
        return mk;
    }
    for (int j0 = wave; j0 < nlist; j0 += 4 * NW) {
        float4 q[4];
        uint32_t sd[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = min(j0 + e * NW, nlist - 1);
            q[e] = qv[j];
            sd[e] = qm[j].y;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float B = __uint_as_float(__float_as_uint(q[e].w * q[e].w * 1.00001f)) * kLbGrow;
            mk |= (B < INFINITY) ? __ballot(mine && pt_lb(b, q[e].x, q[e].y, q[e].z) <= B) : ~0ull;
            mk |= 1ull << (min(sd[e], (uint32_t)(m - 1)) / (uint32_t)(kLdsLeaf * kSuper));
        }
    }
    return mk;
}

// The superblock mask of a small item (stage_sel): reach_mask over the workgroup's waves, ORed through
// selm (kLdsWaves words of LDS); ends with a barrier.  stage_tile then loads the targets of the named
// superblocks only (a late pass's item of a few misses stages a few KB instead of the whole 128-KB
// tile, for one more round trip: the queries and superblock boxes before the targets).
template <int WG>
__device__ __forceinline__ uint64_t reach_all(unsigned long long* selm, const WorkArgs& w, int p, int nsb, int m,
                                              const float4* qv, const uint2* qm, int nlist) {
    const int tid = threadIdx.x, lane = tid & 63;
    const v4f* sbg = reinterpret_cast<const v4f*>(w.sbox + (int64_t)p * 2 * w.sb_stride);
    const int sbl = min(lane, nsb - 1);
    const uint64_t mk = reach_mask<WG>(qv, qm, nlist, m, nsb, sbg[2 * sbl], sbg[2 * sbl + 1]);
    if (lane == 0) selm[tid >> 6] = mk;
    __syncthreads();
    uint64_t M = 0;
#pragma unroll
    for (int v = 0; v < WG / 64; ++v) M |= selm[v];
    // (uniform: scalar registers, not two VGPRs live across the staging)
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(M >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)M);
}

// The exact LDS search of one query list [0, nlist) of pair p (qv / qm: {x, y, z, U}, {source index |
// sorted position << 14, seed target position}, in sorted-position order) against the staged tile,
// by the workgroup's kLdsWaves waves (this wave: its runs, with bestl / secl / ring its LDS state).
// CACHE: the second-nearest distance too (X.w = L, nn_u = U, nn_t = the NN's coordinates | positions);
// want_key: the (d², index) key; corr: the correspondence record (plans without the cached state).
template <bool CACHE>
__device__ __forceinline__ void lds_runs(const LdsTile& sh, unsigned long long* bestl, uint32_t* secl, uint16_t* ring,
                                         const float4* qv, const uint2* qm, int nlist, int m, int nsb, const v4f isl,
                                         const v4f ish, const PairArgs& a, const WorkArgs& w, int p, int64_t xs0,
                                         float4* X, NNKey* key, bool want_key, bool corr, RunStats& rs,
                                         uint32_t lflag = 0u) {  // (kLazyFlag in a pending pass: ORed into L)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // Queries per wave run: the list is cut into R rounds of kLdsWaves equal position-contiguous
    // runs of at most 64 (R = ceil(nlist / (kLdsWaves * 64))), so every wave gets the same share —
    // a short list (the misses of a late pass) spreads over all waves, and the traversal,
    // latency-bound per wave, runs on small runs whose tight query box prunes most superblocks.
    const int rounds = max(1, (nlist + kLdsWaves * 64 - 1) / (kLdsWaves * 64));
    const int per = (nlist + kLdsWaves * rounds - 1) / (kLdsWaves * rounds);
    const int stride = kLdsWaves * per;
    // the run's records (idle lanes shadow the run's first query: they never queue work and
    // never widen the run's box); the next run's are loaded while this one is searched
    auto fetch = [&](int b, float4& v, uint2& mq) {
        const int s = (b + lane < min(b + per, nlist)) ? b + lane : b;
        v = qv[s];
        mq = qm[s];
    };
    float4 nv = make_float4(0.f, 0.f, 0.f, 0.f);
    uint2 nm = make_uint2(0u, 0u);
    if (wave * per < nlist) fetch(wave * per, nv, nm);
    for (int base = wave * per; base < nlist; base += stride) {
        const int cend = min(base + per, nlist);
        const uint64_t ck0 = __builtin_readcyclecounter();
        ++rs.ev_runs;
        rs.ev_q += (uint32_t)(cend - base);
        const float x = nv.x, y = nv.y, z = nv.z, uu = nv.w;
        const bool live = base + lane < cend;
        const int orig = (int)(nm.x & kNtIdxMask);
        const int spos = (int)(nm.x >> kNtPosShift);
        const int pj = min((int)nm.y, m - 1);
        __builtin_amdgcn_sched_barrier(0);  // the current record consumed before the prefetch
        if (base + stride < nlist) fetch(base + stride, nv, nm);
        float bnd;  // pruning bound: best d² (plain search) / second-best d² (CACHE search);
                    // -1 on idle lanes (never queue work, never widen the coarse bound)
        const int seed_pos0 = __builtin_amdgcn_readfirstlane(pj);
        const int seed_blk = pj / kLdsLeaf;
        {
            // seed: the previous match (first pass: the target at the same relative position)
            // and the rest of its 16-target block, evaluated up front from LDS — tight initial
            // bounds, so the coarse rs.tests below already prune with them
            NNKey lo = ~0ull;       // the smallest key seen
            uint32_t s2 = ~0u;      // the smallest d² of every other target seen (bits)
            v4f cs[kLdsLeaf];
            lds_block(sh.tl, pj / kLdsLeaf, cs);
            __builtin_amdgcn_sched_barrier(0);  // all 16 reads in flight before the first use
#pragma unroll
            for (int t = 0; t < kLdsLeaf; ++t) {
                const v4f c = cs[t];
                const float d2 = l2_simple(x, y, z, tl_x(c), tl_y(c), tl_z(c));
                const NNKey kn = make_key(d2, tl_key(c));
                if (CACHE) s2 = second_d2((uint32_t)(lo >> 32), __float_as_uint(d2), s2);
                lo = kn < lo ? kn : lo;
            }
            bestl[lane] = lo;
            if (CACHE) {
                // U of the previous search, moved since: an upper bound of the second-nearest
                // distance even if no evaluated target attains it (all-query passes: +inf)
                const uint32_t sec0 = min(s2, __float_as_uint(uu * uu * 1.00001f));
                secl[lane] = sec0;
                bnd = live ? __uint_as_float(sec0) * kLbGrow : -1.0f;
            } else {
                bnd = live ? key_d2(lo) * kLbGrow : -1.0f;
            }
            rs.evals += 64 * kLdsLeaf;  // the wave's lanes (counted once by lane 0)
        }
        float qlo[3] = {x, y, z}, qhi[3] = {x, y, z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // DPP reductions (no LDS round trips), wave-uniform results
            qlo[k] = wave_minf(qlo[k]);
            qhi[k] = wave_maxf(qhi[k]);
        }
        const float qmax = wave_maxf(bnd);

        // Evaluate `cnt` (<= 64) queued items from ring[head..]: lane L takes item head + L.
        uint32_t head = 0, tail = 0;
        auto drain = [&](uint32_t cnt) {
            ++rs.ev_drain;
            rs.ev_items += cnt;
            const bool act = (uint32_t)lane < cnt;
            const uint32_t it = ring[(head + lane) & (kRing - 1)];
            const int owner = act ? (int)(it >> 9) : 0;
            const int b = act ? (int)(it & 0x1ffu) : 0;
            // the query's coordinates from its owner lane
            const float qx = __shfl(x, owner, 64), qy = __shfl(y, owner, 64), qz = __shfl(z, owner, 64);
            if (act) {
                NNKey k1 = ~0ull;
                uint32_t s2 = ~0u;  // second-smallest d² of the block (bits; >= k1's throughout)
                // block b's targets sit XOR-swizzled (lds_swz): at step t lane L reads slot
                // t ^ (b_L & 15), so lanes on different blocks spread over the 64 banks instead of
                // all hitting the 4 banks of slot t (a 64-way conflict: every block is 256 B)
                // all 16 reads issued before the first compare (the compiler otherwise keeps two
                // in flight: 8 dependent LDS round trips per drain)
                v4f cs[kLdsLeaf];
                lds_block(sh.tl, b, cs);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < kLdsLeaf; ++t) {
                    const v4f c = cs[t];
                    const float d2 = l2_simple(qx, qy, qz, tl_x(c), tl_y(c), tl_z(c));
                    const NNKey kn = make_key(d2, tl_key(c));
                    if (CACHE) s2 = second_d2((uint32_t)(k1 >> 32), __float_as_uint(d2), s2);
                    k1 = kn < k1 ? kn : k1;
                }
                if (CACHE) {
                    // every key but the final winner loses exactly one comparison: keep the smallest loser
                    const NNKey old = atomicMin(&bestl[owner], k1);
                    const uint32_t cand =
                        k1 < old ? min((uint32_t)(old >> 32), s2) : (k1 == old ? s2 : (uint32_t)(k1 >> 32));
                    atomicMin(&secl[owner], cand);
                } else {
                    atomicMin(&bestl[owner], k1);
                }
            }
            head += cnt;
            rs.evals += (unsigned long long)cnt * kLdsLeaf;
            // tighter bounds for the rs.tests
            bnd = !live ? -1.0f : (CACHE ? __uint_as_float(secl[lane]) : key_d2(bestl[lane])) * kLbGrow;
        };
        // coarse test of every superblock at once (lane = superblock; nsb <= 64 here): the boxes
        // sit in the lanes' registers for the whole item (isl / ish)
        const uint64_t cmask = __ballot(lane < nsb && box_lb(isl, ish, qlo, qhi) <= qmax);
        rs.tests += nsb;
        const int sb0 = seed_pos0 / (kLdsLeaf * kSuper);
        // the candidate superblocks outward from the seed's, alternating up / down (only set bits
        // of cmask are visited: a scalar loop over all nsb cost ~10 SALU per superblock per run)
        uint64_t um = sb0 < 64 ? (cmask >> sb0) << sb0 : 0ull, dm = cmask & ~um;
        bool upnext = true;
        auto next_sb = [&]() -> int {
            if (!(um | dm)) return -1;
            int sb;
            if (um && (upnext || !dm)) {
                sb = __builtin_ctzll(um);
                um &= um - 1;
            } else {
                sb = 63 - __builtin_clzll(dm);
                dm &= ~(1ull << sb);
            }
            upnext = !upnext;
            return sb;
        };
        // Candidates are taken kSbBatch at a time: their per-query superblock rs.tests run as
        // independent chains (the traversal is bound by dependent latency, not by issue); then
        // every superblock some lane may reach has its 8 blocks tested for every lane in one
        // straight-line sequence (boxes broadcast from LDS, 8 independent rs.tests in flight), and
        // the non-empty ones are queued.  A test may use a bound a drain has since tightened:
        // that only queues more work, never loses a target.
        const uint64_t ck1 = __builtin_readcyclecounter();
        // A superblock some lane may reach has its 8 blocks tested for those lanes only: the c
        // lanes that passed are compacted (ds_permute: rank k -> lane k), and each round rs.tests 8
        // of them against the 8 blocks at once — lane L takes passed lane r0 + L / 8 and block
        // L % 8, with that query's coordinates and bound pulled from its lane (ds_bpermute).  The
        // (query, block) pairs that pass are queued with one ballot per round.  (Testing all 64
        // lanes against all 8 blocks spent 80 VALU per superblock on the ~5 lanes that need it.)
        const int blk8 = lane & (kSuper - 1);
        for (;;) {
            // kSbBatch candidates tested together (independent LDS reads and test chains), then
            // the ones some lane may reach processed in order
            int sbs[kSbBatch];
            uint64_t ms[kSbBatch];
#pragma unroll
            for (int j = 0; j < kSbBatch; ++j) sbs[j] = next_sb();
            if (sbs[0] < 0) break;
#pragma unroll
            for (int j = 0; j < kSbBatch; ++j) {
                const auto* sbb = lds_vbase(&sh.sbx[sbs[j] < 0 ? 0 : sbs[j]][0]);
                ms[j] = sbs[j] < 0 ? 0ull : __ballot(pt_lb(sbb, x, y, z) <= bnd);
                rs.ev_sbv += sbs[j] < 0 ? 0 : 1;
            }
            rs.tests += 64 * kSbBatch;
#pragma unroll
            for (int j = 0; j < kSbBatch; ++j) {
            const int sb = sbs[j];
            const uint64_t m = ms[j];
            if (m == 0) continue;
            ++rs.ev_sbp;
            const int c = __builtin_popcountll(m);
            // this lane's tag: its lane id, and its seed block if that lies in sb (never queued:
            // it was evaluated whole up front)
            const int rel = seed_blk - sb * kSuper;
            const uint32_t tag = (uint32_t)lane | ((uint32_t)rel < (uint32_t)kSuper ? (8u | (uint32_t)rel) << 6 : 0u);
            const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            // passed lanes go to lane rank, the others to distinct lanes >= c (no collisions)
            const uint32_t dst = lane_select(m, (uint32_t)c + (uint32_t)lane - rk, rk);
            const uint32_t packed = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)tag);
            // this lane's block box (8 rows, each read by 8 lanes: broadcast)
            const auto* brow = lds_vbase(&sh.bx[sb * kSuper + blk8][0]);
            float bb[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) bb[k] = brow[k];
            rs.tests += 8 * c;
            for (int r0 = 0; r0 < c; r0 += 8) {
                const int srcl = r0 + (lane >> 3);
                const uint32_t tg = (uint32_t)__builtin_amdgcn_ds_bpermute(srcl << 2, (int)packed);
                const int owner = (int)(tg & 63u);
                const float qx = __shfl(x, owner, 64), qy = __shfl(y, owner, 64), qz = __shfl(z, owner, 64);
                const float qb = __shfl(bnd, owner, 64);
                const bool ok = srcl < c && (tg >> 6) != (8u | (uint32_t)blk8) && pt_lb(bb, qx, qy, qz) <= qb;
                const uint64_t pm = __ballot(ok);
                if (pm == 0) continue;
                rs.ev_blk += __builtin_popcountll(pm);
                const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)pm, tail));
                const uint32_t at = lane_select(pm, (uint32_t)(kRing + lane), slot & (kRing - 1));
                ring[at] = (uint16_t)(((uint32_t)owner << 9) | (uint32_t)(sb * kSuper + blk8));
                tail += (uint32_t)__builtin_popcountll(pm);
                if (tail - head >= 64) drain(64);
            }
            }
        }
        if (tail != head) drain(tail - head);
        const uint64_t ck2 = __builtin_readcyclecounter();
        // the winner's coordinates come from its LDS slot (the key carries its position)
        const NNKey kb = bestl[lane];
        const uint32_t tpos = lk_pos(kb);
        const v4f t = sh.tl[lds_swz((int)tpos)];
        if (live) {
            const NNKey ko = make_key(key_d2(kb), lk_idx(kb));  // (d², original index): PCL's answer
            if (want_key) key[orig] = ko;
            if (CACHE) {  // the update reads X, nn_t: no correspondence record
                const float2 lu = lu_from_sec(__uint_as_float(secl[lane]));
                float4* const xo = &X[orig];
                *xo = make_float4(x, y, z, __uint_as_float(__float_as_uint(lu.x) | lflag));  // .w = L
                w.nn_u[xs0 + orig] = lu.y;
                float4* const to = &w.nn_t[xs0 + orig];
                *to = make_float4(tl_x(t), tl_y(t), tl_z(t), nt_pack((int)tpos, spos));
            } else if (corr) {
                write_corr_t(w, a, p, orig, x, y, z, key_d2(kb), make_float4(tl_x(t), tl_y(t), tl_z(t), 0.f));
            }
        }
        const uint64_t ck3 = __builtin_readcyclecounter();
        rs.ck_setup += ck1 - ck0;
        rs.ck_trav += ck2 - ck1;
        rs.ck_write += ck3 - ck2;
    }
}

}  // namespace icp4r
