// icp4r_index.hip — the index build, once per registration: the kd / Morton order of target and source,
// the block and superblock boxes, and the source order by the target's tree.
#include "icp4r_common.hpp"

namespace icp4r {

// ---------------------------------------------------------------------------------------------
// index_kernel: the pruned search's per-pair index (once per registration; the target never moves
// and a rigid motion keeps the source's spatial order).  blockIdx.x = pair, blockIdx.y = 0 target /
// 1 source.  The order only decides how well blocks prune — the search is exact for any order.
//
//  * n <= kKdMaxN (every scan of the benchmark): a balanced kd-tree order.  Segment [s, e) splits at
//    the median of its widest axis into a left part of floor(units / 2) whole units (unit = one
//    superblock of leaf * kSuper points while the segment is larger than that, else one leaf), so
//    every block of `leaf` consecutive positions is a kd leaf and every superblock a kd subtree.
//    Measured on the benchmark pairs (CPU model of the exact pruning, blocks whose box can reach
//    the second-nearest distance): 2.4 blocks / 1.6 superblocks per query vs 6.6 / 4.7 for the
//    Morton-cell order — the Morton blocks straddle cell boundaries and their boxes are long.
//    Built in LDS with the classic presorted-lists method: the points sorted once per axis
//    (bitonic, unique keys (coordinate, index), so deterministic), then per level a stable
//    partition of all three lists by "left of the split", which keeps each list sorted inside
//    every segment.
//  * larger clouds (the C5 scan-to-map target): a counting sort over 2^14 Morton cells of the
//    bounding box (x, y: 32 cells, z: 16 — radar scans are flat); order inside a cell is whatever
//    the LDS atomics give.
constexpr int kIdxWG = 512;  // two index workgroups per CU (74 KB of LDS each): their barrier-bound levels overlap
constexpr int kIdxWaves = kIdxWG / 64;
constexpr int kKdPer = kKdMaxN / kIdxWG;  // consecutive list positions per thread

constexpr int kKdBins = 2048;             // counting-sort bins per axis (11-bit quantised coordinate)

typedef uint8_t kd_flag_t;  // kd levels: a byte per point flag (one dword per flag measured no change)
struct KdShared {
    uint16_t L[3][kKdMaxN];  // per axis: the point indices, sorted by that axis inside every segment
    union {
        uint32_t hist[3][kKdBins];  // the per-axis counting sorts
        struct {
            kd_flag_t left[kKdMaxN + 4];  // per point: left of its segment's split (+ a junk slot)
            uint16_t tpre[3][kIdxWG];  // per list: exclusive prefix of "left" at each thread's first position
        } p;
        float4 bbox[2 * kKdMaxN / 16];  // index_kernel: block boxes (lo, hi) for the superblock boxes
    } u;
    uint16_t seg_mid[kIdxWG];  // per segment, at the thread owning its first position: split position
    uint8_t seg_ax[kIdxWG];    // ... and axis (3: leaf)
    alignas(16) uint16_t wsum[3][kIdxWaves];
    float red[kIdxWaves][6];
    float lo[3], sc[3];
};

struct MortonShared {
    uint32_t bins[kCellBins];
    float red[kIdxWaves][6];
    uint32_t wsum[kIdxWaves];
    float lo_s[3], sc_s[3];
};

union IndexShared {
    KdShared kd;
    MortonShared mo;
};

// float -> u32 with the same order (finite inputs)
__device__ __forceinline__ uint32_t ord_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The split of segment [s, e) (see above): left part [s, s + h); h = 0 for a leaf.
__device__ __forceinline__ int kd_split(int S, int leaf) {
    if (S <= leaf) return 0;
    const int unit = S > leaf * kSuper ? leaf * kSuper : leaf;
    return (((S + unit - 1) / unit) >> 1) * unit;
}

// Balanced kd order of pts[0, n) (n <= kKdMaxN) into sh.L[0][0, n).  The per-axis orders are
// counting sorts of the coordinate quantised to kKdBins levels over the cloud's extent; the order
// of equal keys (LDS atomics) is arbitrary, which only moves points between the two sides of a
// split among equals — the search is exact for any order.
// kdn (nullable): the tree is also written out for src_order_kernel — the quantisation (lo, scale
// bits at [0, 6)) and every internal node at [8 + heap id] (root 1, children 2i / 2i + 1) as
// 1 << 31 | mid << 13 | axis << 11 | key of the first point right of the split (on its axis); the
// caller zeroes the node slots (0: leaf).
// KPER: list positions per thread in the levels (16 covers kKdMaxN; 8 for clouds of at most
// kKdMaxN / 2 points, so that a level's per-thread LDS work halves).
template <int KPER, typename Get>  // Get: int -> float4, point i of the cloud
__device__ void kd_order(KdShared& sh, Get pts, int n, int leaf, uint64_t* tk, uint32_t* kdn = nullptr,
                         uint16_t* gk = nullptr) {
    static_assert(KPER % 8 == 0 && KPER <= 16 && KPER * kIdxWG >= kKdMaxN / 2, "list positions per thread");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tk) tk[0] = __builtin_amdgcn_s_memrealtime();
    // 1. bounding box -> quantisation.  The thread's points (i = tid + k * kIdxWG) are loaded once,
    // every load in flight together, and kept for the counting sorts: three load-use passes over the
    // cloud had waited out a global round trip per point and pass (45 us of a build under load).
    float px[kKdPer], py[kKdPer], pz[kKdPer];  // (xyz only: whole float4s spilled registers)
#pragma unroll
    for (int k = 0; k < kKdPer; ++k) {
        const float4 v = pts(min(tid + k * kIdxWG, n - 1));
        px[k] = v.x;
        py[k] = v.y;
        pz[k] = v.z;
    }
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int k = 0; k < kKdPer; ++k) {  // (a clamped duplicate of point n - 1 changes no extent)
        const float4 v = make_float4(px[k], py[k], pz[k], 0.0f);
        mn[0] = fminf(mn[0], v.x); mn[1] = fminf(mn[1], v.y); mn[2] = fminf(mn[2], v.z);
        mx[0] = fmaxf(mx[0], v.x); mx[1] = fmaxf(mx[1], v.y); mx[2] = fmaxf(mx[2], v.z);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // (DPP: no ds_bpermute round trips)
        mn[k] = wave_minf(mn[k]);
        mx[k] = wave_maxf(mx[k]);
    }
    if (lane == 0)
        for (int k = 0; k < 3; ++k) {
            sh.red[wave][k] = mn[k];
            sh.red[wave][3 + k] = mx[k];
        }
    for (int b = tid; b < 3 * kKdBins; b += kIdxWG) (&sh.u.hist[0][0])[b] = 0;
    __syncthreads();
    if (tid < 3) {
        float l = INFINITY, h = -INFINITY;
        for (int v = 0; v < kIdxWaves; ++v) {
            l = fminf(l, sh.red[v][tid]);
            h = fmaxf(h, sh.red[v][3 + tid]);
        }
        sh.lo[tid] = l;
        sh.sc[tid] = h > l ? (float)kKdBins / (h - l) : 0.0f;
        if (kdn) {
            kdn[tid] = __float_as_uint(l);
            kdn[3 + tid] = __float_as_uint(sh.sc[tid]);
        }
    }
    __syncthreads();
    const float lo[3] = {sh.lo[0], sh.lo[1], sh.lo[2]}, sc[3] = {sh.sc[0], sh.sc[1], sh.sc[2]};
    auto bin = [&](float c, int ax) { return min(kKdBins - 1, max(0, (int)((c - lo[ax]) * sc[ax]))); };
    // 2. three counting sorts at once: histogram, exclusive scan, scatter
#pragma unroll
    for (int k = 0; k < kKdPer; ++k) {
        if (tid + k * kIdxWG >= n) continue;
        const float4 v = make_float4(px[k], py[k], pz[k], 0.0f);
        atomicAdd(&sh.u.hist[0][bin(v.x, 0)], 1u);
        atomicAdd(&sh.u.hist[1][bin(v.y, 1)], 1u);
        atomicAdd(&sh.u.hist[2][bin(v.z, 2)], 1u);
    }
    __syncthreads();
    {
        constexpr int per = 3 * kKdBins / kIdxWG;  // 6 bins per thread; an axis = 2048 / 6 threads (not whole)
        static_assert(3 * kKdBins % kIdxWG == 0, "bins per thread");
        uint32_t* hb = &sh.u.hist[0][0];
        uint32_t loc[per], run = 0;
        // scan each axis separately: a thread's bins may straddle two axes, so carry the axis start
#pragma unroll
        for (int k = 0; k < per; ++k) {
            const int gb = tid * per + k;
            loc[k] = run;
            run += hb[gb];
        }
        uint32_t incl = run;
        incl = wave_scan_incl(incl);  // (DPP)
        if (lane == 63) sh.red[wave][0] = __uint_as_float(incl);  // (the bbox partials are consumed)
        __syncthreads();
        uint32_t wbase = 0;
        for (int v = 0; v < wave; ++v) wbase += __float_as_uint(sh.red[v][0]);
        const uint32_t tbase = wbase + incl - run;  // exclusive prefix over all 3 axes' bins
        __syncthreads();
#pragma unroll
        for (int k = 0; k < per; ++k) {
            const int gb = tid * per + k;
            hb[gb] = tbase + loc[k] - (uint32_t)(gb / kKdBins) * (uint32_t)n;  // axis a's bins start at a * n
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kKdPer; ++k) {
        const int i = tid + k * kIdxWG;
        if (i >= n) continue;
        const float4 v = make_float4(px[k], py[k], pz[k], 0.0f);
        const int bx = bin(v.x, 0), by = bin(v.y, 1), bz = bin(v.z, 2);
        if (gk) {  // (coalesced: the levels read them back from this XCD's L2)
            gk[i] = (uint16_t)bx;
            gk[kKdMaxN + i] = (uint16_t)by;
            gk[2 * kKdMaxN + i] = (uint16_t)bz;
        }
        sh.L[0][atomicAdd(&sh.u.hist[0][bx], 1u)] = (uint16_t)i;
        sh.L[1][atomicAdd(&sh.u.hist[1][by], 1u)] = (uint16_t)i;
        sh.L[2][atomicAdd(&sh.u.hist[2][bz], 1u)] = (uint16_t)i;
    }
    __syncthreads();
    if (tk) tk[1] = __builtin_amdgcn_s_memrealtime();
    // 3. levels: split every non-leaf segment at the median of its widest axis.  Segment bounds are
    // multiples of 16 >= KPER, so a thread's positions [p0, p0 + KPER) share one segment [s, e),
    // tracked per thread; the thread owning a segment's first position decides its split.
    const int p0 = tid * KPER;
    int s = 0, e = n, node = 1;  // this thread's segment and its heap id
    for (;;) {
        bool any = false;
        if (p0 == s && p0 < n) {
            const int h = kd_split(e - s, leaf);
            uint8_t ax = 3;
            if (h) {
                // the segment's extent per axis from the keys of its first and last point in that axis'
                // list, re-quantised from the (cache-resident) cloud: no per-point key array in LDS
                // (keeping the small clouds' bins in LDS instead was measured: no faster)
                float ext[3];
                if (gk) {  // the quantised keys written above: 2-B reads of an L2-resident 48 KB
                    int kf[3], kl[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        kf[a] = gk[a * kKdMaxN + sh.L[a][s]];
                        kl[a] = gk[a * kKdMaxN + sh.L[a][e - 1]];
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a) ext[a] = (float)(kl[a] - kf[a]) / sc[a];
                } else {
                    float4 pf[3], pl[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        pf[a] = pts(sh.L[a][s]);
                        pl[a] = pts(sh.L[a][e - 1]);
                    }
                    ext[0] = (float)(bin(pl[0].x, 0) - bin(pf[0].x, 0)) / sc[0];
                    ext[1] = (float)(bin(pl[1].y, 1) - bin(pf[1].y, 1)) / sc[1];
                    ext[2] = (float)(bin(pl[2].z, 2) - bin(pf[2].z, 2)) / sc[2];
                }
                ax = ext[0] >= ext[1] && ext[0] >= ext[2] ? 0 : (ext[1] >= ext[2] ? 1 : 2);
                any = true;
                if (kdn && node < kKdNodes) {
                    uint32_t km;
                    if (gk) {
                        km = gk[ax * kKdMaxN + sh.L[ax][s + h]];
                    } else {
                        const float4 pm = pts(sh.L[ax][s + h]);
                        km = (uint32_t)bin(ax == 0 ? pm.x : (ax == 1 ? pm.y : pm.z), ax);
                    }
                    kdn[8 + node] = 0x80000000u | ((uint32_t)(s + h) << 13) | ((uint32_t)ax << 11) | km;
                }
            }
            sh.seg_mid[tid] = (uint16_t)(s + h);
            sh.seg_ax[tid] = ax;
        }
        if (!__syncthreads_or(any)) {
            if (tk) tk[2] = __builtin_amdgcn_s_memrealtime();
            break;
        }
        int mid = 0, ax = 3;
        if (p0 < n) {
            mid = sh.seg_mid[s / KPER];
            ax = sh.seg_ax[s / KPER];
        }
        // this thread's list entries (one 16-B LDS read per list; entries >= n are never used), two
        // u16 entries per register as read (a u16 array went to scratch, 32-bit elements filled the
        // register budget: a spill in every level)
        uint32_t vp[3][KPER / 2];
        static_assert(KPER % 8 == 0, "whole 16-B reads of the lists");
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int q8 = 0; q8 < KPER / 8; ++q8) {
                const uint4 r = *reinterpret_cast<const uint4*>(&sh.L[a][p0 + 8 * q8]);
                vp[a][4 * q8] = r.x;
                vp[a][4 * q8 + 1] = r.y;
                vp[a][4 * q8 + 2] = r.z;
                vp[a][4 * q8 + 3] = r.w;
            }
        auto ent = [&](int a, int k) -> uint32_t { return (vp[a][k >> 1] >> (16 * (k & 1))) & 0xffffu; };
        const int nv = min(KPER, n - p0);  // valid entries (<= 0: none)
        const bool act = nv > 0 && ax < 3;    // this thread's segment splits
        // Every LDS access of the level below is unconditional: a per-entry guard had put a branch and
        // a wait around each (~6 us per level on a single 2k-point build).  Entries past nv (the thread
        // holding position n - 1) may hold anything: their flag goes to the junk slot, their flag reads
        // are masked into range and dropped, and their partition writes land in [n, p0 + KPER).
        if (act) {  // "left" per point, from the split axis' list
            uint32_t va[KPER / 2];  // the split axis' entries, re-read from LDS (a select among the
                                      // registers became a dynamic index: a round trip through scratch)
#pragma unroll
            for (int q8 = 0; q8 < KPER / 8; ++q8) {
                const uint4 r = *reinterpret_cast<const uint4*>(&sh.L[ax][p0 + 8 * q8]);
                va[4 * q8] = r.x;
                va[4 * q8 + 1] = r.y;
                va[4 * q8 + 2] = r.z;
                va[4 * q8 + 3] = r.w;
            }
            const uint32_t lf = p0 < mid ? 1u : 0u;  // (segment bounds and mid are multiples of KPER)
#pragma unroll
            for (int k = 0; k < KPER; ++k) {
                const uint32_t i = (va[k >> 1] >> (16 * (k & 1))) & 0xffffu;
                sh.u.p.left[k < nv ? i : kKdMaxN] = (kd_flag_t)lf;
            }
        }
        __syncthreads();
        // stable partition of the three lists: exclusive prefix of "left" in list order; the flags of
        // this thread's entries as bit masks (the split axis' own read back what this thread wrote)
        uint32_t fb[3] = {0u, 0u, 0u};
        if (act) {
            uint32_t fl[3][KPER];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int k = 0; k < KPER; ++k) fl[a][k] = sh.u.p.left[ent(a, k) & (kKdMaxN - 1)];
            const uint32_t vm = nv >= 32 ? ~0u : (1u << nv) - 1u;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int k = 0; k < KPER; ++k) fb[a] |= fl[a][k] << k;
                fb[a] &= vm;
            }
        }
        const int cnt[3] = {__builtin_popcount(fb[0]), __builtin_popcount(fb[1]), __builtin_popcount(fb[2])};
        int incl[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) incl[a] = (int)wave_scan_incl((uint32_t)cnt[a]);  // (DPP)
        if (lane == 63)
#pragma unroll
            for (int a = 0; a < 3; ++a) sh.wsum[a][wave] = (uint16_t)incl[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) sh.u.p.tpre[a][tid] = (uint16_t)(incl[a] - cnt[a]);  // in-wave exclusive
        __syncthreads();  // wave totals and in-wave prefixes visible; every thread holds its entries in v
        const int sw = (s / KPER) >> 6;  // the wave owning the segment's first position
        if (act) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (a == ax) continue;  // already partitioned: every entry stays where it is
                // the wave totals before `wave` and before `sw` (u16 each, 16-B LDS reads)
                static_assert(kIdxWaves % 8 == 0 && kIdxWaves <= 16, "wave totals in whole 16-B reads");
                uint32_t ww[kIdxWaves / 2];
#pragma unroll
                for (int q8 = 0; q8 < kIdxWaves / 8; ++q8) {
                    const uint4 r = *reinterpret_cast<const uint4*>(&sh.wsum[a][8 * q8]);
                    ww[4 * q8] = r.x; ww[4 * q8 + 1] = r.y; ww[4 * q8 + 2] = r.z; ww[4 * q8 + 3] = r.w;
                }
                int bw = 0, bs = 0;
#pragma unroll
                for (int k = 0; k < kIdxWaves; ++k) {
                    const int c = (int)((ww[k >> 1] >> (16 * (k & 1))) & 0xffffu);
                    bw += k < wave ? c : 0;
                    bs += k < sw ? c : 0;
                }
                // "left" points before p0 inside the segment
                int ones = (bw + incl[a] - cnt[a]) - (bs + (int)sh.u.p.tpre[a][s / KPER]);
#pragma unroll
                for (int k = 0; k < KPER; ++k) {
                    const int f = (fb[a] >> k) & 1;
                    const int np = f ? s + ones : mid + (p0 + k - s) - ones;
                    ones += f;
                    sh.L[a][np] = (uint16_t)ent(a, k);
                }
            }
            if (p0 < mid) {
                e = mid;
                node = 2 * node;
            } else {
                s = mid;
                node = 2 * node + 1;
            }
        }
        __syncthreads();
    }
}

__device__ void index_boxes(const WorkArgs& w, int p, int n) {
    const int tid = threadIdx.x;
    float4* ts = w.tsort + (int64_t)p * w.t_stride;
    __syncthreads();  // workgroup-scope release/acquire: the scatter above is visible to this WG
    // 5. tail duplicates, block boxes, superblock boxes
    // padding: +inf coordinates (d² = +inf never beats a real target, and no padding entry
    // can pose as a second-nearest duplicate of a real one); .w = the last target's index
    const float4 last = ts[n - 1];
    for (int64_t pos = n + tid; pos < w.t_stride; pos += kIdxWG) ts[pos] = make_float4(INFINITY, INFINITY, INFINITY, last.w);
    const int B = w.leaf;
    const int nb = (n + B - 1) / B;
    float4* tb = w.tbox + (int64_t)p * 2 * w.b_stride;
    // (each block's points, and each superblock's block boxes, loaded all at once: a load-use loop
    // had waited out one round trip per point — 8 blocks x 16 points per thread for a 65k-point map)
    constexpr int kHalf = 16;  // w.leaf: 16 or 32 points, 16 at a time
    for (int b = tid; b < w.b_stride; b += kIdxWG) {
        float4 l = make_float4(INFINITY, INFINITY, INFINITY, 0.f), h = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        if (b < nb) {
            const int e = min(n, (b + 1) * B) - 1;  // the block's last real point
            for (int h0 = 0; h0 < B; h0 += kHalf) {
                float vx[kHalf], vy[kHalf], vz[kHalf];
#pragma unroll
                for (int k = 0; k < kHalf; ++k) {  // (repeats of the last point: no change)
                    const float4 v = ts[min(b * B + h0 + k, e)];
                    vx[k] = v.x;
                    vy[k] = v.y;
                    vz[k] = v.z;
                }
#pragma unroll
                for (int k = 0; k < kHalf; ++k) {
                    l.x = fminf(l.x, vx[k]); l.y = fminf(l.y, vy[k]); l.z = fminf(l.z, vz[k]);
                    h.x = fmaxf(h.x, vx[k]); h.y = fmaxf(h.y, vy[k]); h.z = fmaxf(h.z, vz[k]);
                }
            }
        }
        tb[2 * b] = l;
        tb[2 * b + 1] = h;
    }
    __syncthreads();  // workgroup-scope release/acquire: the scatter above is visible to this WG
    float4* sbx = w.sbox + (int64_t)p * 2 * w.sb_stride;
    for (int s = tid; s < w.sb_stride; s += kIdxWG) {
        float4 l = make_float4(INFINITY, INFINITY, INFINITY, 0.f), h = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        float4 bb[2 * kSuper];
#pragma unroll
        for (int k = 0; k < 2 * kSuper; ++k) bb[k] = tb[2 * s * kSuper + k];
#pragma unroll
        for (int k = 0; k < kSuper; ++k) {
            const float4 bl = bb[2 * k], bh = bb[2 * k + 1];
            l.x = fminf(l.x, bl.x); l.y = fminf(l.y, bl.y); l.z = fminf(l.z, bl.z);
            h.x = fmaxf(h.x, bh.x); h.y = fmaxf(h.y, bh.y); h.z = fmaxf(h.z, bh.z);
        }
        sbx[2 * s] = l;
        sbx[2 * s + 1] = h;
    }
}

// One cloud's index (the target or the source of pair p) by one workgroup: index_kernel, and the
// source column of index_refine_kernel when the target's Morton sort is multi-workgroup (w.mo_hist).
__device__ __forceinline__ void index_cloud(IndexShared& shu, const PairArgs& a, const WorkArgs& w, int p, bool is_tgt) {
    if (w.state[p].phase == kPhaseInvalid) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = is_tgt ? a.tgt_n[p] : a.src_n[p];
    if (n <= 0) return;
    const float4* pts = is_tgt ? a.tgt + a.tgt_off[p] : a.src + a.src_off[p];
    if (!is_tgt && src_by_tgt_tree(a, w, p)) return;  // src_order_kernel orders it
    if ((w.kd_index & (is_tgt ? 1 : 2)) && n <= kKdMaxN && (!is_tgt || w.t_stride <= kKdMaxN)) {
#if ICP4R_WG_TICKS  // diagnostic build: every cloud's build start / end and XCC / CU (tools/experiments/idx_ticks.py)
        uint64_t* it = (w.ticks && tid == 0) ? w.ticks + 32 + 12 * (int64_t)gridDim.x + 8 * (int64_t)p + (is_tgt ? 0 : 4) : nullptr;
        if (it) {
            it[0] = __builtin_amdgcn_s_memrealtime();
            it[2] = (uint64_t)(uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
                    ((uint64_t)(uint32_t)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
        }
#endif
        uint64_t* tk = (w.ticks && p == 0 && is_tgt && tid == 0) ? w.ticks + 12 : nullptr;
        uint32_t* kdn = (is_tgt && w.kdn && w.src_by_tgt) ? w.kdn + (int64_t)p * kKdnStride : nullptr;
        if (kdn)
            for (int k = tid; k < kKdnStride; k += kIdxWG) kdn[k] = 0u;  // (kd_order syncs before writing)
        // the quantised keys' scratch (3 x kKdMaxN u16): the pair's query-record area, unused until
        // the source order / first search writes it; the kd levels read the keys from this copy, not the points
        // (targets only: a pair's source build may run beside it on the same area)
        uint16_t* gk = (is_tgt && w.qv && (int64_t)w.x_stride * (int64_t)sizeof(float4) >= 3 * kKdMaxN * 2)
                           ? reinterpret_cast<uint16_t*>(w.qv + (int64_t)p * w.x_stride)
                           : nullptr;
        if (n <= kKdMaxN / 2)
            kd_order<8>(shu.kd, [&](int i) { return pts[i]; }, n, is_tgt ? w.leaf : 16, tk, kdn, gk);
        else
            kd_order<16>(shu.kd, [&](int i) { return pts[i]; }, n, is_tgt ? w.leaf : 16, tk, kdn, gk);
        const uint16_t* ord = shu.kd.L[0];
        if (is_tgt) {
            // sorted targets, padding (+inf coordinates, .w = the last target's index: never a match,
            // never a second-nearest duplicate), and block boxes reduced over `leaf` adjacent lanes
            float4* ts = w.tsort + (int64_t)p * w.t_stride;
            int32_t* tinv = w.tinv + (int64_t)p * w.t_stride;
            float4* tb = w.tbox + (int64_t)p * 2 * w.b_stride;
            const float lastw = __uint_as_float((uint32_t)ord[n - 1]);
            const int B = w.leaf;
            // The coordinates by sorted position come through LDS, not a gather pts[ord[pos]] (16-B
            // reads of 64-B lines: 4.6x the cloud fetched): every position's point writes its inverse
            // (tinv, here coalesced by point), each thread re-reads its own points in index order, and
            // a quarter of the positions at a time is staged in the free axis lists L[1..2] (x, y, z
            // rows) and written out by position.  (t_stride <= kKdMaxN here and a multiple of 64, so
            // the position guard is wave-uniform: the shuffles below see every lane.)
            uint16_t* inv = shu.kd.L[1];
#pragma unroll
            for (int k = 0; k < kKdPer; ++k) {
                const int pos = tid + k * kIdxWG;
                if (pos < n) inv[ord[pos]] = (uint16_t)pos;
            }
            __syncthreads();
            float px[kKdPer], py[kKdPer], pz[kKdPer];
            uint32_t pos2[kKdPer / 2];  // the thread's points' positions, two per dword (0xffff: none)
#pragma unroll
            for (int k = 0; k < kKdPer; ++k) {
                const float4 c = pts[min(tid + k * kIdxWG, n - 1)];
                px[k] = c.x;
                py[k] = c.y;
                pz[k] = c.z;
            }
#pragma unroll
            for (int k = 0; k < kKdPer; ++k) {
                const int i = tid + k * kIdxWG;
                const uint32_t ps = i < n ? (uint32_t)inv[i] : 0xffffu;
                if (i < n) tinv[i] = (int32_t)ps;
                if ((k & 1) == 0)
                    pos2[k >> 1] = ps;
                else
                    pos2[k >> 1] |= ps << 16;
            }
            constexpr int kQ = kKdMaxN / 4;  // positions per quarter: 3 rows of kQ floats (24 KB of L[1..2])
            static_assert(3 * kQ * 4 <= 2 * kKdMaxN * 2, "staging rows in L[1], L[2]");
            float* rx = reinterpret_cast<float*>(&shu.kd.L[1][0]);
            float* ry = rx + kQ;
            float* rz = ry + kQ;
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                __syncthreads();  // (inv / the previous quarter's rows read)
#pragma unroll
                for (int k = 0; k < kKdPer / 2; ++k) asm volatile("" : "+v"(pos2[k]));  // (nothing hoisted)
#pragma unroll
                for (int k = 0; k < kKdPer; ++k) {
                    const uint32_t r = ((pos2[k >> 1] >> (16 * (k & 1))) & 0xffffu) - (uint32_t)(q * kQ);
                    if (r < (uint32_t)kQ) {
                        rx[r] = px[k];
                        ry[r] = py[k];
                        rz[r] = pz[k];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < kQ / kIdxWG; ++kk) {
                    const int k = q * (kQ / kIdxWG) + kk;
                    const int pos = tid + k * kIdxWG;
                    if (pos < (int)w.t_stride) {
                        float4 v = make_float4(INFINITY, INFINITY, INFINITY, lastw);
                        float4 l = v, h = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
                        if (pos < n) {
                            const int o = pos - q * kQ;
                            v = make_float4(rx[o], ry[o], rz[o], __uint_as_float((uint32_t)ord[pos]));
                            l = v;
                            h = v;
                        }
                        ts[pos] = v;
                        l.x = seg_minf(l.x, B); h.x = seg_maxf(h.x, B);
                        l.y = seg_minf(l.y, B); h.y = seg_maxf(h.y, B);
                        l.z = seg_minf(l.z, B); h.z = seg_maxf(h.z, B);
                        if ((lane & (B - 1)) == 0) {
                            const int b = pos / B;
                            l.w = 0.f;
                            h.w = 0.f;
                            tb[2 * b] = l;
                            tb[2 * b + 1] = h;
                            shu.kd.u.bbox[2 * b] = l;
                            shu.kd.u.bbox[2 * b + 1] = h;
                        }
                    }
                }
            }
            __syncthreads();
            float4* sbx = w.sbox + (int64_t)p * 2 * w.sb_stride;
            for (int sb = tid; sb < w.sb_stride; sb += kIdxWG) {
                float4 l = make_float4(INFINITY, INFINITY, INFINITY, 0.f), h = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
                for (int b = sb * kSuper; b < (sb + 1) * kSuper; ++b) {
                    const float4 bl = shu.kd.u.bbox[2 * b], bh = shu.kd.u.bbox[2 * b + 1];
                    l.x = fminf(l.x, bl.x); l.y = fminf(l.y, bl.y); l.z = fminf(l.z, bl.z);
                    h.x = fmaxf(h.x, bh.x); h.y = fmaxf(h.y, bh.y); h.z = fmaxf(h.z, bh.z);
                }
                sbx[2 * sb] = l;
                sbx[2 * sb + 1] = h;
            }
            if (tk) tk[3] = __builtin_amdgcn_s_memrealtime();
        } else {
            int32_t* sp = w.sperm + (int64_t)p * w.x_stride;
            for (int pos = tid; pos < n; pos += kIdxWG) sp[pos] = ord[pos];
        }
#if ICP4R_WG_TICKS
        __syncthreads();
        if (it) it[1] = __builtin_amdgcn_s_memrealtime();
#endif
        return;
    }
    if (is_tgt && w.mo_hist) return;  // index_mo_hist_kernel / index_mo_scatter_kernel sort it
    uint32_t* bins = shu.mo.bins;
    float(*red)[6] = shu.mo.red;
    uint32_t* wsum = shu.mo.wsum;
    float* lo_s = shu.mo.lo_s;
    float* sc_s = shu.mo.sc_s;
    // Large clouds (the scan-to-map target): every pass over the cloud keeps kMoPer points per thread
    // in flight (a load-use loop had waited out one round trip per 512 points: 3 x 128 of them for a
    // 65k-point map, ~140 us of a single registration)
    constexpr int kMoPer = 16;
    auto sweep = [&](auto&& f) {
        for (int i0 = 0; i0 < n; i0 += kIdxWG * kMoPer) {
            float4 v[kMoPer];
#pragma unroll
            for (int e = 0; e < kMoPer; ++e) v[e] = pts[min(i0 + e * kIdxWG + tid, n - 1)];
#pragma unroll
            for (int e = 0; e < kMoPer; ++e)
                if (i0 + e * kIdxWG + tid < n) f(i0 + e * kIdxWG + tid, v[e]);
        }
    };
    // 1. bounding box (a target's from init_kernel's validation pass: one pass over the cloud fewer)
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (is_tgt && w.tbb) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = w.tbb[(int64_t)p * 8 + k];
            mx[k] = w.tbb[(int64_t)p * 8 + 3 + k];
        }
    } else {
        sweep([&](int, const float4& v) {
            mn[0] = fminf(mn[0], v.x); mn[1] = fminf(mn[1], v.y); mn[2] = fminf(mn[2], v.z);
            mx[0] = fmaxf(mx[0], v.x); mx[1] = fmaxf(mx[1], v.y); mx[2] = fmaxf(mx[2], v.z);
        });
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // (DPP: no ds_bpermute round trips)
        mn[k] = wave_minf(mn[k]);
        mx[k] = wave_maxf(mx[k]);
    }
    if (lane == 0)
        for (int k = 0; k < 3; ++k) {
            red[wave][k] = mn[k];
            red[wave][3 + k] = mx[k];
        }
    for (int b = tid; b < kCellBins; b += kIdxWG) bins[b] = 0;
    __syncthreads();
    if (tid < 3) {
        float l = INFINITY, h = -INFINITY;
        for (int v = 0; v < kIdxWaves; ++v) {
            l = fminf(l, red[v][tid]);
            h = fmaxf(h, red[v][3 + tid]);
        }
        const float cells = tid == 2 ? 16.0f : 32.0f;
        lo_s[tid] = l;
        sc_s[tid] = h > l ? cells / (h - l) : 0.0f;
    }
    __syncthreads();
    float lo[3] = {lo_s[0], lo_s[1], lo_s[2]}, sc[3] = {sc_s[0], sc_s[1], sc_s[2]};
    // 2. histogram of cell codes
    sweep([&](int, const float4& v) { atomicAdd(&bins[cell_code(v.x, v.y, v.z, lo, sc)], 1u); });
    __syncthreads();
    // 3. exclusive scan: thread t owns bins [16 t, 16 t + 16)
    constexpr int per = kCellBins / kIdxWG;
    uint32_t loc[per], run = 0;
#pragma unroll
    for (int k = 0; k < per; ++k) {
        loc[k] = run;
        run += bins[tid * per + k];
    }
    uint32_t incl = run;
    incl = wave_scan_incl(incl);  // (DPP)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int v = 0; v < wave; ++v) wbase += wsum[v];
    const uint32_t tbase = wbase + incl - run;
#pragma unroll
    for (int k = 0; k < per; ++k) bins[tid * per + k] = tbase + loc[k];
    __syncthreads();
    // 4. scatter
    if (is_tgt) {
        float4* ts = w.tsort + (int64_t)p * w.t_stride;
        int32_t* tinv = w.tinv + (int64_t)p * w.t_stride;
        sweep([&](int i, const float4& v) {
            const uint32_t pos = atomicAdd(&bins[cell_code(v.x, v.y, v.z, lo, sc)], 1u);
            ts[pos] = make_float4(v.x, v.y, v.z, __uint_as_float((uint32_t)i));
            tinv[i] = (int32_t)pos;
        });
        index_boxes(w, p, n);
    } else {
        int32_t* sp = w.sperm + (int64_t)p * w.x_stride;
        sweep([&](int i, const float4& v) {
            const uint32_t pos = atomicAdd(&bins[cell_code(v.x, v.y, v.z, lo, sc)], 1u);
            sp[pos] = i;
        });
    }
}


// Multi-workgroup Morton sort of a large target (the C5 submap: 65k points), for few pairs: the
// one-workgroup sort above spends ~125 us of a single registration in its three sweeps over the
// cloud.  Workgroup g of pair p owns points [g * kMoChunk, (g + 1) * kMoChunk): one sweep, 16 points
// per thread in flight.  index_mo_hist_kernel writes each workgroup's cell histogram (row p * G + g
// of w.mo_hist); index_mo_scatter_kernel gives every workgroup the exclusive prefix over (cell,
// workgroup) — the cells of all rows before its cell, plus its cell in the rows before its own —
// and scatters its points there.  The quantisation (w.tbb, from init_kernel) is the one-workgroup
// sort's.  Only for plans whose index_refine_kernel re-orders every chunk afterwards (it writes tinv
// and the boxes of every real block); the scatter writes the padding and the empty tail's boxes.
constexpr int kMoChunk = kIdxWG * 16;

__global__ __launch_bounds__(kIdxWG) void index_mo_hist_kernel(PairArgs a, WorkArgs w) {
    __shared__ uint32_t bins[kCellBins];
    const int g = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const int m = a.tgt_n[p];
    if (w.state[p].phase == kPhaseInvalid || m <= 0 || g * kMoChunk >= m) return;
    const float4* pts = a.tgt + a.tgt_off[p];
    float lo[3], sc[3];
    mo_quant(w, p, lo, sc);
    for (int b = tid; b < kCellBins; b += kIdxWG) bins[b] = 0;
    const int i0 = g * kMoChunk;
    float4 v[kMoChunk / kIdxWG];
#pragma unroll
    for (int e = 0; e < kMoChunk / kIdxWG; ++e) v[e] = pts[min(i0 + e * kIdxWG + tid, m - 1)];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kMoChunk / kIdxWG; ++e)
        if (i0 + e * kIdxWG + tid < m) atomicAdd(&bins[cell_code(v[e].x, v[e].y, v[e].z, lo, sc)], 1u);
    __syncthreads();
    // the row as u16 counts (a workgroup's cell holds at most kMoChunk points), 8 cells per 16-B store
    static_assert(kMoChunk < 65536, "u16 cell counts");
    uint4* row = reinterpret_cast<uint4*>(w.mo_hist + ((int64_t)p * w.mo_groups + g) * kCellBins);
    const uint4* b4 = reinterpret_cast<const uint4*>(bins);
    for (int k = tid; k < kCellBins / 8; k += kIdxWG) {
        const uint4 lo4 = b4[2 * k], hi4 = b4[2 * k + 1];
        row[k] = make_uint4(lo4.x | lo4.y << 16, lo4.z | lo4.w << 16, hi4.x | hi4.y << 16, hi4.z | hi4.w << 16);
    }
}

__global__ __launch_bounds__(kIdxWG) void index_mo_scatter_kernel(PairArgs a, WorkArgs w) {
    __shared__ uint32_t bins[kCellBins];
    __shared__ uint32_t wsum[kIdxWaves];
    const int g = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.tgt_n[p];
    if (w.state[p].phase == kPhaseInvalid || m <= 0 || g * kMoChunk >= m) return;
    const int ng = (m + kMoChunk - 1) / kMoChunk;  // rows of this pair
    const float4* pts = a.tgt + a.tgt_off[p];
    const int i0 = g * kMoChunk;
    float4 v[kMoChunk / kIdxWG];  // this workgroup's points, in flight while the prefix is formed
#pragma unroll
    for (int e = 0; e < kMoChunk / kIdxWG; ++e) v[e] = pts[min(i0 + e * kIdxWG + tid, m - 1)];
    // thread t owns cells [per * t, per * (t + 1)): per cell its count over every row (tot) and over the
    // rows before g (bef); u16 counts, eight cells per 16-B read, kMoRows rows' reads in flight at once
    // (a row at a time had waited out one L2 round trip per row: ~15 us of a 65k-point sort)
    constexpr int per = kCellBins / kIdxWG;
    constexpr int kMoRows = 3;
    static_assert(per % 8 == 0, "whole 16-B reads of the rows");
    uint32_t tot[per], bef[per];
#pragma unroll
    for (int k = 0; k < per; ++k) tot[k] = bef[k] = 0u;
    const uint16_t* rows = w.mo_hist + (int64_t)p * w.mo_groups * kCellBins + tid * per;
    for (int r0 = 0; r0 < ng; r0 += kMoRows) {
        uint4 c[kMoRows][per / 8];
#pragma unroll
        for (int j = 0; j < kMoRows; ++j) {
            const uint4* rr = reinterpret_cast<const uint4*>(rows + (int64_t)min(r0 + j, ng - 1) * kCellBins);
#pragma unroll
            for (int q = 0; q < per / 8; ++q) c[j][q] = rr[q];
        }
#pragma unroll
        for (int j = 0; j < kMoRows; ++j) {
            const uint32_t use = r0 + j < ng ? 0xffffffffu : 0u, into_bef = r0 + j < g ? 0xffffffffu : 0u;
#pragma unroll
            for (int q = 0; q < per / 8; ++q) {
                const uint32_t u[4] = {c[j][q].x & use, c[j][q].y & use, c[j][q].z & use, c[j][q].w & use};
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    const uint32_t cnt = (u[h >> 1] >> (16 * (h & 1))) & 0xffffu;
                    tot[8 * q + h] += cnt;
                    bef[8 * q + h] += cnt & into_bef;
                }
            }
        }
    }
    uint32_t run = 0;
#pragma unroll
    for (int k = 0; k < per; ++k) {  // bef[k] := exclusive prefix of cell k inside the thread + its rows before g
        const uint32_t t = tot[k];
        bef[k] += run;
        run += t;
    }
    uint32_t incl = run;
    incl = wave_scan_incl(incl);  // (DPP)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t tbase = incl - run;
    for (int q = 0; q < wave; ++q) tbase += wsum[q];
    int32_t* rep = w.mo_rep ? w.mo_rep + (int64_t)p * kCellBins : nullptr;
#pragma unroll
    for (int k = 0; k < per; ++k) {
        bins[tid * per + k] = tbase + bef[k];
        if (rep && g == 0 && tot[k] == 0) rep[tid * per + k] = -1;  // (the others: a point's index, below)
    }
    __syncthreads();
    float lo[3], sc[3];
    mo_quant(w, p, lo, sc);
    float4* ts = w.tsort + (int64_t)p * w.t_stride;
#pragma unroll
    for (int e = 0; e < kMoChunk / kIdxWG; ++e) {
        const int i = i0 + e * kIdxWG + tid;
        if (i < m) {
            const uint32_t cell = cell_code(v[e].x, v[e].y, v[e].z, lo, sc);
            const uint32_t pos = atomicAdd(&bins[cell], 1u);
            ts[pos] = make_float4(v[e].x, v[e].y, v[e].z, __uint_as_float((uint32_t)i));
            if (rep) rep[cell] = i;  // (any of the cell's points: the last store wins)
        }
    }
    if (g != ng - 1) return;
    // the tail: padding (+inf coordinates, .w = a real index: never a match) and the boxes of the
    // blocks and superblocks past the last real block (index_refine_kernel writes the real ones)
    for (int64_t pos = m + tid; pos < w.t_stride; pos += kIdxWG)
        ts[pos] = make_float4(INFINITY, INFINITY, INFINITY, __uint_as_float((uint32_t)(m - 1)));
    const int nb = (m + w.leaf - 1) / w.leaf, nsb = (nb + kSuper - 1) / kSuper;
    const float4 el = make_float4(INFINITY, INFINITY, INFINITY, 0.f), eh = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    float4* tb = w.tbox + (int64_t)p * 2 * w.b_stride;
    for (int64_t b = nb + tid; b < w.b_stride; b += kIdxWG) {
        tb[2 * b] = el;
        tb[2 * b + 1] = eh;
    }
    float4* sbx = w.sbox + (int64_t)p * 2 * w.sb_stride;
    for (int64_t s = nsb + tid; s < w.sb_stride; s += kIdxWG) {
        sbx[2 * s] = el;
        sbx[2 * s + 1] = eh;
    }
}

// src_order_kernel: one workgroup per pair whose target has the kd order (src_by_tgt_tree).  Every
// source point descends the target's kd tree (the quantised key of the node's axis against the key of
// the first point right of the split; equal keys sit on both sides, so they may go either way — the
// order only decides how well the search prunes), and a counting sort by the leaf reached gives the
// source order (sperm): consecutive queries fall in the same or neighbouring target leaves, so
// query runs stay compact, and the leaf's first target seeds the query's first search (nn_key with
// d² = +inf, read by the first pass).  It replaces the source's own kd build (index_kernel).
constexpr int kSoWG = 512;

struct SoShared {
    uint32_t nodes[kKdNodes];
    uint32_t bins[kKdMaxN / 16];
    uint32_t wsum[kSoWG / 64];
    float qz[6];
    uint32_t sl[kKdMaxN];  // stage_first: a quarter of the sorted positions' records
};
__device__ void src_order_pair(const PairArgs& a, const WorkArgs& w, int p, SoShared& so) {
    uint32_t* nodes = so.nodes;
    uint32_t* bins = so.bins;
    uint32_t* wsum = so.wsum;
    float* qz = so.qz;
    uint32_t* sl = so.sl;
    if (w.state[p].phase == kPhaseInvalid || !src_by_tgt_tree(a, w, p)) return;
    const int n = a.src_n[p], m = a.tgt_n[p];
    if (n <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#if ICP4R_WG_TICKS  // diagnostic build: this pair's source-order start / end (the index stamps' source slots)
    uint64_t* it = (w.ticks && tid == 0) ? w.ticks + 32 + 12 * (int64_t)gridDim.x + 8 * (int64_t)p + 4 : nullptr;
    if (it) {
        it[0] = __builtin_amdgcn_s_memrealtime();
        it[2] = (uint64_t)(uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
                ((uint64_t)(uint32_t)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
    }
#endif
    const int B = w.leaf;
    const int nb = (m + B - 1) / B;  // <= kKdMaxN / 16
    const uint32_t* kd = w.kdn + (int64_t)p * kKdnStride;
    {
        uint32_t nv[kKdNodes / kSoWG];  // every load before the first store
#pragma unroll
        for (int k = 0; k < kKdNodes / kSoWG; ++k) nv[k] = kd[8 + tid + k * kSoWG];
#pragma unroll
        for (int k = 0; k < kKdNodes / kSoWG; ++k) nodes[tid + k * kSoWG] = nv[k];
    }
    if (tid < 6) qz[tid] = __uint_as_float(kd[tid]);
    for (int b = tid; b < kKdMaxN / 16; b += kSoWG) bins[b] = 0u;
    __syncthreads();
    const float lo[3] = {qz[0], qz[1], qz[2]}, sc[3] = {qz[3], qz[4], qz[5]};
    // Every thread's points (i = tid + e * kSoWG) descend in groups of kSoGrp: their loads all in
    // flight together and the descents interleaved level by level (independent LDS chains) — a
    // point-at-a-time loop had waited out a global round trip and 9 dependent LDS reads per point.
    // The points are X (the guess-transformed sources the first pass searches; init_kernel wrote
    // them), in index order: the leaves stay in registers (two per dword) for the scatter.
    const float4* X = w.X + (int64_t)p * w.x_stride;
    constexpr int kSoPer = kKdMaxN / kSoWG, kSoGrp = 8;
    static_assert(kSoPer % kSoGrp == 0 && kSoPer % 2 == 0, "point groups");
    uint32_t lv[kSoPer / 2];
#pragma unroll
    for (int g = 0; g < kSoPer; g += kSoGrp) {
        float4 v[kSoGrp];
#pragma unroll
        for (int e = 0; e < kSoGrp; ++e) v[e] = X[min(tid + (g + e) * kSoWG, n - 1)];
        int key3[kSoGrp][3], node[kSoGrp], sp[kSoGrp];
#pragma unroll
        for (int e = 0; e < kSoGrp; ++e) {
            key3[e][0] = min(kKdBins - 1, max(0, (int)((v[e].x - lo[0]) * sc[0])));
            key3[e][1] = min(kKdBins - 1, max(0, (int)((v[e].y - lo[1]) * sc[1])));
            key3[e][2] = min(kKdBins - 1, max(0, (int)((v[e].z - lo[2]) * sc[2])));
            node[e] = 1;
            sp[e] = 0;
        }
        for (int lvl = 0; lvl < 11; ++lvl) {  // heap ids < kKdNodes = 2^11
            uint32_t nd[kSoGrp];  // the group's node reads all issued, then branch-free steps
#pragma unroll
            for (int e = 0; e < kSoGrp; ++e) nd[e] = nodes[min(node[e], kKdNodes - 1)];
#pragma unroll
            for (int e = 0; e < kSoGrp; ++e) {
                const bool inner = node[e] < kKdNodes && (nd[e] >> 31);
                const uint32_t ax = (nd[e] >> 11) & 3u;
                const int k = ax == 0u ? key3[e][0] : (ax == 1u ? key3[e][1] : key3[e][2]);
                const bool right = k >= (int)(nd[e] & 2047u);
                sp[e] = (inner && right) ? (int)((nd[e] >> 13) & 0x3fffu) : sp[e];
                node[e] = inner ? 2 * node[e] + (right ? 1 : 0) : kKdNodes;  // a leaf: done
            }
        }
#pragma unroll
        for (int e = 0; e < kSoGrp; ++e) {
            const uint32_t leaf = (uint32_t)min(sp[e] / B, nb - 1);
            if (tid + (g + e) * kSoWG < n) atomicAdd(&bins[leaf], 1u);
            if ((e & 1) == 0)
                lv[(g + e) >> 1] = leaf;
            else
                lv[(g + e) >> 1] |= leaf << 16;
        }
    }
    __syncthreads();
#if ICP4R_WG_TICKS
    if (it) it[3] = __builtin_amdgcn_s_memrealtime();
#endif
    {  // exclusive scan of the nb bins: thread t owns bins [2t, 2t + 2)
        constexpr int per = kKdMaxN / 16 / kSoWG;
        uint32_t loc[per], run = 0;
#pragma unroll
        for (int k = 0; k < per; ++k) {
            loc[k] = run;
            run += bins[tid * per + k];
        }
        uint32_t incl = run;
        incl = wave_scan_incl(incl);  // (DPP)
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t base = 0;
        for (int v = 0; v < wave; ++v) base += wsum[v];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < per; ++k) bins[tid * per + k] = base + incl - run + loc[k];
    }
    __syncthreads();
    int32_t* spm = w.sperm + (int64_t)p * w.x_stride;
    NNKey* key = w.nn_key + (int64_t)p * w.x_stride;
    const float4* ts = w.tsort + (int64_t)p * w.t_stride;
    if (w.stage_first) {
        // The batched search's first-pass query records in sorted order: {X_i, U = +inf} and
        // {i | its position << kNtPosShift, the seed = its leaf's first target position} — the
        // search takes them as they are instead of gathering X through sperm at every work item
        // (a chain of dependent global round trips in front of each pair's first search).  Every
        // record is written in position order (scattered 24-B record stores had cost more than the
        // search saved), from LDS, a quarter of the positions at a time: each thread puts its own
        // points' records (x, y, z, i | leaf << 14) at their positions in the quarter, then the
        // quarter is stored coalesced.  (A gather of X by sorted position instead fetched 4x
        // the cloud: 16-B reads of 64-B lines.)
        // (the coordinates read again, from the L2: kept from the descent they cost occupancy)
        float px[kSoPer], py[kSoPer], pz[kSoPer];
#pragma unroll
        for (int g = 0; g < kSoPer; ++g) {
            const float4 v = X[min(tid + g * kSoWG, n - 1)];
            px[g] = v.x;
            py[g] = v.y;
            pz[g] = v.z;
        }
        uint32_t pos2[kSoPer / 2];  // the points' sorted positions, two per dword
#pragma unroll
        for (int g = 0; g < kSoPer; ++g) {
            const int i = tid + g * kSoWG;
            const uint32_t leaf = (lv[g >> 1] >> (16 * (g & 1))) & 0xffffu;
            const uint32_t ps = i < n ? atomicAdd(&bins[leaf], 1u) : 0xffffu;
            if ((g & 1) == 0)
                pos2[g >> 1] = ps;
            else
                pos2[g >> 1] |= ps << 16;
        }
        constexpr int kQ = kKdMaxN / 4;  // positions per quarter: 4 rows of kQ words in sl's 32 KB
        float* rx = reinterpret_cast<float*>(sl);  // (rows, not 16-B records: a record's 4-register
        float* ry = rx + kQ;                       //  tuples, hoisted out of the quarter loop,
        float* rz = ry + kQ;                       //  took 64 registers)
        uint32_t* rw = sl + 3 * kQ;
        float4* qv = w.qv + (int64_t)p * w.x_stride;
        uint2* qm = w.qm + (int64_t)p * w.x_stride;
        for (int q0 = 0; q0 < n; q0 += kQ) {
            __syncthreads();  // (the previous quarter's records read)
#pragma unroll
            for (int k = 0; k < kSoPer / 2; ++k) asm volatile("" : "+v"(pos2[k]), "+v"(lv[k]));  // (nothing derived from them hoisted: registers)
#pragma unroll
            for (int g = 0; g < kSoPer; ++g) {
                const uint32_t ps = (pos2[g >> 1] >> (16 * (g & 1))) & 0xffffu;
                const uint32_t leaf = (lv[g >> 1] >> (16 * (g & 1))) & 0xffffu;
                const uint32_t r = ps - (uint32_t)q0;
                if (r < (uint32_t)kQ) {
                    rx[r] = px[g];
                    ry[r] = py[g];
                    rz[r] = pz[g];
                    rw[r] = (uint32_t)(tid + g * kSoWG) | (leaf << kNtPosShift);
                }
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < kQ / kSoWG; ++e) {
                const int pos = q0 + tid + e * kSoWG;
                if (pos >= n) continue;
                const int o = tid + e * kSoWG;
                const uint32_t e8 = rw[o];
                const uint32_t i = e8 & kNtIdxMask, leaf = e8 >> kNtPosShift;
                spm[pos] = (int32_t)i;
                qv[pos] = make_float4(rx[o], ry[o], rz[o], INFINITY);
                qm[pos] = make_uint2(i | ((uint32_t)pos << kNtPosShift), leaf * (uint32_t)B);
            }
        }
#if ICP4R_WG_TICKS
        __syncthreads();
        if (it) it[1] = __builtin_amdgcn_s_memrealtime();
#endif
        return;
    }
#pragma unroll
    for (int g = 0; g < kSoPer; g += kSoGrp) {
        float sw[kSoGrp];  // the leaves' first targets' index bits (first-pass seeds), loads in flight together
#pragma unroll
        for (int e = 0; e < kSoGrp; ++e) {
            const uint32_t leaf = (lv[(g + e) >> 1] >> (16 * ((g + e) & 1))) & 0xffffu;
            sw[e] = ts[leaf * B].w;
        }
#pragma unroll
        for (int e = 0; e < kSoGrp; ++e) {
            const int i = tid + (g + e) * kSoWG;
            if (i >= n) continue;
            const uint32_t leaf = (lv[(g + e) >> 1] >> (16 * ((g + e) & 1))) & 0xffffu;
            const uint32_t pos = atomicAdd(&bins[leaf], 1u);
            spm[pos] = i;
            key[i] = make_key(INFINITY, __float_as_uint(sw[e]));  // first-pass seed: the leaf's first target
        }
    }
#if ICP4R_WG_TICKS
    __syncthreads();
    if (it) it[1] = __builtin_amdgcn_s_memrealtime();
#endif
}

__global__ __launch_bounds__(kSoWG) void src_order_kernel(PairArgs a, WorkArgs w) {
    __shared__ SoShared so;
    src_order_pair(a, w, xcd_remap(blockIdx.x, gridDim.x), so);
}

static_assert(sizeof(SoShared) <= sizeof(IndexShared) && kSoWG == kIdxWG, "the source order reuses the index build's workgroup");
__global__ __launch_bounds__(kIdxWG, 4) void index_kernel(PairArgs a, WorkArgs w) {
    __shared__ IndexShared shu;
    // grid (pairs, 2): target and source of every pair; (pairs, 1): targets only, every source
    // ordered by its target's tree — by this workgroup right after the build (fused source order:
    // one launch and one kernel boundary fewer, the tree read back while it is in this XCD's L2)
    const int g = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int p = gridDim.y == 2 ? g >> 1 : g;
    const bool is_tgt = gridDim.y == 2 ? (g & 1) == 0 : true;
    index_cloud(shu, a, w, p, is_tgt);
    if (gridDim.y == 1) {
        __syncthreads();  // the tree (kdn) and sorted targets written; the LDS free
        src_order_pair(a, w, p, *reinterpret_cast<SoShared*>(&shu));
    }
}

// One cloud's index alone (as the target of pair p: no source column, no source order) — the GICP
// source's own index for its k-NN covariances, built on buffers of its own beside the target's chain.
__global__ __launch_bounds__(kIdxWG, 4) void index_cloud_kernel(PairArgs a, WorkArgs w) {
    __shared__ IndexShared shu;
    index_cloud(shu, a, w, xcd_remap(blockIdx.x, gridDim.x), true);
}

// index_refine_kernel: targets too large for the in-LDS kd build (the C5 scan-to-map submap) are
// Morton-sorted by index_kernel, then every 8192-position chunk of that order is re-ordered as a
// balanced kd-tree on its own (one workgroup per chunk, the same builder): superblocks and blocks —
// the units the search prunes with — become kd subtrees and leaves, only the chunk boundaries (every
// 64 superblocks) stay Morton cuts.  Block and superblock boxes of the chunk are recomputed.
__global__ __launch_bounds__(kIdxWG, 4) void index_refine_kernel(PairArgs a, WorkArgs w) {
    __shared__ IndexShared shu;
    const int c = blockIdx.x, p = blockIdx.y;
    if (w.mo_hist && c == (int)gridDim.x - 1) {  // (multi-workgroup Morton sort: no index_kernel launch)
        index_cloud(shu, a, w, p, false);         // the last column builds the pair's source index
        return;
    }
    if (w.state[p].phase == kPhaseInvalid) return;
    const int m = a.tgt_n[p];
    if (m <= 0 || (m <= kKdMaxN && w.t_stride <= kKdMaxN)) return;  // index_kernel's kd path did it
    const int c0 = c * kKdMaxN;
    if (c0 >= m) return;
    const int len = min(kKdMaxN, m - c0);
    const int tid = threadIdx.x, lane = tid & 63;
    float4* ts = w.tsort + (int64_t)p * w.t_stride + c0;
    kd_order<16>(shu.kd, [&](int i) { return ts[i]; }, len, w.leaf, nullptr);
    const uint16_t* ord = shu.kd.L[0];
    float4 v[kKdPer];  // the chunk in its new order (read before anything is overwritten)
#pragma unroll
    for (int k = 0; k < kKdPer; ++k) {
        const int pos = tid + k * kIdxWG;
        v[k] = pos < len ? ts[ord[pos]] : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
    }
    __syncthreads();
    int32_t* tinv = w.tinv + (int64_t)p * w.t_stride;
    float4* tb = w.tbox + (int64_t)p * 2 * w.b_stride;
    const int B = w.leaf;
    const int nbc = (len + B - 1) / B;  // blocks of the chunk (the last may be partial)
#pragma unroll
    for (int k = 0; k < kKdPer; ++k) {
        const int pos = tid + k * kIdxWG;
        const bool real = pos < len;
        if (real) {
            ts[pos] = v[k];
            tinv[__float_as_uint(v[k].w)] = c0 + pos;
        }
        float4 l = real ? v[k] : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
        float4 h = real ? v[k] : make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        l.x = seg_minf(l.x, B); h.x = seg_maxf(h.x, B);
        l.y = seg_minf(l.y, B); h.y = seg_maxf(h.y, B);
        l.z = seg_minf(l.z, B); h.z = seg_maxf(h.z, B);
        if ((lane & (B - 1)) == 0 && pos / B < nbc) {
            const int b = pos / B;
            l.w = 0.f;
            h.w = 0.f;
            tb[2 * (c0 / B + b)] = l;
            tb[2 * (c0 / B + b) + 1] = h;
            shu.kd.u.bbox[2 * b] = l;
            shu.kd.u.bbox[2 * b + 1] = h;
        }
    }
    __syncthreads();
    float4* sbx = w.sbox + (int64_t)p * 2 * w.sb_stride;
    const int nsbc = (nbc + kSuper - 1) / kSuper, sb0 = c0 / (B * kSuper);
    for (int sb = tid; sb < nsbc; sb += kIdxWG) {
        float4 l = make_float4(INFINITY, INFINITY, INFINITY, 0.f), h = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        for (int b = sb * kSuper; b < min((sb + 1) * kSuper, nbc); ++b) {
            const float4 bl = shu.kd.u.bbox[2 * b], bh = shu.kd.u.bbox[2 * b + 1];
            l.x = fminf(l.x, bl.x); l.y = fminf(l.y, bl.y); l.z = fminf(l.z, bl.z);
            h.x = fmaxf(h.x, bh.x); h.y = fmaxf(h.y, bh.y); h.z = fmaxf(h.z, bh.z);
        }
        sbx[2 * (sb0 + sb)] = l;
        sbx[2 * (sb0 + sb) + 1] = h;
    }
}

hipError_t launch_index(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st) {
    // every source by the target's tree: launch the target builds alone (a grid with idle source
    // workgroups left half the CUs without a build)
    const bool tgt_only = w.src_by_tgt && w.kdn && (w.kd_index & 1) && w.t_stride <= kKdMaxN && w.x_stride <= kKdMaxN;
    const unsigned nch = (unsigned)((w.t_stride + kKdMaxN - 1) / kKdMaxN);
    if (w.mo_hist) {  // (setup_work sets it only for plans that refine: see index_mo_hist_kernel)
        if (!(w.tbb && (w.kd_index & 1) && w.t_stride > kKdMaxN && (w.leaf == 16 || w.leaf == 32) &&
              (int64_t)w.mo_groups * kMoChunk >= w.t_stride))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(index_mo_hist_kernel, dim3(w.mo_groups, npairs), dim3(kIdxWG), 0, st, a, w);
        hipLaunchKernelGGL(index_mo_scatter_kernel, dim3(w.mo_groups, npairs), dim3(kIdxWG), 0, st, a, w);
        // (no src_order_kernel: a target past kKdMaxN has no kd tree for its source to descend)
        hipLaunchKernelGGL(index_refine_kernel, dim3(nch + 1, npairs), dim3(kIdxWG), 0, st, a, w);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(index_kernel, dim3(npairs, tgt_only ? 1 : 2), dim3(kIdxWG), 0, st, a, w);
    if (w.src_by_tgt && w.kdn && !tgt_only)
        hipLaunchKernelGGL(src_order_kernel, dim3(npairs), dim3(kSoWG), 0, st, a, w);
    if ((w.kd_index & 1) && w.t_stride > kKdMaxN && (w.leaf == 16 || w.leaf == 32))
        hipLaunchKernelGGL(index_refine_kernel, dim3(nch, npairs), dim3(kIdxWG), 0, st, a, w);
    return hipGetLastError();
}

hipError_t launch_index_cloud(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st) {
    if (w.mo_hist || (w.src_by_tgt && w.kdn)) return hipErrorInvalidValue;  // (the target chain's forms)
    hipLaunchKernelGGL(index_cloud_kernel, dim3(npairs), dim3(kIdxWG), 0, st, a, w);
    if ((w.kd_index & 1) && w.t_stride > kKdMaxN && (w.leaf == 16 || w.leaf == 32)) {
        const unsigned nch = (unsigned)((w.t_stride + kKdMaxN - 1) / kKdMaxN);
        hipLaunchKernelGGL(index_refine_kernel, dim3(nch, npairs), dim3(kIdxWG), 0, st, a, w);
    }
    return hipGetLastError();
}

}  // namespace icp4r
