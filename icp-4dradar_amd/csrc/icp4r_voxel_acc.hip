// icp4r_voxel_acc.hip — the incremental voxel grid for gfx950: a device-resident list of voxels
// (key, partial sums, count) sorted by absolute cell, which every add merges one scan into and every
// filter divides out (include/icp4r/icp4r_voxel_acc.h states the contract, DESIGN.md §6b.2 why the
// result is the full filter's, bit for bit).
//
// An add, all on one stream, every workgroup independent of every other, no float atomics:
//   the scan's bounding box (launch_finite_bbox) -> one thread applies the range rule, folds the box
//   into the accumulated one and renews the overflow verdict (voxel_grid_from_bbox, the filter's own
//   rule) -> (key, i) per point -> a stable sort by key: a scan of at most kAccSmall points by one
//   workgroup in LDS (acc_small_sort_kernel), a larger one by the store's radix sort, once over a
//   scan-relative key or twice over the 64-bit key's words -> run heads compacted (vx_compact) -> per run a binary search
//   of the state's keys -> the new runs compacted into a sorted key list with their ranks -> the merge
//   kernel streams the old state into the other buffer, each voxel shifted by the number of new keys
//   below it -> the chain kernel continues each run's four sums from the stored ones (or +0.0f) over
//   its members in input order and writes the voxel at its place in the new buffer.
// The chain kernel runs after the merge and writes the new buffer itself, so a voxel that an add
// touches needs no record in between and no two kernels write one element in an unordered way.
#include "icp4r_voxel_common.hpp"

namespace icp4r {

constexpr uint64_t kAccNoKey = ~(uint64_t)0;  // a point that does not take part: sorts last

__global__ void acc_clear_kernel(AccMeta* __restrict__ meta) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    AccMeta m = {};
    for (int k = 0; k < 3; ++k) m.bbox[k] = 0xFFFFFFFFu;  // (+inf, -inf) as launch_finite_bbox leaves it
    m.grid_flag = 1;
    *meta = m;
}

// The range rule and the fold (one thread).  A scan outside the range changes nothing but, for the
// device entry, the sticky flag.
__global__ void acc_prep_kernel(const uint32_t* __restrict__ sbox, VoxelArgs a, int32_t sticky, AccMeta* __restrict__ meta,
                                AccScanInfo* __restrict__ info) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    AccScanInfo r = {};
    if (!(float_unord(sbox[0]) <= float_unord(sbox[3]))) {  // no participating point
        r.skip = 1;
        *info = r;
        return;
    }
    bool bad = false;
    int32_t minc[3] = {0, 0, 0}, maxc[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        const float fl = floorf(float_unord(sbox[k]) * a.inv[k]), fh = floorf(float_unord(sbox[3 + k]) * a.inv[k]);
        if (!(fl >= -2147483648.0f && fh < 2147483648.0f)) {
            bad = true;
        } else {
            minc[k] = (int32_t)fl;
            maxc[k] = (int32_t)fh;
        }
    }
    if (!bad) {
        for (int k = 0; k < 3; ++k) {
            const int64_t org = meta->have_origin ? meta->origin[k] : minc[k];
            if ((int64_t)minc[k] - org < -(int64_t)kAccBias || (int64_t)maxc[k] - org >= (int64_t)kAccBias) bad = true;
        }
    }
    if (bad) {
        r.skip = 2;
        if (sticky) meta->range = 1;
        *info = r;
        return;
    }
    if (!meta->have_origin) {
        for (int k = 0; k < 3; ++k) meta->origin[k] = minc[k];
        meta->have_origin = 1;
    }
    for (int k = 0; k < 3; ++k) {
        meta->bbox[k] = min(meta->bbox[k], sbox[k]);
        meta->bbox[3 + k] = max(meta->bbox[3 + k], sbox[3 + k]);
    }
    meta->grid_flag = voxel_grid_from_bbox(meta->bbox, a).flag;
    for (int k = 0; k < 3; ++k) {
        r.minc[k] = minc[k];
        r.ext[k] = maxc[k] - minc[k] + 1;  // <= 2^21
    }
    const int64_t e01 = (int64_t)r.ext[0] * r.ext[1];
    r.cells = e01 > INT32_MAX ? INT64_MAX : e01 * r.ext[2];
    *info = r;
}

// The 64-bit key of every point and its sort pair.  rel: the pair's key is the scan-relative mixed-radix
// cell number (< info->cells <= INT32_MAX), else the 64-bit key's low word.  ckey (the small-scan sort's):
// the cell's offsets from the scan's own minimum cell, packed like the 64-bit key but each field only as
// wide as the scan's box needs — the same order in fewer bits.  A point that does not take part (and
// every point of a skipped add) gets all ones in each.
__global__ __launch_bounds__(kVxWG) void acc_keys_kernel(const float4* __restrict__ pts, int32_t n, VoxelArgs a,
                                                        const AccMeta* __restrict__ meta,
                                                        const AccScanInfo* __restrict__ info, int32_t rel,
                                                        uint64_t* __restrict__ pkey, int2* __restrict__ pairs,
                                                        uint64_t* __restrict__ ckey) {
    const int64_t i = (int64_t)blockIdx.x * kVxWG + threadIdx.x;
    if (i >= n) return;
    uint64_t key = kAccNoKey, ck = kAccNoKey;
    int32_t x = -1;
    const float4 p = pts[i];
    if (info->skip == 0 && finite_xyz(p)) {
        const int32_t c0 = (int32_t)floorf(p.x * a.inv[0]), c1 = (int32_t)floorf(p.y * a.inv[1]),
                      c2 = (int32_t)floorf(p.z * a.inv[2]);
        const uint64_t o0 = (uint64_t)((int64_t)c0 - meta->origin[0] + kAccBias), o1 = (uint64_t)((int64_t)c1 - meta->origin[1] + kAccBias),
                       o2 = (uint64_t)((int64_t)c2 - meta->origin[2] + kAccBias);
        key = (o2 << (2 * kAccAxisBits)) | (o1 << kAccAxisBits) | o0;
        if (rel)
            x = (int32_t)((int64_t)(c0 - info->minc[0]) + (int64_t)(c1 - info->minc[1]) * info->ext[0] +
                          (int64_t)(c2 - info->minc[2]) * ((int64_t)info->ext[0] * info->ext[1]));
        else
            x = (int32_t)(uint32_t)key;
        if (ckey) {  // each field as wide as the scan's own box needs (at most 21 bits)
            const int s0 = info->ext[0] > 1 ? 32 - __builtin_clz((uint32_t)(info->ext[0] - 1)) : 0,
                      s1 = info->ext[1] > 1 ? 32 - __builtin_clz((uint32_t)(info->ext[1] - 1)) : 0;
            ck = (uint64_t)(uint32_t)(c0 - info->minc[0]) | ((uint64_t)(uint32_t)(c1 - info->minc[1]) << s0) |
                 ((uint64_t)(uint32_t)(c2 - info->minc[2]) << (s0 + s1));
        }
    }
    pkey[i] = key;
    if (pairs) pairs[i] = make_int2(x, (int32_t)i);
    if (ckey) ckey[i] = ck;
}

// Between the two sorts: the pairs, in the low word's order, re-keyed by the high word.
__global__ __launch_bounds__(kVxWG) void acc_rekey_kernel(const int2* __restrict__ sorted, int32_t n,
                                                         const uint64_t* __restrict__ pkey, int2* __restrict__ pairs) {
    const int64_t t = (int64_t)blockIdx.x * kVxWG + threadIdx.x;
    if (t >= n) return;
    const int32_t i = sorted[t].y;
    pairs[t] = make_int2((int32_t)(uint32_t)(pkey[i] >> 32), i);
}

// The 64-bit keys in sorted order.
__global__ __launch_bounds__(kVxWG) void acc_skey_kernel(const int2* __restrict__ sorted, int32_t n,
                                                        const uint64_t* __restrict__ pkey, uint64_t* __restrict__ skey) {
    const int64_t t = (int64_t)blockIdx.x * kVxWG + threadIdx.x;
    if (t >= n) return;
    skey[t] = pkey[sorted[t].y];
}

// A scan of at most kAccSmall points is sorted by one workgroup in LDS, in one launch: at 6,554 points
// every launch of the global sort is latency, and this kernel chooses its passes on the device, which
// the device entry's host side cannot.  The participating points' indices are compacted in input order
// (the others go to the tail), then stable LSD passes of 8 key bits — ranked by ballots, as
// ds_radix_scatter_kernel ranks — reorder the 16-bit indices in LDS; a pass starts at the lowest key bit that still
// differs between two participating keys, so bytes that no key pair differs in cost nothing; the passes
// read the compact key (ckey: a 160 m scan at leaf 0.5 has about 23 bits, three passes), whose order is
// the 64-bit key's.  Out: the pairs' .y and the sorted 64-bit keys.
constexpr int kAccSortWG = 1024;
constexpr int kAccSortPer = kAccSmall / kAccSortWG;

__device__ __forceinline__ uint64_t acc_shfl_xor64(uint64_t v, int off) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kAccSortWG) void acc_small_sort_kernel(const uint64_t* __restrict__ pkey,
                                                                   const uint64_t* __restrict__ ckey, int32_t n,
                                                                   int2* __restrict__ sorted, uint64_t* __restrict__ skey) {
    constexpr int kWaves = kAccSortWG / 64;
    static_assert(kAccSmall <= 65536 && kAccSortWG >= 256 && kAccSortWG * 4 == kWaves * 256, "16-bit indices; the zeroing below");
    __shared__ uint16_t ord[2][kAccSmall];
    __shared__ int32_t cnt[256 * kWaves];  // per (digit, wave), digit-major: the count, then the next output position
    __shared__ int32_t wtot[2][kWaves];
    __shared__ uint64_t wmask[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    // the participating points to ord[0], the others to ord[1], both in input order
    int32_t m = 0, rest = 0;
    for (int k = 0; k < kAccSortPer; ++k) {
        const int32_t i = k * kAccSortWG + tid;
        const bool in = i < n;
        const bool part = in && pkey[i] != kAccNoKey, none = in && !part;
        const uint64_t mp = __ballot(part), mn = __ballot(none);
        if (lane == 0) {
            wtot[0][wave] = __builtin_popcountll(mp);
            wtot[1][wave] = __builtin_popcountll(mn);
        }
        __syncthreads();
        int32_t bp = 0, tp = 0, bn = 0, tn = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            bp += w < wave ? wtot[0][w] : 0;
            tp += wtot[0][w];
            bn += w < wave ? wtot[1][w] : 0;
            tn += wtot[1][w];
        }
        if (part) ord[0][m + bp + __builtin_popcountll(mp & below)] = (uint16_t)i;
        if (none) ord[1][rest + bn + __builtin_popcountll(mn & below)] = (uint16_t)i;
        m += tp;
        rest += tn;
        __syncthreads();
    }
    for (int32_t j = tid; j < rest; j += kAccSortWG) {
        sorted[m + j] = make_int2(-1, (int32_t)ord[1][j]);
        skey[m + j] = kAccNoKey;
    }
    // the key bits in which two participating keys differ
    uint64_t vary = 0;
    if (m > 0) {
        const uint64_t key0 = ckey[ord[0][0]];
        for (int k = 0; k < kAccSortPer; ++k) {
            const int32_t pos = k * kAccSortWG + tid;
            if (pos < m) vary |= ckey[ord[0][pos]] ^ key0;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vary |= acc_shfl_xor64(vary, off);
    if (lane == 0) wmask[wave] = vary;
    __syncthreads();  // (also: ord[1] has been read)
    vary = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) vary |= wmask[w];
    // Each wave owns a contiguous chunk of the list.  A pass: the waves count their chunks' digits; one
    // scan of the 256 x kWaves counts, digit-major, gives every (digit, wave) its first output position;
    // each wave then places its chunk 64 elements at a time in order, the lanes of one digit ranked by
    // lane, the digit's lowest lane moving the wave's position on.  Chunks, rounds and lanes ascend with
    // the list position, so the pass is stable.
    const int32_t per = (m + kWaves - 1) / kWaves;  // <= 64 * kAccSortPer
    const int32_t lo = wave * per, hi = lo + per < m ? lo + per : m;
    int cur = 0;
    while (vary) {  // (the same in every thread)
        const int shift = __builtin_ctzll(vary);
        vary &= ~((uint64_t)0xFF << shift);
        const uint16_t* src = ord[cur];
        uint16_t* dst = ord[cur ^ 1];
        uint16_t id[kAccSortPer];
        int32_t dg[kAccSortPer];
#pragma unroll
        for (int k = 0; k < kAccSortPer; ++k) {
            const int32_t pos = lo + k * 64 + lane;
            id[k] = pos < hi ? src[pos] : (uint16_t)0;
            dg[k] = pos < hi ? (int32_t)((ckey[id[k]] >> shift) & 255) : 0;
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) cnt[w * kAccSortWG + tid] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kAccSortPer; ++k)
            if (lo + k * 64 + lane < hi) atomicAdd(&cnt[dg[k] * kWaves + wave], 1);
        __syncthreads();
        {  // the exclusive scan of cnt[256 * kWaves]: four entries per thread
            const int32_t c0 = cnt[4 * tid], c1 = cnt[4 * tid + 1], c2 = cnt[4 * tid + 2], c3 = cnt[4 * tid + 3];
            const int32_t sum = c0 + c1 + c2 + c3;
            int32_t incl = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int32_t up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            if (lane == 63) wtot[0][wave] = incl;
            __syncthreads();
            int32_t ex = incl - sum;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) ex += w < wave ? wtot[0][w] : 0;
            cnt[4 * tid] = ex;
            cnt[4 * tid + 1] = ex + c0;
            cnt[4 * tid + 2] = ex + c0 + c1;
            cnt[4 * tid + 3] = ex + c0 + c1 + c2;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kAccSortPer; ++k) {
            if (lo + k * 64 >= hi) break;  // (the whole wave)
            const bool valid = lo + k * 64 + lane < hi;
            const int d = dg[k];
            uint64_t same = __ballot(valid);  // the wave's valid lanes with this lane's digit
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1;
                const uint64_t bm = __ballot(bit);
                same &= bit ? bm : ~bm;
            }
            const int rank = __builtin_popcountll(same & below);
            int32_t at = 0;
            if (valid) at = cnt[d * kWaves + wave];
            __builtin_amdgcn_wave_barrier();  // every lane of the digit has read the position before it moves
            if (valid) {
                dst[at + rank] = id[k];
                if (rank == 0) cnt[d * kWaves + wave] = at + __builtin_popcountll(same);
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int k = 0; k < kAccSortPer; ++k) {
        const int32_t pos = k * kAccSortWG + tid;
        if (pos < m) {
            const int32_t i = ord[cur][pos];
            sorted[pos] = make_int2(0, i);
            skey[pos] = pkey[i];
        }
    }
}

struct AccHeadPred {  // the sorted positions where a run of equal keys starts (the kAccNoKey run included)
    const uint64_t* skey;
    int32_t n;
    int32_t* heads;
    __device__ __forceinline__ int32_t size() const { return n; }
    __device__ __forceinline__ bool keep(int64_t t) const { return t == 0 || skey[t - 1] != skey[t]; }
    __device__ __forceinline__ void emit(int64_t t, int32_t rank) const { heads[rank] = (int32_t)t; }
};

// The runs that are voxels: all but a last run of kAccNoKey.
__device__ __forceinline__ int32_t acc_real_runs(const uint64_t* __restrict__ skey, const int32_t* __restrict__ heads,
                                                 int32_t nruns) {
    return nruns - (skey[heads[nruns - 1]] == kAccNoKey ? 1 : 0);
}

__device__ __forceinline__ int32_t acc_lower_bound(const uint64_t* __restrict__ keys, int32_t n, uint64_t k) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Per run: its lower bound among the state's keys, bit 31 set when the key is there.
__global__ __launch_bounds__(kVxWG) void acc_search_kernel(const uint64_t* __restrict__ skey, const int32_t* __restrict__ heads,
                                                          const int32_t* __restrict__ nruns,
                                                          const AccMeta* __restrict__ meta,
                                                          const uint64_t* __restrict__ keys, uint32_t* __restrict__ posf) {
    const int64_t r = (int64_t)blockIdx.x * kVxWG + threadIdx.x;
    if (r >= acc_real_runs(skey, heads, *nruns)) return;
    const uint64_t k = skey[heads[r]];
    const int32_t nv = meta->nvox;
    const int32_t pos = acc_lower_bound(keys, nv, k);
    const bool found = pos < nv && keys[pos] == k;
    posf[r] = (uint32_t)pos | (found ? 0x80000000u : 0u);
}

struct AccNewPred {  // the runs whose cell the state does not hold: their keys in order, their ranks
    const uint64_t* skey;
    const int32_t* heads;
    const int32_t* nruns;
    const uint32_t* posf;
    int32_t* newrank;
    uint64_t* newkeys;
    __device__ __forceinline__ int32_t size() const { return acc_real_runs(skey, heads, *nruns); }
    __device__ __forceinline__ bool keep(int64_t r) const { return (posf[r] & 0x80000000u) == 0; }
    __device__ __forceinline__ void emit(int64_t r, int32_t rank) const {
        newrank[r] = rank;
        newkeys[rank] = skey[heads[r]];
    }
};

// The old state into the other buffer: voxel i moves to i + (new keys below its key).  A workgroup
// searches its first and last key in the new-key list (at most the scan's runs: L2-resident) and
// copies with that one shift when the two agree, else it searches per element.  A thread takes two
// neighbouring voxels at a time: 16-byte loads of keys and sums, 16-byte key stores where the
// destination pair is aligned.
__global__ __launch_bounds__(kVxWG) void acc_merge_kernel(const AccMeta* __restrict__ meta, AccState cur, AccState next,
                                                         const uint64_t* __restrict__ newkeys,
                                                         const int32_t* __restrict__ nnew_p) {
    const int64_t n = meta->nvox;
    const int64_t base = (int64_t)blockIdx.x * kAccMergeBlock;
    if (base >= n) return;  // (the whole workgroup)
    const int32_t nnew = *nnew_p;
    const int64_t last = (base + kAccMergeBlock < n ? base + kAccMergeBlock : n) - 1;
    const int32_t s0 = acc_lower_bound(newkeys, nnew, cur.key[base]);
    const bool uniform = s0 == acc_lower_bound(newkeys, nnew, cur.key[last]);
    for (int k = 0; k < kAccMergeBlock / (2 * kVxWG); ++k) {
        const int64_t i = base + 2 * (int64_t)(k * kVxWG + threadIdx.x);
        if (i + 1 <= last) {
            const ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(cur.key + i);
            const float4 sa = cur.sums[i], sb = cur.sums[i + 1];
            const uint2 cc = *reinterpret_cast<const uint2*>(cur.count + i);
            int32_t ha = s0, hb = s0;
            if (!uniform) {
                ha = acc_lower_bound(newkeys, nnew, kk.x);
                hb = acc_lower_bound(newkeys, nnew, kk.y);
            }
            const int64_t da = i + ha, db = i + 1 + hb;
            if (ha == hb && (da & 1) == 0) {
                *reinterpret_cast<ulonglong2*>(next.key + da) = kk;
                *reinterpret_cast<uint2*>(next.count + da) = cc;
            } else {
                next.key[da] = kk.x;
                next.key[db] = kk.y;
                next.count[da] = cc.x;
                next.count[db] = cc.y;
            }
            next.sums[da] = sa;
            next.sums[db] = sb;
        } else if (i <= last) {
            const uint64_t ka = cur.key[i];
            const int64_t da = i + (uniform ? s0 : acc_lower_bound(newkeys, nnew, ka));
            next.key[da] = ka;
            next.sums[da] = cur.sums[i];
            next.count[da] = cur.count[i];
        }
    }
}

// Chains: a lane per run.  A run starts from the stored sums when the state holds its cell, else from
// +0.0f — never from its first member, whose -0.0f would survive — and adds its members in input order
// in voxel_centroid_kernel's two forms: a lane walks a run of at most kVxShort members, the whole wave
// takes a longer one, 64 members per gather, added lane after lane.  The voxel goes to its place in
// the new buffer: an old one to its position plus the new keys below it, a new one to its lower bound
// plus its own rank.  Thread 0 also commits the new voxel count (nothing else reads it here).
__global__ __launch_bounds__(kVxWG) void acc_chain_kernel(const float4* __restrict__ pts, const int2* __restrict__ sorted,
                                                         int32_t n, const uint64_t* __restrict__ skey,
                                                         const int32_t* __restrict__ heads,
                                                         const int32_t* __restrict__ nruns_p,
                                                         const uint32_t* __restrict__ posf,
                                                         const int32_t* __restrict__ newrank,
                                                         const uint64_t* __restrict__ newkeys,
                                                         const int32_t* __restrict__ nnew_p, AccState cur, AccState next,
                                                         AccMeta* __restrict__ meta) {
    const int32_t nruns = *nruns_p;
    const int32_t R = acc_real_runs(skey, heads, nruns);
    const int32_t nnew = *nnew_p;
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * kVxWG + threadIdx.x;
    if (v == 0) meta->nvox += nnew;
    if (v - lane >= R) return;  // (the whole wave)
    const bool have = v < R;
    int32_t start = 0, m = 0;
    uint32_t pf = 0, cnt0 = 0;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
    if (have) {
        start = heads[v];
        m = (v + 1 < nruns ? heads[v + 1] : n) - start;
        pf = posf[v];
        if (pf & 0x80000000u) {
            const float4 s = cur.sums[pf & 0x7fffffffu];
            sx = s.x, sy = s.y, sz = s.z, sw = s.w;
            cnt0 = cur.count[pf & 0x7fffffffu];
        }
    }
    if (have && m <= kVxShort) {
        for (int32_t u = 0; u < m; u += 4) {
            float4 p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = pts[sorted[start + min(u + j, m - 1)].y];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (u + j < m) {
                    sx += p[j].x;
                    sy += p[j].y;
                    sz += p[j].z;
                    sw += p[j].w;
                }
        }
    }
    uint64_t todo = __ballot(have && m > kVxShort);
    while (todo) {
        const int owner = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int32_t st = __builtin_amdgcn_readlane(start, owner), mm = __builtin_amdgcn_readlane(m, owner);
        float cx = vx_lane(sx, owner), cy = vx_lane(sy, owner), cz = vx_lane(sz, owner), cw = vx_lane(sw, owner);
        float4 next_p = make_float4(0.f, 0.f, 0.f, 0.f);  // (lanes past the run's end: never read)
        if (lane < mm) next_p = pts[sorted[st + lane].y];
        for (int64_t c = 0; c < mm; c += 64) {
            const float4 cur_p = next_p;
            if (c + 64 + lane < mm) next_p = pts[sorted[st + c + 64 + lane].y];
            const int cnt = (int)(mm - c < 64 ? mm - c : 64);
            for (int j = 0; j < cnt; ++j) {
                cx += vx_lane(cur_p.x, j);
                cy += vx_lane(cur_p.y, j);
                cz += vx_lane(cur_p.z, j);
                cw += vx_lane(cur_p.w, j);
            }
        }
        if (lane == owner) sx = cx, sy = cy, sz = cz, sw = cw;
    }
    if (have) {
        const uint64_t key = skey[start];
        const int64_t pos = pf & 0x7fffffffu;
        const int64_t dst = pos + ((pf & 0x80000000u) ? acc_lower_bound(newkeys, nnew, key) : newrank[v]);
        next.key[dst] = key;
        next.sums[dst] = make_float4(sx, sy, sz, sw);
        next.count[dst] = cnt0 + (uint32_t)m;
    }
}

// -1: grid overflow (it comes first); -2: the range flag; 0: the state may be read.
__device__ __forceinline__ int32_t acc_verdict(const AccMeta* __restrict__ meta) {
    return meta->grid_flag < 0 ? -1 : (meta->range ? -2 : 0);
}

__device__ __forceinline__ float4 acc_centroid(const AccState& s, int64_t i, int32_t all_data) {
    const float4 t = s.sums[i];
    const float fm = (float)s.count[i];
    float w = 0.0f;
    if (all_data) w = __fdiv_rn(t.w, fm);
    return make_float4(__fdiv_rn(t.x, fm), __fdiv_rn(t.y, fm), __fdiv_rn(t.z, fm), w);
}

// Every voxel is an output point: one stream over the state.
__global__ __launch_bounds__(kVxWG) void acc_filter_kernel(const AccMeta* __restrict__ meta, AccState cur, int32_t all_data,
                                                          float4* __restrict__ out, int32_t* __restrict__ count) {
    const int64_t v = (int64_t)blockIdx.x * kVxWG + threadIdx.x;
    const int32_t bad = acc_verdict(meta), n = meta->nvox;
    if (v == 0) *count = bad ? bad : n;
    if (bad || v >= n) return;
    out[v] = acc_centroid(cur, v, all_data);
}

struct AccKeepPred {  // the voxels with enough members; rank = the output position
    const AccMeta* meta;
    AccState cur;
    uint32_t min_pts;
    int32_t all_data;
    float4* out;
    __device__ __forceinline__ int32_t size() const { return acc_verdict(meta) ? 0 : meta->nvox; }
    __device__ __forceinline__ bool keep(int64_t i) const { return cur.count[i] >= min_pts; }
    __device__ __forceinline__ void emit(int64_t i, int32_t rank) const { out[rank] = acc_centroid(cur, i, all_data); }
};

__global__ void acc_count_kernel(const AccMeta* __restrict__ meta, const int32_t* __restrict__ total, int32_t* __restrict__ count) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int32_t bad = acc_verdict(meta);
    *count = bad ? bad : *total;
}

static size_t acc_align(size_t x) { return (x + 255) & ~(size_t)255; }

AccLayout acc_layout(int64_t n) {
    AccLayout L;
    const size_t m = (size_t)(n > 0 ? n : 1);
    const size_t nblk = 256 * (size_t)sector_blocks((int64_t)m);  // the radix sort's counts; the compactions need fewer
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += acc_align(bytes);
        return at;
    };
    L.bbox = take(6 * sizeof(uint32_t));
    L.info = take(sizeof(AccScanInfo));
    L.tot = take(4 * sizeof(int32_t));  // runs, new runs, the radix scans' total
    L.pkey = take(m * sizeof(uint64_t));
    L.pa = take(m * sizeof(int2));
    L.pb = take(m * sizeof(int2));
    L.counts = take(nblk * sizeof(int32_t));
    L.offsets = take(nblk * sizeof(int32_t));
    L.skey = take(m * sizeof(uint64_t));
    L.heads = take(m * sizeof(int32_t));
    L.posf = take(m * sizeof(uint32_t));
    L.newrank = take(m * sizeof(int32_t));
    L.newkeys = take(m * sizeof(uint64_t));
    L.bytes = o;
    return L;
}

hipError_t launch_acc_clear(AccMeta* meta, hipStream_t st) {
    hipLaunchKernelGGL(acc_clear_kernel, dim3(1), dim3(64), 0, st, meta);
    return hipGetLastError();
}

hipError_t launch_acc_prep(const float4* pts, int64_t n, const VoxelArgs& a, AccMeta* meta, void* work, int sticky,
                           hipStream_t st) {
    const AccLayout L = acc_layout(n);
    char* w = static_cast<char*>(work);
    uint32_t* sbox = reinterpret_cast<uint32_t*>(w + L.bbox);
    hipError_t e;
    if ((e = launch_finite_bbox(pts, n, sbox, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(acc_prep_kernel, dim3(1), dim3(64), 0, st, sbox, a, (int32_t)sticky, meta,
                       reinterpret_cast<AccScanInfo*>(w + L.info));
    return hipGetLastError();
}

hipError_t launch_acc_merge(const float4* pts, int64_t n, const VoxelArgs& a, int sort_bits, AccMeta* meta, const AccState& cur,
                            const AccState& next, int64_t max_vox, void* work, hipStream_t st) {
    const AccLayout L = acc_layout(n);
    char* w = static_cast<char*>(work);
    const AccScanInfo* info = reinterpret_cast<const AccScanInfo*>(w + L.info);
    int32_t* tot = reinterpret_cast<int32_t*>(w + L.tot);
    uint64_t* pkey = reinterpret_cast<uint64_t*>(w + L.pkey);
    int2 *pa = reinterpret_cast<int2*>(w + L.pa), *pb = reinterpret_cast<int2*>(w + L.pb);
    int32_t* counts = reinterpret_cast<int32_t*>(w + L.counts);
    int32_t* offsets = reinterpret_cast<int32_t*>(w + L.offsets);
    uint64_t* skey = reinterpret_cast<uint64_t*>(w + L.skey);
    int32_t* heads = reinterpret_cast<int32_t*>(w + L.heads);
    uint32_t* posf = reinterpret_cast<uint32_t*>(w + L.posf);
    int32_t* newrank = reinterpret_cast<int32_t*>(w + L.newrank);
    uint64_t* newkeys = reinterpret_cast<uint64_t*>(w + L.newkeys);
    const int32_t n32 = (int32_t)n;
    const dim3 per_point((unsigned)((n + kVxWG - 1) / kVxWG)), wg(kVxWG);
    int2* sorted;
    if (n <= kAccSmall) {
        uint64_t* ckey = reinterpret_cast<uint64_t*>(pa);  // (n x 8 bytes, as the pairs)
        hipLaunchKernelGGL(acc_keys_kernel, per_point, wg, 0, st, pts, n32, a, meta, info, 0, pkey, static_cast<int2*>(nullptr),
                           ckey);
        sorted = pb;
        hipLaunchKernelGGL(acc_small_sort_kernel, dim3(1), dim3(kAccSortWG), 0, st, pkey, ckey, n32, sorted, skey);
    } else {
        hipLaunchKernelGGL(acc_keys_kernel, per_point, wg, 0, st, pts, n32, a, meta, info, (int32_t)(sort_bits > 0), pkey, pa,
                           static_cast<uint64_t*>(nullptr));
        if (sort_bits > 0) {
            sorted = launch_radix_sort(pa, pb, n32, sort_bits, counts, offsets, tot + 2, st);
        } else {
            int2* lo = launch_radix_sort(pa, pb, n32, 32, counts, offsets, tot + 2, st);
            int2* other = lo == pa ? pb : pa;
            hipLaunchKernelGGL(acc_rekey_kernel, per_point, wg, 0, st, lo, n32, pkey, other);
            sorted = launch_radix_sort(other, lo, n32, 32, counts, offsets, tot + 2, st);
        }
        hipLaunchKernelGGL(acc_skey_kernel, per_point, wg, 0, st, sorted, n32, pkey, skey);
    }
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = vx_compact(AccHeadPred{skey, n32, heads}, n, counts, offsets, tot, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(acc_search_kernel, per_point, wg, 0, st, skey, heads, tot, meta, cur.key, posf);
    if ((e = vx_compact(AccNewPred{skey, heads, tot, posf, newrank, newkeys}, n, counts, offsets, tot + 1, st)) != hipSuccess)
        return e;
    const int64_t mblk = (max_vox + kAccMergeBlock - 1) / kAccMergeBlock;
    if (mblk > 0) hipLaunchKernelGGL(acc_merge_kernel, dim3((unsigned)mblk), wg, 0, st, meta, cur, next, newkeys, tot + 1);
    hipLaunchKernelGGL(acc_chain_kernel, per_point, wg, 0, st, pts, sorted, n32, skey, heads, tot, posf, newrank, newkeys,
                       tot + 1, cur, next, meta);
    return hipGetLastError();
}

size_t acc_filter_scan_bytes(int64_t max_vox) {
    return (2 * (size_t)vx_blocks(max_vox > 0 ? max_vox : 1) + 1) * sizeof(int32_t);
}

hipError_t launch_acc_filter(const AccMeta* meta, const AccState& cur, int64_t max_vox, const VoxelArgs& a, int32_t* scan,
                             float4* out, int32_t* count, hipStream_t st) {
    if (a.min_pts <= 1) {
        const int64_t nblk = max_vox > 0 ? (max_vox + kVxWG - 1) / kVxWG : 1;
        hipLaunchKernelGGL(acc_filter_kernel, dim3((unsigned)nblk), dim3(kVxWG), 0, st, meta, cur, a.all_data, out, count);
        return hipGetLastError();
    }
    const int64_t nblk = vx_blocks(max_vox > 0 ? max_vox : 1);
    int32_t *counts = scan, *offsets = scan + nblk, *total = scan + 2 * nblk;
    hipError_t e;
    if ((e = vx_compact(AccKeepPred{meta, cur, a.min_pts, a.all_data, out}, max_vox > 0 ? max_vox : 1, counts, offsets, total,
                        st)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(acc_count_kernel, dim3(1), dim3(64), 0, st, meta, total, count);
    return hipGetLastError();
}

}  // namespace icp4r
