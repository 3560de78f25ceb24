// icp4r_map.hip — scan-to-map store kernels for gfx950 (include/icp4r/icp4r_map.h).
//
// The reference keeps its radar map in an ikd-Tree and, per scan, takes the submap with
// Sector_Search — a full traversal with a per-point keep test (ikd_Tree.cpp:1098-1140).  Here the
// map is a dense float4 array in HBM, in insertion order, and the query is a stable stream compaction
// at HBM bandwidth: count per 4096-point block -> exclusive scan of the block counts -> ordered write.
// Both passes read the map once (16 B/point) and the write pass stores the kept points (16 B each).
// Box_Search, Radius_Search and Delete_Point_Boxes are the same compaction with another keep test
// (the delete keeps what lies outside the boxes and the host swaps buffers); the downsampling
// Add_Points is a per-cell reduction over a hash table followed by one such compaction.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icp4r_device.hpp"
#include "icp4r_internal.hpp"

namespace icp4r {

constexpr int kSecWG = 256;
constexpr int kSecPer = 16;                  // points per thread
constexpr int kSecBlock = kSecWG * kSecPer;  // points per workgroup
constexpr double kPi = 3.14159265358979323846;  // glibc's M_PI (math.h), the reference's constant

// KD_TREE::calc_heading (ikd_Tree.cpp:1434-1448): float asinf / sqrtf (ikd_Tree.h's `using namespace
// std` picks the float overloads), `* 180` in float, `/ M_PI` and `180 +` in double, stored as float.
__device__ __forceinline__ float map_calc_heading(float ax, float ay, float az, float bx, float by, float bz) {
    const float r = (ax - bx) / sqrtf(map_calc_dist(ax, ay, az, bx, by, bz));
    float h;
    if (ay - by < 0.0f)
        h = (float)(180.0 + (double)(asinf(r) * 180.0f) / kPi);
    else
        h = (float)((double)(-asinf(r) * 180.0f) / kPi);
    if (h > 180.0f && h < 360.0f) h = h - 360.0f;
    return h;
}

// Search_by_sector's keep test (ikd_Tree.cpp:1114-1116), precedence included; nothing is deleted.
__device__ __forceinline__ bool sector_keep(const float4 p, const SectorArgs& a) {
    const float dh = fabsf(map_calc_heading(p.x, p.y, p.z, a.cx, a.cy, a.cz) - a.heading);
    return (map_calc_dist(p.x, p.y, p.z, a.cx, a.cy, a.cz) <= a.radius * a.radius && dh < 60.0f) || (dh > 300.0f);
}

// pointAssociateToMap (radar_odometry.cpp:137-145): p_w = Rtrans * p + t_w_curr in double, per row
// ((R0*x + R1*y) + R2*z) + t (Eigen's packet order), cast to float; intensity copied.
__global__ __launch_bounds__(256) void associate_kernel(const float4* __restrict__ in, int64_t n, Mat3x4d M,
                                                        float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 v = in[i];
    const double x = v.x, y = v.y, z = v.z;
    double w[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double s = M.R[3 * r] * x;
        s = s + M.R[3 * r + 1] * y;
        s = s + M.R[3 * r + 2] * z;
        w[r] = s + M.t[r];
    }
    out[i] = make_float4((float)w[0], (float)w[1], (float)w[2], v.w);
}

// ---- compaction predicates: load(i) is element i of the filtered sequence, keep(i, p) its test.
struct SectorPred {
    const float4* map;
    SectorArgs a;
    __device__ __forceinline__ float4 load(int64_t i) const { return map[i]; }
    __device__ __forceinline__ bool keep(int64_t, const float4 p) const { return sector_keep(p, a); }
};

// ikd-Tree's box membership (ikd_Tree.cpp:678, :786, :1034): half-open, min <= p && max > p per axis
// (a NaN coordinate or bound fails it).
__device__ __forceinline__ bool map_in_box(const float4 p, const float* lo, const float* hi) {
    return lo[0] <= p.x && hi[0] > p.x && lo[1] <= p.y && hi[1] > p.y && lo[2] <= p.z && hi[2] > p.z;
}

struct BoxPred {  // Box_Search
    const float4* map;
    BoxArgs b;
    __device__ __forceinline__ float4 load(int64_t i) const { return map[i]; }
    __device__ __forceinline__ bool keep(int64_t, const float4 p) const { return map_in_box(p, b.lo, b.hi); }
};

struct RadiusPred {  // Radius_Search: calc_dist(p, c) <= fl(r * r)
    const float4* map;
    float cx, cy, cz, r2;
    __device__ __forceinline__ float4 load(int64_t i) const { return map[i]; }
    __device__ __forceinline__ bool keep(int64_t, const float4 p) const {
        return map_calc_dist(p.x, p.y, p.z, cx, cy, cz) <= r2;
    }
};

struct OutsideBoxesPred {  // Delete_Point_Boxes: the survivors lie in none of the nb boxes
    const float4* map;
    const float* boxes;  // device, nb x 6 (min xyz, max xyz); wave-uniform reads
    int32_t nb;
    __device__ __forceinline__ float4 load(int64_t i) const { return map[i]; }
    __device__ __forceinline__ bool keep(int64_t, const float4 p) const {
        for (int32_t b = 0; b < nb; ++b)
            if (map_in_box(p, boxes + 6 * (int64_t)b, boxes + 6 * (int64_t)b + 3)) return false;
        return true;
    }
};

struct DsPred {  // downsampled insert: the stored points [0, n0), then the arrivals
    const float4* map;
    const float4* arr;
    int64_t n0;
    const int32_t* sslot;  // [n0] the touched cell's slot of a stored member, -1: not a member of one
    const int32_t* swin;   // [slots] the stored point a touched cell keeps, -1: an arrival took it
    const int32_t* akeep;  // [na] 1: the arrival stays
    __device__ __forceinline__ float4 load(int64_t i) const { return i < n0 ? map[i] : arr[i - n0]; }
    __device__ __forceinline__ bool keep(int64_t i, const float4) const {
        if (i >= n0) return akeep[i - n0] != 0;
        const int32_t s = sslot[i];
        return s < 0 || swin[s] == (int32_t)i;
    }
};

template <class Pred>
__global__ __launch_bounds__(kSecWG) void compact_count_kernel(Pred pr, int64_t n, int32_t* __restrict__ counts) {
    __shared__ int32_t wsum[kSecWG / 64];
    const int64_t base = (int64_t)blockIdx.x * kSecBlock;
    int c = 0;
#pragma unroll 4
    for (int k = 0; k < kSecPer; ++k) {
        const int64_t i = base + k * kSecWG + threadIdx.x;
        if (i < n && pr.keep(i, pr.load(i))) ++c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kSecWG / 64; ++w) t += wsum[w];
        counts[blockIdx.x] = t;
    }
}

// Exclusive scan of the block counts by one workgroup (tiles of 1024); total -> *total.
__global__ __launch_bounds__(1024) void sector_scan_kernel(const int32_t* __restrict__ counts, int nblk,
                                                           int32_t* __restrict__ offsets, int32_t* __restrict__ total) {
    __shared__ int32_t wsum[16];
    __shared__ int32_t carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblk; b0 += 1024) {
        const int i = b0 + tid;
        const int v = i < nblk ? counts[i] : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int wbase = 0;
        for (int w = 0; w < wave; ++w) wbase += wsum[w];
        const int c0 = carry;
        if (i < nblk) offsets[i] = c0 + wbase + incl - v;
        __syncthreads();
        if (tid == 1023) carry = c0 + wbase + incl;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// The same exclusive scan for long inputs (the radix sort's 256 counts per block: 410 k entries at
// 6.5 M pairs, where tiles of 1024 cost 400 rounds of three barriers): a thread takes 8 consecutive
// entries per round, so a round covers 8192.
constexpr int kScanPer = 8;  // (the 16-byte accesses below spell out 8)
__global__ __launch_bounds__(1024) void wide_scan_kernel(const int32_t* __restrict__ counts, int nblk,
                                                         int32_t* __restrict__ offsets, int32_t* __restrict__ total) {
    __shared__ int32_t wsum[16];
    __shared__ int32_t carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    const bool vec = ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(offsets)) & 15) == 0;
    for (int b0 = 0; b0 < nblk; b0 += 1024 * kScanPer) {
        const int i0 = b0 + tid * kScanPer;
        const bool whole = vec && i0 + kScanPer <= nblk;  // two 16-byte accesses instead of eight of 4
        int v[kScanPer], t = 0;
        if (whole) {
            const int4 a = reinterpret_cast<const int4*>(counts + i0)[0], b = reinterpret_cast<const int4*>(counts + i0)[1];
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < kScanPer; ++e) v[e] = i0 + e < nblk ? counts[i0 + e] : 0;
        }
#pragma unroll
        for (int e = 0; e < kScanPer; ++e) t += v[e];
        int incl = t;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int wbase = 0;
        for (int w = 0; w < wave; ++w) wbase += wsum[w];
        const int c0 = carry;
        int run = c0 + wbase + incl - t;
        int x[kScanPer];
#pragma unroll
        for (int e = 0; e < kScanPer; ++e) {
            x[e] = run;
            run += v[e];
        }
        if (whole) {
            reinterpret_cast<int4*>(offsets + i0)[0] = make_int4(x[0], x[1], x[2], x[3]);
            reinterpret_cast<int4*>(offsets + i0)[1] = make_int4(x[4], x[5], x[6], x[7]);
        } else {
#pragma unroll
            for (int e = 0; e < kScanPer; ++e)
                if (i0 + e < nblk) offsets[i0 + e] = x[e];
        }
        __syncthreads();
        if (tid == 1023) carry = c0 + wbase + incl;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// Ordered write: within a block, round k covers 256 consecutive points, wave w its 64, lane its one
// — so ranks taken round by round, wave by wave, lane by lane are insertion order.
template <class Pred>
__global__ __launch_bounds__(kSecWG) void compact_write_kernel(Pred pr, int64_t n, const int32_t* __restrict__ offsets,
                                                               float4* __restrict__ out) {
    __shared__ int32_t wcnt[kSecWG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * kSecBlock;
    int32_t run = offsets[blockIdx.x];
    for (int k = 0; k < kSecPer; ++k) {
        const int64_t i = base + k * kSecWG + tid;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        bool keep = false;
        if (i < n) {
            p = pr.load(i);
            keep = pr.keep(i, p);
        }
        const uint64_t m = __ballot(keep);
        if (lane == 0) wcnt[wave] = __builtin_popcountll(m);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kSecWG / 64; ++w) {
            before += w < wave ? wcnt[w] : 0;
            tot += wcnt[w];
        }
        if (keep) {
            const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            out[run + before + (int32_t)r] = p;
        }
        run += tot;
        __syncthreads();
    }
}

hipError_t launch_associate(const float4* in, int64_t n, const Mat3x4d& M, float4* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(associate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, n, M, out);
    return hipGetLastError();
}

int64_t sector_blocks(int64_t n) { return (n + kSecBlock - 1) / kSecBlock; }

// The stable compaction of the n-element sequence pr describes: count per block -> scan -> ordered
// write of the kept elements to out (room for every kept element), their number to *total.
template <class Pred>
hipError_t launch_compact(const Pred& pr, int64_t n, int32_t* counts, int32_t* offsets, int32_t* total, float4* out,
                          hipStream_t st) {
    const int64_t nblk = sector_blocks(n);
    if (nblk == 0) return hipMemsetAsync(total, 0, sizeof(int32_t), st);
    hipLaunchKernelGGL(compact_count_kernel<Pred>, dim3((unsigned)nblk), dim3(kSecWG), 0, st, pr, n, counts);
    hipLaunchKernelGGL(sector_scan_kernel, dim3(1), dim3(1024), 0, st, counts, (int)nblk, offsets, total);
    hipLaunchKernelGGL(compact_write_kernel<Pred>, dim3((unsigned)nblk), dim3(kSecWG), 0, st, pr, n, offsets, out);
    return hipGetLastError();
}

hipError_t launch_sector(const float4* map, int64_t n, const SectorArgs& a, int32_t* counts, int32_t* offsets,
                         int32_t* total, float4* out, hipStream_t st) {
    return launch_compact(SectorPred{map, a}, n, counts, offsets, total, out, st);
}

hipError_t launch_box(const float4* map, int64_t n, const BoxArgs& b, int32_t* counts, int32_t* offsets,
                      int32_t* total, float4* out, hipStream_t st) {
    return launch_compact(BoxPred{map, b}, n, counts, offsets, total, out, st);
}

hipError_t launch_radius(const float4* map, int64_t n, const float* c, float radius, int32_t* counts,
                         int32_t* offsets, int32_t* total, float4* out, hipStream_t st) {
    return launch_compact(RadiusPred{map, c[0], c[1], c[2], radius * radius}, n, counts, offsets, total, out, st);
}

hipError_t launch_outside_boxes(const float4* map, int64_t n, const float* d_boxes, int32_t nb, int32_t* counts,
                                int32_t* offsets, int32_t* total, float4* out, hipStream_t st) {
    return launch_compact(OutsideBoxesPred{map, d_boxes, nb}, n, counts, offsets, total, out, st);
}

// ---- downsampled insert: Add_Points(points, true) (ikd_Tree.cpp:430-457), factored by downsample
// cell.  Of every cell an arrival falls in, one point stays: the nearest to the cell's centre among
// its stored members and its arrivals (an arrival wins a tie, the last tied arrival among arrivals,
// the lowest index among stored points); the counter follows the reference's sequential loop, which
// per cell is a walk over the cell's arrivals in input order.  Steps: claim a table slot per touched
// cell; per slot the stored members' count and nearest (integer atomics only); a stable radix sort of
// the arrivals by slot (8 bits per pass), which leaves each cell's arrivals adjacent and in input
// order; the walk, one thread per cell; one compaction of stored points + arrivals into the new store.
struct DsCell {
    float cx, cy, cz;  // floorf(p / ds), -0 as +0
    float dist;        // calc_dist(p, the box's centre)
    bool inside;       // lo <= p && hi > p on every axis
    bool nan;          // a cell coordinate is NaN: the point shares its cell with nothing
};

__device__ __forceinline__ DsCell ds_cell(const float4 p, float ds) {
    const float v[3] = {p.x, p.y, p.z};
    float c[3], mid[3];
    bool inside = true, nan = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = floorf(__fdiv_rn(v[k], ds));
        const float lo = c[k] * ds;
        const float hi = lo + ds;
        mid[k] = (float)((double)lo + (double)(float)(hi - lo) / 2.0);
        inside = inside && lo <= v[k] && hi > v[k];
        nan = nan || c[k] != c[k];
        if (c[k] == 0.0f) c[k] = 0.0f;
    }
    DsCell q;
    q.cx = c[0];
    q.cy = c[1];
    q.cz = c[2];
    q.dist = map_calc_dist(p.x, p.y, p.z, mid[0], mid[1], mid[2]);
    q.inside = inside;
    q.nan = nan;
    return q;
}

__device__ __forceinline__ uint32_t ds_hash(const DsCell& q) {
    uint32_t h = __float_as_uint(q.cx) * 0x9E3779B1u;
    h = (h ^ (h >> 15)) + __float_as_uint(q.cy) * 0x85EBCA77u;
    h = (h ^ (h >> 13)) + __float_as_uint(q.cz) * 0xC2B2AE3Du;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    return h;
}

__device__ __forceinline__ bool ds_same_cell(const DsCell& a, const DsCell& b) {
    return a.cx == b.cx && a.cy == b.cy && a.cz == b.cz;
}

// Per arrival: find or claim its cell's slot (rep[slot] = an arrival of that cell; keys are compared
// through that arrival's cell).  The table has `size` = mask + 1 >= 2 na slots, so a probe ends; which
// slot a cell gets may vary from run to run, what is computed per cell does not.  Slot `size` is the
// arrivals that share a cell with nothing (NaN coordinates).
__global__ __launch_bounds__(256) void ds_claim_kernel(const float4* __restrict__ arr, int32_t na, float ds,
                                                       int32_t* __restrict__ rep, uint32_t mask,
                                                       int2* __restrict__ pairs) {
    const int32_t j = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (j >= na) return;
    const DsCell q = ds_cell(arr[j], ds);
    int32_t slot = (int32_t)(mask + 1);
    if (!q.nan) {
        uint32_t s = ds_hash(q) & mask;
        for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
            int32_t r = rep[s];
            if (r < 0) r = atomicCAS(&rep[s], -1, j);
            if (r < 0 || ds_same_cell(ds_cell(arr[r], ds), q)) {
                slot = (int32_t)s;
                break;
            }
        }
    }
    pairs[j] = make_int2(slot, j);
}

// Per stored point that lies inside its own box and whose cell an arrival touched: count it and fold
// it into the cell's nearest stored member, (dist bits << 32 | index) by atomicMin.
__global__ __launch_bounds__(256) void ds_stored_kernel(const float4* __restrict__ map, int32_t n0,
                                                        const float4* __restrict__ arr, float ds,
                                                        const int32_t* __restrict__ rep, uint32_t mask,
                                                        int32_t* __restrict__ scount,
                                                        unsigned long long* __restrict__ smin,
                                                        int32_t* __restrict__ sslot) {
    const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n0) return;
    const DsCell q = ds_cell(map[i], ds);
    int32_t slot = -1;
    if (q.inside && !q.nan) {
        uint32_t s = ds_hash(q) & mask;
        for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
            const int32_t r = rep[s];
            if (r < 0) break;
            if (ds_same_cell(ds_cell(arr[r], ds), q)) {
                slot = (int32_t)s;
                break;
            }
        }
    }
    if (slot >= 0) {
        atomicAdd(&scount[slot], 1);
        atomicMin(&smin[slot], ((unsigned long long)__float_as_uint(q.dist) << 32) | (uint32_t)i);
    }
    sslot[i] = slot;
}

// Stable LSD radix sort of (slot, arrival) pairs by slot, one 8-bit digit per pass: per-block digit
// counts (digit-major, so one scan of 256 x nblk counts gives every block's first position per
// digit), then the ordered scatter.
__global__ __launch_bounds__(kSecWG) void ds_radix_count_kernel(const int2* __restrict__ in, int32_t n, int shift,
                                                                int32_t nblk, int32_t* __restrict__ counts) {
    __shared__ int32_t h[256];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kSecBlock;
    for (int k = 0; k < kSecPer; ++k) {
        const int64_t i = base + k * kSecWG + tid;
        if (i < n) atomicAdd(&h[(in[i].x >> shift) & 255], 1);
    }
    __syncthreads();
    counts[(int64_t)tid * nblk + blockIdx.x] = h[tid];
}

__global__ __launch_bounds__(kSecWG) void ds_radix_scatter_kernel(const int2* __restrict__ in, int2* __restrict__ out,
                                                                  int32_t n, int shift, int32_t nblk,
                                                                  const int32_t* __restrict__ offsets) {
    static_assert(kSecWG == 256, "one thread per digit");
    __shared__ int32_t first[256];                // next output position per digit
    __shared__ int32_t wcnt[kSecWG / 64][256];    // this round's elements per wave and digit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * kSecBlock;
    first[tid] = offsets[(int64_t)tid * nblk + blockIdx.x];
    for (int k = 0; k < kSecPer; ++k) {
#pragma unroll
        for (int w = 0; w < kSecWG / 64; ++w) wcnt[w][tid] = 0;
        __syncthreads();
        const int64_t i = base + k * kSecWG + tid;
        const bool valid = i < n;
        const int2 e = valid ? in[i] : make_int2(0, 0);
        const int d = (e.x >> shift) & 255;
        uint64_t same = __ballot(valid);  // the wave's valid lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const uint64_t bm = __ballot(bit);
            same &= bit ? bm : ~bm;
        }
        const int rank = __builtin_popcountll(same & (((uint64_t)1 << lane) - 1));
        if (valid && rank == 0) wcnt[wave][d] = __builtin_popcountll(same);
        __syncthreads();
        if (valid) {
            int pos = first[d] + rank;
            for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
            out[pos] = e;
        }
        int add = 0;
#pragma unroll
        for (int w = 0; w < kSecWG / 64; ++w) add += wcnt[w][tid];
        __syncthreads();
        first[tid] += add;
    }
}

// Sorts n (key, value) pairs by the low `bits` bits of the key, stably, 8 bits per pass, ping-ponging
// between a and b; -> the buffer that holds the result.  counts / offsets: 256 * sector_blocks(n)
// entries each; total: one int32 the scans write.
int2* launch_radix_sort(int2* a, int2* b, int32_t n, int bits, int32_t* counts, int32_t* offsets, int32_t* total,
                        hipStream_t st) {
    const int32_t nblk = (int32_t)sector_blocks(n);
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(ds_radix_count_kernel, dim3((unsigned)nblk), dim3(kSecWG), 0, st, a, n, shift, nblk, counts);
        hipLaunchKernelGGL(wide_scan_kernel, dim3(1), dim3(1024), 0, st, counts, 256 * nblk, offsets, total);
        hipLaunchKernelGGL(ds_radix_scatter_kernel, dim3((unsigned)nblk), dim3(kSecWG), 0, st, a, b, n, shift, nblk,
                           offsets);
        int2* t = a;
        a = b;
        b = t;
    }
    return a;
}

hipError_t launch_block_scan(const int32_t* counts, int nblk, int32_t* offsets, int32_t* total, hipStream_t st) {
    hipLaunchKernelGGL(wide_scan_kernel, dim3(1), dim3(1024), 0, st, counts, nblk, offsets, total);
    return hipGetLastError();
}

// bbox[0..2] = min, bbox[3..5] = max over the finite points (set to all-ones / zero beforehand; no
// finite point leaves min = +inf, max = -inf).
__global__ __launch_bounds__(256) void finite_bbox_kernel(const float4* __restrict__ pts, int64_t n,
                                                          uint32_t* __restrict__ bbox) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float4 p = pts[i];
        if (finite_xyz(p)) {
            lo[0] = fminf(lo[0], p.x), hi[0] = fmaxf(hi[0], p.x);
            lo[1] = fminf(lo[1], p.y), hi[1] = fmaxf(hi[1], p.y);
            lo[2] = fminf(lo[2], p.z), hi[2] = fmaxf(hi[2], p.z);
        }
    }
    // Waves -> workgroup through LDS, then one atomic per word, and only where it can still move the
    // word: every wave of a launch hitting the same six words costs ~10 ns per atomic at one L2
    // channel (0.5 ms of a 6.5 M-point map's 0.57 ms).  A stale read only costs a needless atomic: the
    // words move one way.
    __shared__ uint32_t part[4][6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // (every lane is here: the DPP reductions need the whole wave)
        const float l = wave_minf(lo[k]), h = wave_maxf(hi[k]);
        if ((threadIdx.x & 63) == 0) {
            part[threadIdx.x >> 6][k] = float_ord(l);
            part[threadIdx.x >> 6][3 + k] = float_ord(h);
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        uint32_t v = part[0][k];
        for (int w = 1; w < 4; ++w) v = k < 3 ? min(v, part[w][k]) : max(v, part[w][k]);
        const uint32_t cur = __builtin_nontemporal_load(&bbox[k]);
        if (k < 3 ? v < cur : v > cur) {
            if (k < 3) atomicMin(&bbox[k], v);
            else atomicMax(&bbox[k], v);
        }
    }
}

hipError_t launch_finite_bbox(const float4* pts, int64_t n, uint32_t* bbox, hipStream_t st) {
    hipError_t e;
    if ((e = hipMemsetAsync(bbox, 0xFF, 3 * sizeof(uint32_t), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(bbox + 3, 0, 3 * sizeof(uint32_t), st)) != hipSuccess) return e;
    const int64_t bb = (n + 255) / 256;
    if (bb > 0) hipLaunchKernelGGL(finite_bbox_kernel,dim3((unsigned)(bb < 2048 ? bb : 2048)), dim3(256), 0, st, pts, n, bbox);
    return hipGetLastError();
}

// KD_TREE::same_point (ikd_Tree.cpp:1422-1423): float fabs against the double 1e-6.
__device__ __forceinline__ bool ds_same_point(const float4 a, const float4 b) {
    return (double)fabsf(a.x - b.x) < 1e-6 && (double)fabsf(a.y - b.y) < 1e-6 && (double)fabsf(a.z - b.z) < 1e-6;
}

// The reference's loop per cell: the thread at a cell's first sorted arrival walks the cell's arrivals
// in input order against the holder (first the nearest stored member), counts as the reference does,
// and leaves the point that stays: swin[slot] (a stored point) or akeep (an arrival).
__global__ __launch_bounds__(256) void ds_walk_kernel(const int2* __restrict__ pairs, int32_t na, int32_t size,
                                                      const float4* __restrict__ map, const float4* __restrict__ arr,
                                                      float ds, const int32_t* __restrict__ scount,
                                                      const unsigned long long* __restrict__ smin,
                                                      int32_t* __restrict__ swin, int32_t* __restrict__ akeep,
                                                      int32_t* __restrict__ counter) {
    const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    int cnt = 0;
    if (t < na) {
        const int32_t slot = pairs[t].x;
        if (slot >= size) {  // alone in its cell: stays and counts
            akeep[pairs[t].y] = 1;
            cnt = 1;
        } else if (t == 0 || pairs[t - 1].x != slot) {
            const int32_t ns = scount[slot];
            bool has = ns > 0;
            int32_t hstored = -1, harr = -1;
            float hd = 0.0f;
            float4 hp = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has) {
                const NNKey key = smin[slot];
                hstored = key_idx(key);
                hd = key_d2(key);
                hp = map[hstored];
            }
            for (int32_t u = t; u < na && pairs[u].x == slot; ++u) {
                const int32_t j = pairs[u].y;
                const float4 p = arr[j];
                const float dj = ds_cell(p, ds).dist;
                if (!has || !(hd < dj)) {  // the arrival is at least as near: it takes the cell
                    has = true;
                    hd = dj;
                    hp = p;
                    harr = j;
                    hstored = -1;
                    ++cnt;
                } else if ((u == t && ns > 1) || ds_same_point(p, hp)) {
                    ++cnt;  // counted by the reference, then dropped
                }
            }
            swin[slot] = hstored;
            if (harr >= 0) akeep[harr] = 1;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(counter, cnt);
}

int ds_table_log2(int64_t na) {
    int b = 8;
    while (((int64_t)1 << b) < 2 * na) ++b;
    return b;
}

static size_t ds_align(size_t x) { return (x + 255) & ~(size_t)255; }

DsLayout ds_layout(int64_t n0, int64_t na) {
    DsLayout L;
    const size_t size = (size_t)1 << ds_table_log2(na);
    const size_t nblk = (size_t)sector_blocks(na);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += ds_align(bytes);
        return at;
    };
    L.smin = take(size * 8);
    L.rep = take(size * 4);
    L.scount = take(size * 4);
    L.swin = take(size * 4);
    L.pairs_a = take((size_t)na * 8);
    L.pairs_b = take((size_t)na * 8);
    L.sslot = take((size_t)(n0 > 0 ? n0 : 1) * 4);
    L.akeep = take((size_t)na * 4);
    L.rcounts = take(256 * nblk * 4);
    L.roffsets = take(256 * nblk * 4);
    L.counter = take(8);  // the counter, the radix scans' total
    L.bytes = o;
    return L;
}

hipError_t launch_downsample(const float4* map, int64_t n0, const float4* arr, int64_t na, float ds, void* scratch,
                             int32_t* counts, int32_t* offsets, int32_t* total, float4* out, int32_t** counter,
                             hipStream_t st) {
    const DsLayout L = ds_layout(n0, na);
    char* w = static_cast<char*>(scratch);
    const int bits = ds_table_log2(na);
    const int32_t size = (int32_t)1 << bits;
    const uint32_t mask = (uint32_t)size - 1u;
    auto* smin = reinterpret_cast<unsigned long long*>(w + L.smin);
    auto* rep = reinterpret_cast<int32_t*>(w + L.rep);
    auto* scount = reinterpret_cast<int32_t*>(w + L.scount);
    auto* swin = reinterpret_cast<int32_t*>(w + L.swin);
    int2* pa = reinterpret_cast<int2*>(w + L.pairs_a);
    int2* pb = reinterpret_cast<int2*>(w + L.pairs_b);
    auto* sslot = reinterpret_cast<int32_t*>(w + L.sslot);
    auto* akeep = reinterpret_cast<int32_t*>(w + L.akeep);
    auto* rcounts = reinterpret_cast<int32_t*>(w + L.rcounts);
    auto* roffsets = reinterpret_cast<int32_t*>(w + L.roffsets);
    int32_t* cnt = reinterpret_cast<int32_t*>(w + L.counter);
    *counter = cnt;
    hipError_t e;
    // smin and rep are adjacent: all ones = no stored member (max key), no representative (-1)
    if ((e = hipMemsetAsync(w + L.smin, 0xFF, L.scount - L.smin, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(scount, 0, (size_t)size * 4, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(akeep, 0, (size_t)na * 4, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(cnt, 0, 8, st)) != hipSuccess) return e;
    const unsigned ga = (unsigned)((na + 255) / 256);
    hipLaunchKernelGGL(ds_claim_kernel, dim3(ga), dim3(256), 0, st, arr, (int32_t)na, ds, rep, mask, pa);
    if (n0 > 0)
        hipLaunchKernelGGL(ds_stored_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, map, (int32_t)n0, arr,
                           ds, rep, mask, scount, smin, sslot);
    pa = launch_radix_sort(pa, pb, (int32_t)na, bits + 1, rcounts, roffsets, cnt + 1, st);  // slots 0 .. size: bits + 1 key bits
    hipLaunchKernelGGL(ds_walk_kernel, dim3(ga), dim3(256), 0, st, pa, (int32_t)na, size, map, arr, ds, scount, smin, swin,
                       akeep, cnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_compact(DsPred{map, arr, n0, sslot, swin, akeep}, n0 + na, counts, offsets, total, out, st);
}

}  // namespace icp4r
