// icp4r_gate.hip — the Doppler gate for gfx950 (include/icp4r/icp4r_gate.h): a stable,
// batched stream compaction of float4 clouds by a byte mask into one tightly packed buffer.
//
// The reference node built with USE_STATIC_POINTS pushes only the static points of a scan into the
// clouds it registers (src/iterative_closest_point.cpp:404-406, :482-484), in input order.  Here the
// ego-velocity kernels leave the mask and the float4 points in HBM (ego_select_kernel,
// ego_features_kernel) and three launches pack every scan of a batch, no workgroup waiting on another:
//
//   gate_count_kernel    one wave per (scan, tile of kGateTile points): each lane reads 16 mask bytes
//                        as one 16-B word and counts the non-zero ones, the wave sums them
//   gate_scan_kernel     one workgroup: the exclusive scan over (scan, tile) in order — the tile bases —
//                        and the per-scan descriptors pair_off / pair_n ([s0, s0, s1, ...])
//   gate_scatter_kernel  one wave per (scan, tile), 64 points a round: rank = the tile's base + the kept
//                        lanes below (ballot prefix); float4 loads and stores of the kept points only
//
// Integer arithmetic only, no atomics: the packed buffer is a function of the inputs alone.  A scan
// whose count is negative or above max_n counts 0 and its mask is never read (ego_select_kernel
// refuses such a scan and writes no mask for it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp4r/icp4r_gate.h"
#include "icp4r_internal.hpp"

namespace icp4r {

__device__ __forceinline__ int gate_scan_n(const GateArgs& g, int s) {
    const int n = g.cnt[s];
    return (n < 0 || n > g.max_n) ? 0 : n;
}

// the non-zero bytes of a word: bit 7 of each byte := (low 7 bits != 0) | bit 7
__device__ __forceinline__ int gate_nz_bytes(uint32_t w) {
    return __popc((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u);
}

__global__ __launch_bounds__(256) void gate_count_kernel(GateArgs g) {
    const int s = blockIdx.y, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= g.tiles) return;
    const int n = gate_scan_n(g, s);
    const int i0 = tile * kGateTile + lane * 16;
    int c = 0;
    if (i0 < n) {
        const int len = min(16, n - i0);
        if (g.all) {
            c = len;
        } else {
            const uint8_t* m = g.mask + (g.off[s] + i0);
            if (len == 16 && ((uintptr_t)m & 15) == 0) {
                const uint4 v = *reinterpret_cast<const uint4*>(m);
                c = gate_nz_bytes(v.x) + gate_nz_bytes(v.y) + gate_nz_bytes(v.z) + gate_nz_bytes(v.w);
            } else {  // the scan's last word, or a scan that does not start on a 16-B boundary
                for (int k = 0; k < len; ++k) c += m[k] != 0 ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if (lane == 0) g.counts[(int64_t)s * g.tiles + tile] = c;
}

constexpr int kGateScanWG = 256;

__global__ __launch_bounds__(kGateScanWG) void gate_scan_kernel(GateArgs g) {
    __shared__ int wsum[kGateScanWG / 64];
    __shared__ long long carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t E = (int64_t)g.nscans * g.tiles;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t e0 = 0; e0 < E; e0 += kGateScanWG) {
        const int64_t e = e0 + tid;
        const int c = e < E ? g.counts[e] : 0;
        int inc = c;  // inclusive scan within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int wbase = 0;
        for (int w = 0; w < wave; ++w) wbase += wsum[w];
        const long long b = carry + wbase + inc - c;
        if (e < E) {
            g.base[e] = b;
            if (e % g.tiles == 0) g.pair_off[1 + e / g.tiles] = b;
            if (e == 0) g.pair_off[0] = b;
        }
        __syncthreads();
        if (tid == kGateScanWG - 1) carry = b + c;
        __syncthreads();
    }
    for (int s = tid; s < g.nscans; s += kGateScanWG) {
        int n = 0;
        for (int t = 0; t < g.tiles; ++t) n += g.counts[(int64_t)s * g.tiles + t];
        g.pair_n[1 + s] = n;
        if (s == 0) g.pair_n[0] = n;
        if (g.bad && g.bad[s]) g.results[s].status = ICP4R_E_INVALID;  // a scan outside the workspace
    }
}

__global__ __launch_bounds__(256) void gate_scatter_kernel(GateArgs g) {
    const int s = blockIdx.y, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= g.tiles) return;
    const int n = gate_scan_n(g, s);
    const int t0 = tile * kGateTile;
    if (t0 >= n) return;
    const int end = min(n, t0 + kGateTile);
    const int64_t first = g.off[s];
    int64_t o = g.base[(int64_t)s * g.tiles + tile];
    for (int r = t0; r < end; r += 64) {  // wave-uniform trip count
        const int i = r + lane;
        const bool keep = i < end && (g.all || g.mask[first + i] != 0);
        const unsigned long long b = __ballot(keep);
        const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if (keep) g.clouds[o + below] = g.xyzi[first + i];
        o += __popcll(b);
    }
}

// Which scans the ego kernels may touch with a workspace of `cap` records (points and mask bytes
// indexed off[s] + i): a scan that reaches outside is handed to them as empty and flagged.
__global__ __launch_bounds__(256) void gate_guard_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ cnt,
                                                         int nscans, int max_n, int64_t cap, int32_t* __restrict__ cnt_safe,
                                                         int32_t* __restrict__ bad) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nscans) return;
    const int n = cnt[s];
    const int64_t o = off[s];
    const int64_t ext = n > 0 ? (int64_t)min(n, max(max_n, 1)) : 0;  // ego_features_kernel writes this many points
    const bool ok = n <= 0 || (o >= 0 && o <= cap - ext);
    cnt_safe[s] = ok ? n : 0;
    bad[s] = ok ? 0 : 1;
}

hipError_t launch_gate_guard(const int64_t* off, const int32_t* cnt, int nscans, int max_n, int64_t cap, int32_t* cnt_safe,
                             int32_t* bad, hipStream_t st) {
    if (nscans <= 0) return hipSuccess;
    hipLaunchKernelGGL(gate_guard_kernel, dim3((nscans + 255) / 256), dim3(256), 0, st, off, cnt, nscans, max_n, cap,
                       cnt_safe, bad);
    return hipGetLastError();
}

hipError_t launch_gate(const GateArgs& g, hipStream_t st) {
    if (g.nscans <= 0) return hipSuccess;
    const dim3 grid((g.tiles + 3) / 4, g.nscans);
    hipLaunchKernelGGL(gate_count_kernel, grid, dim3(256), 0, st, g);
    hipLaunchKernelGGL(gate_scan_kernel, dim3(1), dim3(kGateScanWG), 0, st, g);
    hipLaunchKernelGGL(gate_scatter_kernel, grid, dim3(256), 0, st, g);
    return hipGetLastError();
}

}  // namespace icp4r
