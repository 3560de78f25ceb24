// icp4r_vgicp.hip — voxelized generalized ICP for gfx950 (include/icp4r/icp4r_vgicp.h states the
// algorithm).
//
// fast_gicp's FastVGICP restated device-resident, beside the GICP of icp4r_gicp.hip:
//
//   the map build        vgicp_key_kernel    per target point: the cell key (3 x 21 bits) of floor(p / resolution)
//                        the store's stable LSD radix sort of (key word, element) pairs: the key's low
//                        word, its high word, then (batches) the pair — the elements end ordered by (pair,
//                        key, index)
//                        vx_compact          the voxels: the first element of every run of equal keys,
//                        in order (the stable compaction of icp4r_voxel_common.hpp)
//                        vgicp_bounds_kernel each pair's voxel range (a binary search per pair)
//                        vgicp_sum_kernel    one lane per voxel: Σp and ΣC over its run, sequentially in
//                        ascending target index, then mean and cov
//   per iteration        vgicp_lin_kernel    over slices of the source (gicp_slice_pts, as GICP): the cell of
//                        Ta, a binary search of the pair's sorted voxel keys per offset (deterministic,
//                        independent of insertion order), W = sqrt(num) (cov_v + R C_i Rᵀ)⁻¹, the sums of
//                        H, g, y; the last slice adds the slices in order and solves the first LM trials
//                        vgicp_trial_kernel  the trials' errors over the stored correspondences with W
//                        recomputed from R0; the last slice decides
//
// No nearest-neighbour pass and no move of X in the loop: the fitness pass forms X from the final pose.
// The sums use no double atomics: fixed-order wave reductions, waves in order, slices in order; the
// workgroups of a pair meet only through gicp_publish / gicp_last_slice.
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icp4r_device.hpp"
#include "icp4r_gicp_dev.hpp"
#include "icp4r_internal.hpp"
#include "icp4r_vgicp.hpp"
#include "icp4r_vgicp_math.hpp"
#include "icp4r_voxel_common.hpp"

namespace icp4r {

namespace vg = icp4r_vgicp;

constexpr int kVgWG = 256;

static size_t vg_align(size_t b) { return (b + 255) & ~(size_t)255; }

VgicpLayout vgicp_layout(int64_t npairs, int64_t t_stride, int64_t x_stride, int noff) {
    const size_t N = (size_t)(npairs * t_stride);
    const size_t nblk = (size_t)sector_blocks((int64_t)N) > (size_t)vx_blocks((int64_t)N) ? (size_t)sector_blocks((int64_t)N)
                                                                                        : (size_t)vx_blocks((int64_t)N);
    VgicpLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += vg_align(bytes);
        return at;
    };
    L.pkey = take(N * sizeof(uint64_t));
    L.pa = take(N * sizeof(int2));
    L.pb = take(N * sizeof(int2));
    L.counts = take(256 * nblk * sizeof(int32_t));
    L.offsets = take(256 * nblk * sizeof(int32_t));
    L.total = take(2 * sizeof(int32_t));
    L.vstart = take(N * sizeof(int32_t));
    L.bad = take((size_t)npairs * sizeof(int32_t));
    L.vkey = take(N * sizeof(uint64_t));
    L.vnum = take(N * sizeof(int32_t));
    L.vmean = take(N * 3 * sizeof(double));
    L.vcov = take(N * 6 * sizeof(double));
    L.vbeg = take((size_t)(npairs + 1) * sizeof(int32_t));
    L.corr = take((size_t)(npairs * x_stride) * (size_t)noff * sizeof(int32_t));
    L.bytes = o;
    return L;
}

void vgicp_bind(void* work, const VgicpLayout& L, VgicpArgs& m) {
    char* w = static_cast<char*>(work);
    m.pkey = reinterpret_cast<uint64_t*>(w + L.pkey);
    m.pa = reinterpret_cast<int2*>(w + L.pa);
    m.pb = reinterpret_cast<int2*>(w + L.pb);
    m.counts = reinterpret_cast<int32_t*>(w + L.counts);
    m.offsets = reinterpret_cast<int32_t*>(w + L.offsets);
    m.total = reinterpret_cast<int32_t*>(w + L.total);
    m.vstart = reinterpret_cast<int32_t*>(w + L.vstart);
    m.bad = reinterpret_cast<int32_t*>(w + L.bad);
    m.vkey = reinterpret_cast<uint64_t*>(w + L.vkey);
    m.vnum = reinterpret_cast<int32_t*>(w + L.vnum);
    m.vmean = reinterpret_cast<double*>(w + L.vmean);
    m.vcov = reinterpret_cast<double*>(w + L.vcov);
    m.vbeg = reinterpret_cast<int32_t*>(w + L.vbeg);
    m.corr = reinterpret_cast<int32_t*>(w + L.corr);
    m.sorted = nullptr;
}

// ---- the map build

// the cell key of a point, or kNoKey with *out = true when a coordinate lies outside the key range
__device__ __forceinline__ uint64_t vgicp_key_of(double x, double y, double z, double res, bool* out) {
    const double c[3] = {vg::cell_of(x, res), vg::cell_of(y, res), vg::cell_of(z, res)};
    if (!(vg::cell_in_range(c[0]) && vg::cell_in_range(c[1]) && vg::cell_in_range(c[2]))) {
        *out = true;
        return vg::kNoKey;
    }
    return vg::cell_key((int32_t)c[0], (int32_t)c[1], (int32_t)c[2]);
}

__global__ __launch_bounds__(kVgWG) void vgicp_key_kernel(const float4* __restrict__ tgt, const int64_t* __restrict__ off,
                                                          const int32_t* __restrict__ cnt, const PairState* state,
                                                          VgicpArgs m, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * kVgWG + threadIdx.x;
    if (e >= total) return;
    const int p = (int)(e / m.t_stride), i = (int)(e - (int64_t)p * m.t_stride);
    uint64_t key = vg::kNoKey;
    if (i < cnt[p] && !(state && state[p].phase == kPhaseInvalid)) {
        const float4 q = tgt[off[p] + i];
        bool out = false;
        key = vgicp_key_of((double)q.x, (double)q.y, (double)q.z, m.resolution, &out);
        if (out) m.bad[p] = 1;  // (every writer stores the same value)
    }
    m.pkey[e] = key;
    m.pa[e] = make_int2((int32_t)(uint32_t)key, (int32_t)e);
}

// the next sort's key word of every element: word 1 the cell key's high word, word 2 the pair
__global__ __launch_bounds__(kVgWG) void vgicp_rekey_kernel(int2* __restrict__ s, const uint64_t* __restrict__ pkey,
                                                            int64_t total, int64_t t_stride, int word) {
    const int64_t e = (int64_t)blockIdx.x * kVgWG + threadIdx.x;
    if (e >= total) return;
    const int32_t el = s[e].y;
    s[e].x = word == 1 ? (int32_t)(uint32_t)(pkey[el] >> 32) : (int32_t)(el / t_stride);
}

// the compaction's test: the first element of a run of equal keys inside a pair's segment (the sort
// leaves pair p's elements at [p * t_stride, (p + 1) * t_stride), padding last)
struct VgicpHeads {
    const int2* sorted;
    const uint64_t* pkey;
    int64_t n, t_stride;
    int32_t* vstart;
    uint64_t* vkey;
    __device__ int64_t size() const { return n; }
    __device__ bool keep(int64_t s) const {
        const uint64_t k = pkey[sorted[s].y];
        if (k == vg::kNoKey) return false;
        return s % t_stride == 0 || pkey[sorted[s - 1].y] != k;
    }
    __device__ void emit(int64_t s, int32_t rank) const {
        vstart[rank] = (int32_t)s;
        vkey[rank] = pkey[sorted[s].y];
    }
};

// each pair's first voxel (vbeg[npairs]: the batch's count); a pair with a coordinate outside the key
// range becomes invalid, as init_kernel leaves an invalid pair
__global__ void vgicp_bounds_kernel(VgicpArgs m, PairState* state, int npairs) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > npairs) return;
    const int nv = m.total[0];
    const int64_t want = (int64_t)p * m.t_stride;
    int lo = 0, hi = nv;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)m.vstart[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    m.vbeg[p] = lo;
    if (p < npairs && state && m.bad[p] && state[p].phase != kPhaseInvalid) {
        PairState& st = state[p];
        mat4_identity(st.final_T);
        st.phase = kPhaseInvalid;
        st.status = kStatusInvalid;
    }
}

// one lane per voxel: Σp and ΣC over its run of the sorted elements — ascending target index, the sort
// being stable — starting from the first term, then mean = Σp / num and cov = ΣC / num
__global__ __launch_bounds__(kVgWG) void vgicp_sum_kernel(const float4* __restrict__ tgt, const int64_t* __restrict__ off,
                                                          const double* __restrict__ cov6, VgicpArgs m) {
    const int v = blockIdx.x * kVgWG + threadIdx.x;
    if (v >= m.total[0]) return;
    const int64_t s0 = m.vstart[v];
    const int p = (int)(s0 / m.t_stride);
    const int64_t end = (int64_t)(p + 1) * m.t_stride;
    const uint64_t key = m.vkey[v];
    const float4* c = tgt + off[p];
    double sp[3], sc[6];
    int num = 0;
    for (int64_t s = s0; s < end; ++s) {
        const int32_t el = m.sorted[s].y;
        if (s > s0 && m.pkey[el] != key) break;
        const int i = (int)(el - (int64_t)p * m.t_stride);
        const float4 q = c[i];
        const double* cv = cov6 + (int64_t)el * 6;
        if (num == 0) {
            sp[0] = (double)q.x, sp[1] = (double)q.y, sp[2] = (double)q.z;
            for (int t = 0; t < 6; ++t) sc[t] = cv[t];
        } else {
            sp[0] += (double)q.x, sp[1] += (double)q.y, sp[2] += (double)q.z;
            for (int t = 0; t < 6; ++t) sc[t] += cv[t];
        }
        ++num;
    }
    m.vnum[v] = num;
    for (int t = 0; t < 3; ++t) m.vmean[(int64_t)v * 3 + t] = sp[t] / (double)num;
    for (int t = 0; t < 6; ++t) m.vcov[(int64_t)v * 6 + t] = sc[t] / (double)num;
}

hipError_t launch_vgicp_map(const float4* tgt, const int64_t* off, const int32_t* cnt, const double* cov6,
                            PairState* state, VgicpArgs& m, int npairs, hipStream_t st) {
    const int64_t N = (int64_t)npairs * m.t_stride;
    if (npairs <= 0 || N <= 0) return hipSuccess;
    if (N > INT32_MAX) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((N + kVgWG - 1) / kVgWG);
    hipError_t e = hipMemsetAsync(m.bad, 0, (size_t)npairs * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vgicp_key_kernel, dim3(blocks), dim3(kVgWG), 0, st, tgt, off, cnt, state, m, N);
    // the key's low word, its high word (kNoKey's is all ones: 32 bits), then the pair
    int2* s = launch_radix_sort(m.pa, m.pb, (int32_t)N, 32, m.counts, m.offsets, m.total + 1, st);
    hipLaunchKernelGGL(vgicp_rekey_kernel, dim3(blocks), dim3(kVgWG), 0, st, s, m.pkey, N, m.t_stride, 1);
    s = launch_radix_sort(s, s == m.pa ? m.pb : m.pa, (int32_t)N, 32, m.counts, m.offsets, m.total + 1, st);
    if (npairs > 1) {
        int bits = 1;
        while ((1 << bits) < npairs) ++bits;
        hipLaunchKernelGGL(vgicp_rekey_kernel, dim3(blocks), dim3(kVgWG), 0, st, s, m.pkey, N, m.t_stride, 2);
        s = launch_radix_sort(s, s == m.pa ? m.pb : m.pa, (int32_t)N, bits, m.counts, m.offsets, m.total + 1, st);
    }
    m.sorted = s;
    const VgicpHeads heads = {s, m.pkey, N, m.t_stride, m.vstart, m.vkey};
    if ((e = vx_compact(heads, N, m.counts, m.offsets, m.total, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(vgicp_bounds_kernel, dim3((npairs + 1 + 255) / 256), dim3(256), 0, st, m, state, npairs);
    // (the voxel count is on the device: a lane per element, those past the count return)
    hipLaunchKernelGGL(vgicp_sum_kernel, dim3(blocks), dim3(kVgWG), 0, st, tgt, off, cov6, m);
    return hipGetLastError();
}

// ---- per iteration

struct VgicpPairView {
    int n, ps, ns;  // points, points per slice, slices
    int vb, ve;     // the pair's voxels
    const float4* src;
    const double* cs;
    int32_t* corr;
};

__device__ __forceinline__ VgicpPairView vgicp_view(const PairArgs& a, const WorkArgs& w, const GicpArgs& g,
                                                    const VgicpArgs& m, int p) {
    VgicpPairView v;
    v.n = a.src_n[p];
    v.ps = gicp_slice_pts(v.n);
    v.ns = gicp_slices(v.n);
    v.vb = m.vbeg[p];
    v.ve = m.vbeg[p + 1];
    v.src = a.src + a.src_off[p];
    v.cs = g.cov_src + (int64_t)p * w.x_stride * 6;
    v.corr = m.corr + (int64_t)p * w.x_stride * m.noff;
    return v;
}

// the voxel of `key` among the sorted keys [lo, hi), or -1
__device__ __forceinline__ int vgicp_find(const uint64_t* __restrict__ vkey, int lo, int hi, uint64_t key) {
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (vkey[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && vkey[lo] == key ? lo : -1;
}

// P = R C Rᵀ of a source point's covariance (packed upper triangle), GICP's operation order
__device__ __forceinline__ void vgicp_rcr(const double* R, const double* c6, double (&P)[9]) {
    double CA[9], RC[9];
    sym_unpack(c6, CA);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) RC[3 * r + c] = R[3 * r] * CA[c] + R[3 * r + 1] * CA[3 + c] + R[3 * r + 2] * CA[6 + c];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) P[3 * r + c] = RC[3 * r] * R[3 * c] + RC[3 * r + 1] * R[3 * c + 1] + RC[3 * r + 2] * R[3 * c + 2];
}

// W = sqrt(num_v) (cov_v + P)⁻¹: the cofactor inverse, its upper triangle scaled and mirrored
__device__ __forceinline__ void vgicp_weight(const VgicpArgs& m, int v, const double (&P)[9], double (&W)[9]) {
    double CB[9], S[9], Mi[9];
    sym_unpack(m.vcov + (int64_t)v * 6, CB);
    for (int t = 0; t < 9; ++t) S[t] = CB[t] + P[t];
    gicp_inv3(S, Mi);
    const double w = sqrt((double)m.vnum[v]);
    const double m6[6] = {w * Mi[0], w * Mi[1], w * Mi[2], w * Mi[4], w * Mi[5], w * Mi[8]};
    sym_unpack(m6, W);
}

// the error terms of point i's stored correspondences at (R, t) with W from R0, into e[0]
__device__ __forceinline__ void vgicp_point_err(const VgicpPairView& v, const VgicpArgs& m, int i, const double* R0,
                                                const double* R, const double* t, double* e) {
    const float4 sa = v.src[i];
    const double a[3] = {sa.x, sa.y, sa.z};
    double ta[3], P[9];
    bool have = false;
    for (int q = 0; q < m.noff; ++q) {
        const int vx = v.corr[(int64_t)i * m.noff + q];
        if (vx < 0) continue;
        if (!have) {
            vg::transform(R, t, a, ta);
            vgicp_rcr(R0, v.cs + (int64_t)i * 6, P);
            have = true;
        }
        double W[9];
        vgicp_weight(m, vx, P, W);
        const double* mu = m.vmean + (int64_t)vx * 3;
        const double ev[3] = {mu[0] - ta[0], mu[1] - ta[1], mu[2] - ta[2]};
        gicp_terms<false>(ta, ev, W, e);
    }
}

// (1) the lookup and the linearisation over one slice: the voxels of every (point, offset) (kept for the
// trials) and the slice's sums of H, g, y and the number of correspondences at x0.  The last slice sums
// the slices in order and solves the first LM trials.
__global__ __launch_bounds__(kGicpSliceWG) void vgicp_lin_kernel(PairArgs a, WorkArgs w, GicpArgs g, VgicpArgs m,
                                                                 int npairs, int W) {
    __shared__ double red[kGicpSliceWaves * kGicpSys];
    __shared__ int32_t last;
    int p, j;
    if (!gicp_block(npairs, W, p, j)) return;
    if (w.state[p].phase != kPhaseActive) return;
    const VgicpPairView v = vgicp_view(a, w, g, m, p);
    if (j >= v.ns) return;
    const int nw = min(W, v.ns);
    const GicpState& gs = g.gs[p];
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = gs.R[k];
    for (int k = 0; k < 3; ++k) t[k] = gs.t[k];
    double* part = g.part_lin + (int64_t)p * kGicpMaxSlices * kGicpSys;
    for (int q = j; q < v.ns; q += W) {
        double acc[kGicpSys];
        for (int k = 0; k < kGicpSys; ++k) acc[k] = 0.0;
        const int hi = min(v.n, (q + 1) * v.ps);
        for (int i = q * v.ps + threadIdx.x; i < hi; i += kGicpSliceWG) {
            const float4 sa = v.src[i];
            const double av[3] = {sa.x, sa.y, sa.z};
            double ta[3];
            vg::transform(R, t, av, ta);
            const double c[3] = {vg::cell_of(ta[0], m.resolution), vg::cell_of(ta[1], m.resolution),
                                 vg::cell_of(ta[2], m.resolution)};
            // (a cell outside the key range, or no number: no neighbour of it is looked up)
            const bool in = vg::cell_in_range(c[0]) && vg::cell_in_range(c[1]) && vg::cell_in_range(c[2]);
            const int32_t ci[3] = {in ? (int32_t)c[0] : 0, in ? (int32_t)c[1] : 0, in ? (int32_t)c[2] : 0};
            double P[9];
            bool have = false;
#pragma unroll 1
            for (int o = 0; o < m.noff; ++o) {
                int32_t d[3];
                vg::offset_of(m.mode, o, d);
                const int32_t nx = ci[0] + d[0], ny = ci[1] + d[1], nz = ci[2] + d[2];
                int vx = -1;
                if (in && nx >= -vg::kBias && nx < vg::kBias && ny >= -vg::kBias && ny < vg::kBias && nz >= -vg::kBias &&
                    nz < vg::kBias)
                    vx = vgicp_find(m.vkey, v.vb, v.ve, vg::cell_key(nx, ny, nz));
                v.corr[(int64_t)i * m.noff + o] = vx;
                if (vx < 0) continue;
                if (!have) {
                    vgicp_rcr(R, v.cs + (int64_t)i * 6, P);
                    have = true;
                }
                double Wm[9];
                vgicp_weight(m, vx, P, Wm);
                const double* mu = m.vmean + (int64_t)vx * 3;
                const double e[3] = {mu[0] - ta[0], mu[1] - ta[1], mu[2] - ta[2]};
                gicp_terms<true>(ta, e, Wm, acc);
            }
        }
        const double r = gicp_slice_sum_sys(acc, red);
        if (threadIdx.x < kGicpSys) gicp_publish(part + q * kGicpSys + threadIdx.x, r);
    }
    if (!gicp_last_slice(g.cnt + p, nw, &last)) return;
    gicp_lin_finish(g, p, v.ns, part, red);
}

// (2) the trials' errors over one slice, on the stored correspondences with W from R0; the last slice
// sums them in order and decides.
__global__ __launch_bounds__(kGicpSliceWG) void vgicp_trial_kernel(PairArgs a, WorkArgs w, GicpArgs g, VgicpArgs m,
                                                                   int npairs, int W, int it) {
    __shared__ double red[kGicpSliceWaves * kGicpSpec];
    __shared__ double pose[kGicpSpec][12];
    __shared__ double r0[9];
    __shared__ int32_t last;
    int p, j;
    if (!gicp_block(npairs, W, p, j)) return;
    PairState& st = w.state[p];
    if (st.phase != kPhaseActive) return;
    const VgicpPairView v = vgicp_view(a, w, g, m, p);
    const int ns = v.ns;
    if (j >= ns) return;
    const int nw = min(W, ns);
    const int nt = min(g.spec, g.lm_max_iterations);
    const GicpCand& gc = g.cand[p];
    if (threadIdx.x < nt * 12) {
        const int k = threadIdx.x / 12, q = threadIdx.x % 12;
        pose[k][q] = q < 9 ? gc.c[k].R[q] : gc.c[k].t[q - 9];
    }
    if (threadIdx.x >= 64 && threadIdx.x < 64 + 9) r0[threadIdx.x - 64] = gc.R0[threadIdx.x - 64];
    __syncthreads();
    double* part = g.part_err + (int64_t)p * kGicpMaxSlices * kGicpSpec;
    for (int q = j; q < ns; q += W) {
        double acc[kGicpSpec];
        for (int k = 0; k < kGicpSpec; ++k) acc[k] = 0.0;
        const int hi = min(v.n, (q + 1) * v.ps);
        for (int i = q * v.ps + threadIdx.x; i < hi; i += kGicpSliceWG) {
            const float4 sa = v.src[i];
            const double av[3] = {sa.x, sa.y, sa.z};
            double P[9];
            bool have = false;
            for (int o = 0; o < m.noff; ++o) {
                const int vx = v.corr[(int64_t)i * m.noff + o];
                if (vx < 0) continue;
                if (!have) {
                    vgicp_rcr(r0, v.cs + (int64_t)i * 6, P);
                    have = true;
                }
                double Wm[9];
                vgicp_weight(m, vx, P, Wm);
                const double* mu = m.vmean + (int64_t)vx * 3;
                for (int k = 0; k < nt; ++k) {
                    double ta[3];
                    vg::transform(pose[k], pose[k] + 9, av, ta);
                    const double e[3] = {mu[0] - ta[0], mu[1] - ta[1], mu[2] - ta[2]};
                    gicp_terms<false>(ta, e, Wm, acc + k);
                }
            }
        }
        const double r = gicp_slice_sum(acc, red);
        if (threadIdx.x < kGicpSpec) gicp_publish(part + q * kGicpSpec + threadIdx.x, r);
    }
    if (!gicp_last_slice(g.cnt + p, nw, &last)) return;
    gicp_trial_finish(g, st, p, ns, nt, it, part, red, [&](int q, const double* R, const double* t, double* e) {
        const int hi = min(v.n, (q + 1) * v.ps);
        for (int i = q * v.ps + threadIdx.x; i < hi; i += kGicpSliceWG) vgicp_point_err(v, m, i, r0, R, t, e);
    });
}

hipError_t launch_vgicp_iter(const PairArgs& a, const WorkArgs& w, const GicpArgs& g, const VgicpArgs& m, int npairs,
                             int max_n, int it, hipStream_t st) {
    if (npairs <= 0) return hipSuccess;
    int W;
    unsigned blocks;
    gicp_iter_grid(npairs, max_n, g.grid, W, blocks);
    const dim3 grid(blocks), block(kGicpSliceWG);
    hipLaunchKernelGGL(vgicp_lin_kernel, grid, block, 0, st, a, w, g, m, npairs, W);
    hipLaunchKernelGGL(vgicp_trial_kernel, grid, block, 0, st, a, w, g, m, npairs, W, it);
    return hipGetLastError();
}

}  // namespace icp4r
