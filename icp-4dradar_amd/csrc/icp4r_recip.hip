// icp4r_recip.hip — reciprocal correspondences (pcl::registration::CorrespondenceEstimation::
// determineReciprocalCorrespondences, icp4r_params.use_reciprocal_correspondences).
//
// After the search of an iteration every source i of an active pair holds its key (d2_i, m): the exact
// nearest target of the moved point X_i.  PCL keeps i iff the exact nearest neighbour of t_m in X —
// the same float distance, ties to the lowest index — is i again.  In the project's key order: i is
// kept iff no source j has (d2(X_j, t_m), j) < (d2_i, i).  Two launches per iteration decide it:
//
//   recip_vote_kernel   every source in index order (sperm: kd / Morton, compact blocks although X
//                       moves — it moves rigidly) votes its key (d2_i, i) into its target's winner word
//                       by a u64 atomicMin (integer, order-free: the minimum is the minimum), writes
//                       its point into the sorted source copy and, per block of kRecipLeaf sources,
//                       the block's bounding box; it also clears the winner words of the next
//                       iteration (two buffers, taken in turn: no clearing launch).
//   recip_check_kernel  a source that lost its target's vote is rejected at once (the winner is a
//                       source with a smaller key at t_m).  A winner searches X from t_m, bounded by
//                       its own key: every block whose box can hold a point at most d2_i away is
//                       evaluated exactly, and any smaller key rejects.  A rejected source's d² is set
//                       to +inf in its key and its correspondence record: every update form drops
//                       d² > max_d2 (max_d2 <= FLT_MAX), every seed of the next pass re-evaluates
//                       the distance from the key's index, which is kept.
//
// Exact: the box bound is compared through kLbShrink as the forward searches do, and the distances are
// l2_simple's (symmetric in its two points bit for bit).  Deterministic: integer atomics only, and
// the result does not depend on the order of their arrival.  No host synchronisation.
#include "icp4r_device.hpp"

namespace icp4r {

constexpr int kRecipWG = 256;

__global__ __launch_bounds__(kRecipWG) void recip_vote_kernel(PairArgs a, WorkArgs w, RecipArgs r, int parity,
                                                              int max_n) {
    const int p = blockIdx.y;
    if (uload(&w.state[p].phase) != kPhaseActive) return;
    const int n = min(uload(a.src_n + p), max_n);
    const int m = (int)min((int64_t)uload(a.tgt_n + p), r.w_stride);
    NNKey* win = r.win + (int64_t)p * 2 * r.w_stride;
    NNKey* cur = win + (int64_t)parity * r.w_stride;
    NNKey* nxt = win + (int64_t)(parity ^ 1) * r.w_stride;
    for (int j = blockIdx.x * kRecipWG + threadIdx.x; j < m; j += gridDim.x * kRecipWG) nxt[j] = ~0ull;
    const int s = blockIdx.x * kRecipWG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (s - lane >= n) return;  // (wave-uniform)
    const bool live = s < n;
    const int64_t xs0 = (int64_t)p * w.x_stride;
    const int o = live ? (w.sperm ? w.sperm[xs0 + s] : s) : 0;
    const float4 v = live ? w.X[xs0 + o] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float lx = wave_minf(live ? v.x : INFINITY), ly = wave_minf(live ? v.y : INFINITY),
                lz = wave_minf(live ? v.z : INFINITY);
    const float hx = wave_maxf(live ? v.x : -INFINITY), hy = wave_maxf(live ? v.y : -INFINITY),
                hz = wave_maxf(live ? v.z : -INFINITY);
    if (lane == 0) {
        float4* box = r.rbox + ((int64_t)p * r.b_stride + s / kRecipLeaf) * 2;
        box[0] = make_float4(lx, ly, lz, 0.f);
        box[1] = make_float4(hx, hy, hz, 0.f);
    }
    if (!live) return;
    r.rsrc[(int64_t)p * r.s_stride + s] = make_float4(v.x, v.y, v.z, __uint_as_float((uint32_t)o));
    const NNKey k = w.nn_key[xs0 + o];
    const float d2 = key_d2(k);
    const uint32_t mi = (uint32_t)key_idx(k);
    if (!(d2 > a.kp.max_d2) && mi < (uint32_t)m) atomicMin(&cur[mi], make_key(d2, (uint32_t)o));
}

__global__ __launch_bounds__(kRecipWG) void recip_check_kernel(PairArgs a, WorkArgs w, RecipArgs r, int parity,
                                                               int max_n) {
    const int p = blockIdx.y;
    if (uload(&w.state[p].phase) != kPhaseActive) return;
    const int n = min(uload(a.src_n + p), max_n);
    const int m = (int)min((int64_t)uload(a.tgt_n + p), r.w_stride);
    const int s = blockIdx.x * kRecipWG + threadIdx.x;
    if (s - (int)(threadIdx.x & 63) >= n) return;  // (wave-uniform)
    const bool live = s < n;
    const int64_t xs0 = (int64_t)p * w.x_stride;
    const float4* src = r.rsrc + (int64_t)p * r.s_stride;
    const uint32_t o = __float_as_uint(src[min(s, n - 1)].w);
    const NNKey k = w.nn_key[xs0 + o];
    const float d2 = key_d2(k);
    const uint32_t mi = (uint32_t)key_idx(k);
    const bool cand = live && !(d2 > a.kp.max_d2) && mi < (uint32_t)m;
    const NNKey mine = make_key(d2, o);
    const NNKey* cur = r.win + ((int64_t)p * 2 + parity) * r.w_stride;
    bool keep = cand && cur[mi] == mine;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (keep) t = a.tgt[uload(a.tgt_off + p) + mi];
    // the blocks and their points are read at wave-uniform addresses: through the scalar cache
    const cv4f_ptr box = as_const(r.rbox + (int64_t)p * r.b_stride * 2);
    const cv4f_ptr pts = as_const(src);
    const int nb = (n + kRecipLeaf - 1) / kRecipLeaf;
    for (int b = 0; b < nb; ++b) {
        if (__ballot(keep) == 0) break;
        const v4f lo = box[2 * b], hi = box[2 * b + 1];
        if (keep && box_lb(lo, hi, t.x, t.y, t.z) * kLbShrink <= d2) {
            const int cnt = min(kRecipLeaf, n - b * kRecipLeaf);
            for (int e = 0; e < cnt; ++e) {
                const v4f q = pts[b * kRecipLeaf + e];
                if (make_key(l2_simple(t.x, t.y, t.z, q.x, q.y, q.z), __float_as_uint(q.w)) < mine) {
                    keep = false;
                    break;
                }
            }
        }
    }
    if (cand && !keep) {
        w.nn_key[xs0 + o] = make_key(INFINITY, mi);
        if (w.corr) w.corr[(xs0 + o) * 2 + 1].w = INFINITY;
    }
}

hipError_t launch_recip(const PairArgs& a, const WorkArgs& w, const RecipArgs& r, int npairs, int max_n, int parity,
                        hipStream_t st) {
    if (!r.win || !r.rsrc || !r.rbox || npairs <= 0 || (parity != 0 && parity != 1)) return hipErrorInvalidValue;
    const int mn = max_n > 0 ? max_n : 1;
    // (the workspace holds whole workgroups of sources, and a box per kRecipLeaf of them: run_pairs)
    if (r.s_stride < ((int64_t)mn + kRecipWG - 1) / kRecipWG * kRecipWG || r.b_stride * kRecipLeaf < r.s_stride)
        return hipErrorInvalidValue;
    const dim3 grid((mn + kRecipWG - 1) / kRecipWG, npairs);
    hipLaunchKernelGGL(recip_vote_kernel, grid, dim3(kRecipWG), 0, st, a, w, r, parity, mn);
    hipLaunchKernelGGL(recip_check_kernel, grid, dim3(kRecipWG), 0, st, a, w, r, parity, mn);
    return hipGetLastError();
}

}  // namespace icp4r
