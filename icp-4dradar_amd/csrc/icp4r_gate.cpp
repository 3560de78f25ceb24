// icp4r_gate.cpp — C ABI of Doppler-gated registration (include/icp4r/icp4r_gate.h): the ego-velocity
// kernels (icp4r_ego.hip), the gate's compaction (icp4r_gate.hip) and the batched ICP on one stream,
// and the node's running-cloud pairing on the host.  No CPU fallback: every device entry fails with
// ICP4R_E_HIP if the device path cannot run.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "icp4r/icp4r_gate.h"
#include "icp4r_gate_pairs.hpp"
#include "icp4r_host.hpp"
#include "icp4r_internal.hpp"

using icp4r::EgoArgs;
using icp4r::GateArgs;
using icp4r_host::fail;

namespace {

constexpr int32_t kMaxScans = 65535;      // grid.y of the per-scan launches
constexpr int32_t kMaxScanN = 1 << 30;    // tile indices stay in int32

int check_shape(int32_t nscans, int32_t max_n, int32_t mode) {
    if (nscans < 0 || max_n < 0) return fail(ICP4R_E_INVALID, "nscans = %d, max_n = %d", nscans, max_n);
    if (nscans > kMaxScans) return fail(ICP4R_E_TOO_LARGE, "%d scans in one batch (at most %d)", nscans, kMaxScans);
    if (max_n > kMaxScanN) return fail(ICP4R_E_TOO_LARGE, "max_n = %d (at most %d)", max_n, kMaxScanN);
    if (mode != ICP4R_GATE_STATIC && mode != ICP4R_GATE_ALL) return fail(ICP4R_E_INVALID, "gate mode %d", mode);
    return ICP4R_OK;
}

int check_ego_params(const icp4r_ego_params* p) {  // as icp4r_ego.cpp
    if (!p) return ICP4R_OK;
    if (!(p->sigma > 0)) return fail(ICP4R_E_INVALID, "sigma must be > 0");
    if (p->dynamic_threshold != p->dynamic_threshold) return fail(ICP4R_E_INVALID, "dynamic_threshold is NaN");
    return ICP4R_OK;
}

// The compaction's workspace and its launches.
int run_gate(icp4r_ctx* ctx, const float4* xyzi, const int64_t* off, const int32_t* cnt, const uint8_t* mask,
             int32_t nscans, int32_t max_n, int32_t mode, float4* clouds, int64_t* pair_off, int32_t* pair_n,
             const int32_t* bad, icp4r_ego_result* results, hipStream_t st) {
    GateArgs g;
    memset(&g, 0, sizeof(g));
    g.tiles = std::max(1, (max_n + icp4r::kGateTile - 1) / icp4r::kGateTile);
    const size_t entries = (size_t)nscans * (size_t)g.tiles;
    HIP_TRY(ctx->gate_counts.ensure(entries * sizeof(int32_t)));
    HIP_TRY(ctx->gate_base.ensure(entries * sizeof(int64_t)));
    g.xyzi = xyzi;
    g.off = off;
    g.cnt = cnt;
    g.mask = mask;
    g.nscans = nscans;
    g.max_n = max_n;
    g.all = mode == ICP4R_GATE_ALL;
    g.counts = static_cast<int32_t*>(ctx->gate_counts.p);
    g.base = static_cast<int64_t*>(ctx->gate_base.p);
    g.clouds = clouds;
    g.pair_off = pair_off;
    g.pair_n = pair_n;
    g.bad = bad;
    g.results = results;
    HIP_TRY(icp4r::launch_gate(g, st));
    return ICP4R_OK;
}

// Ego velocity then the gate over device-resident scans that lie within the first `cap` records.
int run_static(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt, int32_t nscans,
               int32_t max_n, int64_t cap, const icp4r_ego_params& p, int32_t mode, icp4r_ego_result* results,
               uint8_t* mask, float4* clouds, int64_t* pair_off, int32_t* pair_n, hipStream_t st) {
    const int64_t stride = max_n > 0 ? max_n : 1;
    const int32_t H = p.iterations > 0 ? p.iterations : (int)(max_n * 0.2);  // as icp4r_ego.cpp's workspace
    if (cap < 1) cap = 1;
    HIP_TRY(ctx->ego_feat.ensure((size_t)nscans * stride * sizeof(float4)));
    HIP_TRY(ctx->ego_pd.ensure((size_t)nscans * stride * sizeof(double4)));
    HIP_TRY(ctx->ego_scores.ensure((size_t)nscans * (H > 0 ? H : 1) * sizeof(int32_t)));
    HIP_TRY(ctx->ego_xyzi.ensure((size_t)cap * sizeof(float4)));
    HIP_TRY(ctx->gate_cnt.ensure((size_t)nscans * sizeof(int32_t)));
    HIP_TRY(ctx->gate_bad.ensure((size_t)nscans * sizeof(int32_t)));
    if (!mask) {
        HIP_TRY(ctx->gate_mask.ensure((size_t)cap));
        mask = static_cast<uint8_t*>(ctx->gate_mask.p);
    }
    int32_t* cnt_safe = static_cast<int32_t*>(ctx->gate_cnt.p);
    int32_t* bad = static_cast<int32_t*>(ctx->gate_bad.p);
    float4* xyzi = static_cast<float4*>(ctx->ego_xyzi.p);
    HIP_TRY(icp4r::launch_gate_guard(off, cnt, nscans, max_n, cap, cnt_safe, bad, st));
    EgoArgs e;
    memset(&e, 0, sizeof(e));
    e.rec = records;
    e.off = off;
    e.cnt = cnt_safe;
    e.stride = stride;
    e.feat = static_cast<float4*>(ctx->ego_feat.p);
    e.pd = static_cast<double4*>(ctx->ego_pd.p);
    e.scores = static_cast<int32_t*>(ctx->ego_scores.p);
    e.max_h = H > 0 ? H : 0;
    e.iterations = p.iterations;
    e.sigma = p.sigma;
    e.dyn = p.dynamic_threshold;
    e.seed = p.seed;
    e.mask = mask;
    e.results = results;
    HIP_TRY(icp4r::launch_ego(e, nscans, (int)stride, xyzi, st));
    return run_gate(ctx, xyzi, off, cnt_safe, mask, nscans, max_n, mode, clouds, pair_off, pair_n, bad, results, st);
}

}  // namespace

extern "C" {

int icp4r_compact_by_mask_batch_device(icp4r_ctx* ctx, const float* xyzi, const int64_t* off, const int32_t* cnt,
                                       const uint8_t* mask, int32_t nscans, int32_t max_n, int32_t mode,
                                       float* clouds, int64_t* pair_off, int32_t* pair_n, void* hip_stream) {
    if (!ctx) return fail(ICP4R_E_INVALID, "ctx is NULL");
    int rc;
    if ((rc = check_shape(nscans, max_n, mode))) return rc;
    if (nscans == 0) return ICP4R_OK;
    if (!xyzi || !off || !cnt || !clouds || !pair_off || !pair_n) return fail(ICP4R_E_INVALID, "NULL device array");
    if (mode == ICP4R_GATE_STATIC && !mask) return fail(ICP4R_E_INVALID, "ICP4R_GATE_STATIC needs a mask");
    if (((uintptr_t)xyzi | (uintptr_t)clouds) & 15) return fail(ICP4R_E_INVALID, "xyzi / clouds not 16-B aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    return run_gate(ctx, reinterpret_cast<const float4*>(xyzi), off, cnt, mask, nscans, max_n, mode,
                    reinterpret_cast<float4*>(clouds), pair_off, pair_n, nullptr, nullptr, st);
}

int icp4r_static_clouds_batch_device(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt,
                                     int32_t nscans, int32_t max_n, const icp4r_ego_params* ego_params, int32_t mode,
                                     icp4r_ego_result* ego_results, uint8_t* static_mask, float* clouds,
                                     int64_t* pair_off, int32_t* pair_n, void* hip_stream) {
    if (!ctx || !ego_results) return fail(ICP4R_E_INVALID, "ctx / ego_results is NULL");
    int rc;
    if ((rc = check_shape(nscans, max_n, mode)) || (rc = check_ego_params(ego_params))) return rc;
    if (nscans == 0) return ICP4R_OK;
    if (!records || !off || !cnt || !clouds || !pair_off || !pair_n) return fail(ICP4R_E_INVALID, "NULL device array");
    if ((uintptr_t)clouds & 15) return fail(ICP4R_E_INVALID, "clouds not 16-B aligned");
    icp4r_ego_params p;
    icp4r_ego_params_default(&p);
    if (ego_params) p = *ego_params;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    return run_static(ctx, records, off, cnt, nscans, max_n, (int64_t)nscans * (max_n > 0 ? max_n : 1), p, mode,
                      ego_results, static_mask, reinterpret_cast<float4*>(clouds), pair_off, pair_n, st);
}

int icp4r_static_cloud(icp4r_ctx* ctx, const float* records, int32_t n, const icp4r_ego_params* ego_params,
                       icp4r_ego_result* ego_result, float* xyzi_out, int32_t* n_static) {
    if (!ctx || !ego_result || !n_static) return fail(ICP4R_E_INVALID, "NULL argument");
    if (n < 0 || (n > 0 && (!records || !xyzi_out))) return fail(ICP4R_E_INVALID, "bad scan (n = %d)", n);
    int rc;
    if ((rc = check_shape(1, n, ICP4R_GATE_STATIC)) || (rc = check_ego_params(ego_params))) return rc;
    icp4r_ego_params p;
    icp4r_ego_params_default(&p);
    if (ego_params) p = *ego_params;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t zero = 0;
    const size_t cap = (size_t)(n > 0 ? n : 1);
    HIP_TRY(ctx->ego_rec.ensure(cap * 5 * sizeof(float)));
    HIP_TRY(ctx->ego_off.ensure(sizeof(int64_t)));
    HIP_TRY(ctx->ego_cnt.ensure(sizeof(int32_t)));
    HIP_TRY(ctx->ego_res.ensure(sizeof(icp4r_ego_result)));
    HIP_TRY(ctx->gate_clouds.ensure(cap * sizeof(float4)));
    HIP_TRY(ctx->gate_pair_off.ensure(2 * sizeof(int64_t)));
    HIP_TRY(ctx->gate_pair_n.ensure(2 * sizeof(int32_t)));
    if (n > 0) HIP_TRY(hipMemcpyAsync(ctx->ego_rec.p, records, (size_t)n * 5 * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->ego_off.p, &zero, sizeof(zero), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->ego_cnt.p, &n, sizeof(n), hipMemcpyHostToDevice, st));
    if ((rc = run_static(ctx, static_cast<const float*>(ctx->ego_rec.p), static_cast<const int64_t*>(ctx->ego_off.p),
                         static_cast<const int32_t*>(ctx->ego_cnt.p), 1, n, (int64_t)cap, p, ICP4R_GATE_STATIC,
                         static_cast<icp4r_ego_result*>(ctx->ego_res.p), nullptr, static_cast<float4*>(ctx->gate_clouds.p),
                         static_cast<int64_t*>(ctx->gate_pair_off.p), static_cast<int32_t*>(ctx->gate_pair_n.p), st)))
        return rc;
    int32_t pn[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(ego_result, ctx->ego_res.p, sizeof(*ego_result), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pn, ctx->gate_pair_n.p, sizeof(pn), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_static = pn[1];
    if (pn[1] > 0) {
        HIP_TRY(hipMemcpyAsync(xyzi_out, ctx->gate_clouds.p, (size_t)pn[1] * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (n == 0) return fail(ICP4R_E_EMPTY, "empty scan");
    return ICP4R_OK;
}

int icp4r_sequence_pairs(const int32_t* counts, int32_t nscans, int32_t* src_first, int32_t* src_last,
                         int32_t* tgt_first, int32_t* tgt_last, int32_t* registered) {
    if (nscans < 0 || (nscans > 0 && !counts)) return fail(ICP4R_E_INVALID, "bad counts (nscans = %d)", nscans);
    const int32_t bad = icp4r_gate::sequence_pairs(counts, nscans, src_first, src_last, tgt_first, tgt_last, registered);
    if (bad >= 0) return fail(ICP4R_E_INVALID, "scan %d: count %d", bad, counts[bad]);
    return ICP4R_OK;
}

int icp4r_register_static_sequence_ex(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt,
                                      int32_t nscans, const icp4r_ego_params* ego_params,
                                      const icp4r_params* icp_params, int32_t mode, int32_t pairing,
                                      icp4r_ego_result* ego_results, icp4r_result* icp_results,
                                      int32_t* registered, uint8_t* static_mask_out, float* clouds_out,
                                      int32_t* pair_n_out) {
    if (!ctx || !ego_results || !icp_results || !registered) return fail(ICP4R_E_INVALID, "NULL argument");
    if (pairing != ICP4R_PAIR_NODE && pairing != ICP4R_PAIR_STRICT) return fail(ICP4R_E_INVALID, "pairing %d", pairing);
    if (nscans < 0) return fail(ICP4R_E_INVALID, "nscans = %d", nscans);
    if (nscans == 0) return ICP4R_OK;
    if (!off || !cnt) return fail(ICP4R_E_INVALID, "NULL offset/count array");
    int32_t max_n = 0;
    int64_t extent = 0;
    for (int32_t s = 0; s < nscans; ++s) {
        if (cnt[s] < 0 || off[s] < 0) return fail(ICP4R_E_INVALID, "scan %d: negative offset/count", s);
        max_n = std::max(max_n, cnt[s]);
        if (cnt[s] > 0) extent = std::max<int64_t>(extent, off[s] + cnt[s]);
    }
    if (extent > 0 && !records) return fail(ICP4R_E_INVALID, "NULL records");
    int rc;
    if ((rc = check_shape(nscans, max_n, mode)) || (rc = check_ego_params(ego_params))) return rc;
    icp4r_ego_params p;
    icp4r_ego_params_default(&p);
    if (ego_params) p = *ego_params;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t cap = (size_t)(extent > 0 ? extent : 1), ns = (size_t)nscans;
    HIP_TRY(ctx->ego_rec.ensure(cap * 5 * sizeof(float)));
    HIP_TRY(ctx->ego_off.ensure(ns * sizeof(int64_t)));
    HIP_TRY(ctx->ego_cnt.ensure(ns * sizeof(int32_t)));
    HIP_TRY(ctx->ego_res.ensure(ns * sizeof(icp4r_ego_result)));
    HIP_TRY(ctx->gate_mask.ensure(cap));
    HIP_TRY(ctx->gate_clouds.ensure(cap * sizeof(float4)));
    HIP_TRY(ctx->gate_pair_off.ensure((ns + 1) * sizeof(int64_t)));
    HIP_TRY(ctx->gate_pair_n.ensure((ns + 1) * sizeof(int32_t)));
    HIP_TRY(ctx->results.ensure(ns * sizeof(icp4r_result)));
    // one upload
    if (extent > 0) HIP_TRY(hipMemcpyAsync(ctx->ego_rec.p, records, (size_t)extent * 5 * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->ego_off.p, off, ns * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->ego_cnt.p, cnt, ns * sizeof(int32_t), hipMemcpyHostToDevice, st));
    // ego velocity and the gate
    uint8_t* d_mask = static_cast<uint8_t*>(ctx->gate_mask.p);
    float* d_clouds = static_cast<float*>(ctx->gate_clouds.p);
    int64_t* d_poff = static_cast<int64_t*>(ctx->gate_pair_off.p);
    int32_t* d_pn = static_cast<int32_t*>(ctx->gate_pair_n.p);
    icp4r_result* d_res = static_cast<icp4r_result*>(ctx->results.p);
    if ((rc = run_static(ctx, static_cast<const float*>(ctx->ego_rec.p), static_cast<const int64_t*>(ctx->ego_off.p),
                         static_cast<const int32_t*>(ctx->ego_cnt.p), nscans, max_n, (int64_t)cap, p, mode,
                         static_cast<icp4r_ego_result*>(ctx->ego_res.p), d_mask, reinterpret_cast<float4*>(d_clouds),
                         d_poff, d_pn, st)))
        return rc;
    std::vector<int32_t> pn(ns + 1);
    icp4r_batch b;
    memset(&b, 0, sizeof(b));
    b.src = d_clouds;
    b.tgt = d_clouds;
    std::vector<int32_t> frames;  // ICP4R_PAIR_NODE: the registered frames, in order
    if (pairing == ICP4R_PAIR_STRICT) {
        // frame k = scan k against scan k - 1: the descriptors shifted by one, nothing read back
        b.src_off = d_poff + 1;
        b.src_n = d_pn + 1;
        b.tgt_off = d_poff;
        b.tgt_n = d_pn;
        b.npairs = nscans;
        b.max_src_n = b.max_tgt_n = max_n;
        if ((rc = icp4r_align_batch_device(ctx, &b, icp_params, d_res, st))) return rc;
        HIP_TRY(hipMemcpyAsync(icp_results, d_res, ns * sizeof(icp4r_result), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pn.data(), d_pn, (ns + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else {
        // the node's running clouds: one read-back of the counts, the pairs on the host
        HIP_TRY(hipMemcpyAsync(pn.data(), d_pn, (ns + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<int32_t> sf(ns), sl(ns), tf(ns), tl(ns);
        if ((rc = icp4r_sequence_pairs(pn.data() + 1, nscans, sf.data(), sl.data(), tf.data(), tl.data(), registered)))
            return rc;
        std::vector<int64_t> poff(ns + 1, 0);  // first packed point of scan s (the layout is tight)
        for (size_t s = 0; s < ns; ++s) poff[s + 1] = poff[s] + pn[s + 1];
        std::vector<int64_t> so, to;
        std::vector<int32_t> sn, tn;
        for (int32_t k = 0; k < nscans; ++k) {
            if (!registered[k]) continue;
            frames.push_back(k);
            so.push_back(poff[(size_t)sf[k]]);
            sn.push_back((int32_t)(poff[(size_t)sl[k] + 1] - poff[(size_t)sf[k]]));
            to.push_back(poff[(size_t)tf[k]]);
            tn.push_back((int32_t)(poff[(size_t)tl[k] + 1] - poff[(size_t)tf[k]]));
            b.max_src_n = std::max(b.max_src_n, sn.back());
            b.max_tgt_n = std::max(b.max_tgt_n, tn.back());
        }
        const size_t R = frames.size();
        if (R > 0) {
            HIP_TRY(ctx->src_off.ensure(R * sizeof(int64_t)));
            HIP_TRY(ctx->tgt_off.ensure(R * sizeof(int64_t)));
            HIP_TRY(ctx->src_n.ensure(R * sizeof(int32_t)));
            HIP_TRY(ctx->tgt_n.ensure(R * sizeof(int32_t)));
            HIP_TRY(hipMemcpyAsync(ctx->src_off.p, so.data(), R * sizeof(int64_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->tgt_off.p, to.data(), R * sizeof(int64_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->src_n.p, sn.data(), R * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->tgt_n.p, tn.data(), R * sizeof(int32_t), hipMemcpyHostToDevice, st));
            b.src_off = static_cast<const int64_t*>(ctx->src_off.p);
            b.tgt_off = static_cast<const int64_t*>(ctx->tgt_off.p);
            b.src_n = static_cast<const int32_t*>(ctx->src_n.p);
            b.tgt_n = static_cast<const int32_t*>(ctx->tgt_n.p);
            b.npairs = (int32_t)R;
            if ((rc = icp4r_align_batch_device(ctx, &b, icp_params, d_res, st))) return rc;
        }
    }
    // one download
    std::vector<icp4r_result> packed(frames.size());
    if (!frames.empty())
        HIP_TRY(hipMemcpyAsync(packed.data(), d_res, frames.size() * sizeof(icp4r_result), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ego_results, ctx->ego_res.p, ns * sizeof(icp4r_ego_result), hipMemcpyDeviceToHost, st));
    if (static_mask_out && extent > 0)
        HIP_TRY(hipMemcpyAsync(static_mask_out, d_mask, (size_t)extent, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int64_t total = 0;
    for (size_t s = 0; s < ns; ++s) total += pn[s + 1];
    if (clouds_out && total > 0) {
        HIP_TRY(hipMemcpyAsync(clouds_out, d_clouds, (size_t)total * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (pair_n_out) memcpy(pair_n_out, pn.data(), (ns + 1) * sizeof(int32_t));
    if (pairing == ICP4R_PAIR_STRICT) {
        for (int32_t k = 0; k < nscans; ++k) registered[k] = pn[(size_t)k + 1] > 0 && pn[(size_t)k] > 0;
    } else {
        for (int32_t k = 0; k < nscans; ++k) {
            memset(&icp_results[k], 0, sizeof(icp4r_result));
            icp_results[k].status = ICP4R_E_EMPTY;
        }
        for (size_t q = 0; q < frames.size(); ++q) icp_results[frames[q]] = packed[q];
    }
    return ICP4R_OK;
}

int icp4r_register_static_sequence(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt,
                                   int32_t nscans, const icp4r_ego_params* ego_params,
                                   const icp4r_params* icp_params, int32_t mode, int32_t pairing,
                                   icp4r_ego_result* ego_results, icp4r_result* icp_results, int32_t* registered) {
    return icp4r_register_static_sequence_ex(ctx, records, off, cnt, nscans, ego_params, icp_params, mode, pairing,
                                             ego_results, icp_results, registered, nullptr, nullptr, nullptr);
}

}  // extern "C"
