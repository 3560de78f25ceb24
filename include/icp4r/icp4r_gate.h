/*
 * icp4r_gate.h — C ABI of Doppler-gated registration: ICP over each scan's static points only, the
 * reference node built with USE_STATIC_POINTS.
 *
 * Replaces, in src/iterative_closest_point.cpp of the reference:
 *
 *     #ifdef USE_STATIC_POINTS
 *         cloud_src_in->push_back(static_point_src_cloud ...)          // :404-406 instead of :425-427
 *         cloud_tar_in->push_back(static_point_tar_cloud ...)          // :482-484 instead of :488-493
 *     #endif
 *     if (cloud_tar_in->size() && cloud_src_in->size()) { icp ... ; clear both }   // :505, :698-699
 *
 * The ego-velocity kernels (icp4r_ego.h) leave a static mask per point; a stable, batched stream
 * compaction (icp4r_gate.hip) packs every scan's static points tightly, in input order, and
 * icp4r_align_batch_device registers the packed clouds — all in HBM, on one stream.
 *
 * Packed layout.  clouds: float4 (x, y, z, intensity), the kept points of scan 0, then scan 1, ...;
 * pair_n[nscans + 1] (int32) and pair_off[nscans + 1] (int64) hold each scan's kept count and first
 * point PRECEDED BY ONE DUPLICATE OF SCAN 0's ENTRY: [s0, s0, s1, ..., s(nscans-1)].  The node pairs
 * frame k = scan k against scan k-1, and frame 0 = scan 0 against itself (:306-315), so
 *
 *     src_off = pair_off + 1, src_n = pair_n + 1, tgt_off = pair_off, tgt_n = pair_n
 *
 * are the nscans pairs of an icp4r_batch whose src and tgt both point at `clouds`.
 *
 * Semantics follow the reference with the three departures icp4r_ego.h lists (reproducible hypothesis
 * draws, the draw in [0, n), n an int) and a fourth: the node re-runs fitSineRansac on the PREVIOUS
 * scan in every frame (:467) from a fresh std::random_device, so a scan is split twice, with two
 * different random models.  Here each scan has ONE mask, drawn with its own seed (seed + (s << 32)),
 * used both when the scan is the source and when it is the target: half the RANSAC work, and a run is
 * reproducible.
 *
 * A point is static iff !(delta > dynamic_threshold) — the node's else branch — so a NaN delta is
 * static: non-finite points reach ICP and get its ICP4R_E_NONFINITE.
 *
 * Conventions as icp4r.h: int status returns, icp4r_last_error(), one context per host thread.
 */
#ifndef ICP4R_GATE_H
#define ICP4R_GATE_H

#include <stdint.h>

#include "icp4r.h"
#include "icp4r_ego.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum icp4r_gate_mode {
    ICP4R_GATE_STATIC = 0, /* keep the points whose mask byte is non-zero (USE_STATIC_POINTS)      */
    ICP4R_GATE_ALL = 1     /* keep every point (USE_STATIC_POINTS undefined); same layout          */
} icp4r_gate_mode;

typedef enum icp4r_pairing {
    ICP4R_PAIR_NODE = 0,  /* the node's running clouds (icp4r_sequence_pairs)                      */
    ICP4R_PAIR_STRICT = 1 /* frame k = scan k against scan k-1, whatever is empty                  */
} icp4r_pairing;

/* The compaction alone, on a caller's mask; device-resident, asynchronous on hip_stream (NULL = the
 * context's stream).  xyzi: device float4 per point, 16-B aligned, indexed like the mask: point i of
 * scan s at off[s] + i; off / cnt: device[nscans]; mask: device, one byte per point (ignored with
 * ICP4R_GATE_ALL, may be NULL then); max_n: host-known upper bound of cnt[].  A scan with
 * cnt[s] > max_n (or < 0) gets count 0 and its mask is not read.  clouds: device, room for the sum
 * of the counts; pair_off: device int64[nscans + 1]; pair_n: device int32[nscans + 1]. */
int icp4r_compact_by_mask_batch_device(icp4r_ctx* ctx, const float* xyzi, const int64_t* off, const int32_t* cnt,
                                       const uint8_t* mask, int32_t nscans, int32_t max_n, int32_t mode,
                                       float* clouds, int64_t* pair_off, int32_t* pair_n, void* hip_stream);

/* Ego velocity (as icp4r_ego_velocity_batch_device: scan s uses the seed ego_params->seed + (s << 32))
 * then the gate, on one stream, with no host round trip.  records / off / cnt / max_n / ego_results as
 * there; static_mask: device, one byte per record, or NULL (the context keeps it).  The scans must lie
 * within the first nscans * max_n records of `records` (any layout without gaps does); a scan that
 * does not is not touched: its count is 0 and its ego status ICP4R_E_INVALID. */
int icp4r_static_clouds_batch_device(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt,
                                     int32_t nscans, int32_t max_n, const icp4r_ego_params* ego_params, int32_t mode,
                                     icp4r_ego_result* ego_results, uint8_t* static_mask, float* clouds,
                                     int64_t* pair_off, int32_t* pair_n, void* hip_stream);

/* One scan, host buffers, synchronous: its ego velocity and its static points (xyzi_out: room for
 * n x 4 floats; *n_static of them are written, in input order). */
int icp4r_static_cloud(icp4r_ctx* ctx, const float* records, int32_t n, const icp4r_ego_params* ego_params,
                       icp4r_ego_result* ego_result, float* xyzi_out, int32_t* n_static);

/* Pure host, no device: the node's running-cloud rule (:505 vs :698-699).  Frame k appends scan k to
 * the source cloud and scan k-1 (scan 0 for k = 0) to the target cloud; the frame is registered iff
 * both clouds then hold a point, and only a registered frame clears them.  counts[nscans]: points per
 * scan (>= 0).  Frame k's clouds are the contiguous scan ranges [src_first[k], src_last[k]] and
 * [tgt_first[k], tgt_last[k]] (inclusive; written for skipped frames too: what has accumulated);
 * registered[k]: 1 or 0.  Any output may be NULL.  In the packed layout a range of scans [a, b] is
 * the one cloud (pair_off[1 + a], pair_n[1 + a] + ... + pair_n[1 + b]).  A registered target holds at
 * most one non-empty scan and a registered source at most two: max_tgt_n = max_n and
 * max_src_n = 2 max_n bound every pair. */
int icp4r_sequence_pairs(const int32_t* counts, int32_t nscans, int32_t* src_first, int32_t* src_last,
                         int32_t* tgt_first, int32_t* tgt_last, int32_t* registered);

/* The one-call form, host buffers, synchronous: one upload of the records (5 floats each; scan s =
 * records off[s] .. off[s] + cnt[s]), ego velocity and gate on the device, the pairs, one batched
 * ICP, one download.  ICP4R_PAIR_NODE reads the nscans counts back, runs icp4r_sequence_pairs on them
 * and uploads the descriptors; ICP4R_PAIR_STRICT uses the shifted views with no read-back, and an
 * empty cloud gives that frame the batch's own status (ICP4R_E_EMPTY: empty target,
 * ICP4R_E_TOO_FEW_CORR: empty source).  ego_results[nscans], icp_results[nscans] (frame k at k; a
 * skipped frame's row is zero with status ICP4R_E_EMPTY), registered[nscans] (0: a frame the node
 * skips). */
int icp4r_register_static_sequence(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt,
                                   int32_t nscans, const icp4r_ego_params* ego_params,
                                   const icp4r_params* icp_params, int32_t mode, int32_t pairing,
                                   icp4r_ego_result* ego_results, icp4r_result* icp_results, int32_t* registered);

/* icp4r_register_static_sequence, which also hands back what it packed (each optional): the mask
 * (one byte per record, indexed like records), the packed clouds (room for 4 floats per record) and
 * pair_n (int32[nscans + 1]). */
int icp4r_register_static_sequence_ex(icp4r_ctx* ctx, const float* records, const int64_t* off, const int32_t* cnt,
                                      int32_t nscans, const icp4r_ego_params* ego_params,
                                      const icp4r_params* icp_params, int32_t mode, int32_t pairing,
                                      icp4r_ego_result* ego_results, icp4r_result* icp_results,
                                      int32_t* registered, uint8_t* static_mask_out, float* clouds_out,
                                      int32_t* pair_n_out);

#ifdef __cplusplus
}
#endif

#endif /* ICP4R_GATE_H */
