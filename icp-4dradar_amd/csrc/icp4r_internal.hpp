// icp4r_internal.hpp — types shared by the C-ABI host code and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp4r/icp4r.h"
#include "icp4r/icp4r_ego.h"
#include "icp4r/icp4r_gicp.h"
#include "icp4r_math.hpp"

namespace icp4r {

constexpr int kNNWG = 256;        // threads per NN workgroup (4 waves)
constexpr int kMaxQ = 16;         // register-resident queries per lane in nn_kernel (instantiated)
constexpr int kDefaultQ = 4;      // brute force: default cap (tools/tune_sweep.py)
constexpr int kDefaultPrunedQ = 2;  // pruned: default cap
constexpr int kDefaultLeaf = 16;    // pruned: targets per block
constexpr int kMaxGroups = 3;        // batched plans: pair groups on their own streams (run_pairs)
constexpr int kDefaultGroups = 2;
constexpr int kDefaultStageSel = 32;    // batched search: plan option stage_sel's default
constexpr int kDefaultPartSize = 2048;  // batched search: misses per work item of a heavy pair (round 6: 1024 -> 2048, C3 +0.6 %)
constexpr int kFoldChunk = 1024;  // points per LDS chunk of the sequential fitness fold
constexpr int kSuper = 8;         // target blocks per superblock (pruned NN)
constexpr int kPrunedMinM = 512;  // ICP4R_NN_AUTO prunes when the largest target has >= this many points
constexpr int kCacheMaxN = 16384; // cached-neighbour test (nn_lds_kernel<true>): max source points per pair
// Work counters: one 128-B slot per wave (mod kCountSlots).  A single counter word hit by every wave
// of a launch serialises the atomics at one L2 channel (~10 ns each: 30k waves = 0.3 ms per launch).
constexpr int kKdNodes = 2048;                 // kd tree nodes kept per target (heap ids < this)
constexpr int kKdnStride = 8 + kKdNodes;
constexpr int kCountSlots = 2048;
constexpr int kCountStride = 16;

constexpr int kNumericsPCL = ICP4R_NUMERICS_PCL;
constexpr int kNumericsF64 = ICP4R_NUMERICS_F64;
constexpr int kStatusEmpty = ICP4R_E_EMPTY;
constexpr int kStatusTooFewCorr = ICP4R_E_TOO_FEW_CORR;
constexpr int kStatusNonFinite = ICP4R_E_NONFINITE;
constexpr int kStatusInvalid = ICP4R_E_INVALID;

// per-pair loop phase
constexpr int kPhaseActive = 0;     // iterating
constexpr int kPhaseConverged = 1;  // hasConverged() fired
constexpr int kPhaseFailed = 2;     // |C| < min_correspondences (PCL: converged_ = false, break)
constexpr int kPhaseInvalid = 3;    // empty target / non-finite input: nothing computed

using Result = icp4r_result;

struct KParams {
    ConvParams conv;
    int32_t min_corr;
    int32_t numerics;
    int32_t compute_fitness;
    float max_d2;          // reject a correspondence iff d2 > max_d2 (float image of max_dist^2)
    double huber_delta;    // +inf: unweighted (PCL)
    double fit_max_range;  // getFitnessScore(max_range): keep d2 <= max_range
    int32_t need_mse;      // 0 when no MSE criterion can fire (both thresholds <= 0): the MSE only
                           // feeds those two '<' tests, so its sequential sum is skipped
    int32_t sigma_max_kc;  // Eigen's largest GEMM panel depth for sigma (sigma_max_kc(); INT32_MAX:
                           // no panels) — the panel depth of |C| correspondences is sigma_kc()
};

struct PairArgs {
    const float4* src;
    const float4* tgt;
    const int64_t* src_off;
    const int32_t* src_n;
    const int64_t* tgt_off;
    const int32_t* tgt_n;
    const float* guess;  // npairs*16 column-major or nullptr
    float4* aligned;     // optional
    Result* results;
    KParams kp;
};

// Device-resident per-pair loop state (ICP members of PCL: transformation_, final_transformation_,
// nr_iterations_, converged_, and DefaultConvergenceCriteria's prev MSE / similar counter).
struct PairState {
    float T_inc[16];
    float final_T[16];
    double prev_mse;
    int32_t similar;
    int32_t conv_state;
    int32_t iterations;
    int32_t phase;
    int32_t status;
    int32_t ncorr;
    // Σs of the next update's pass A (Eigen's rowwise().sum() of the moved source, in index order),
    // folded by the previous update's fused tail over the X it wrote (fold_update_kernel: eligible
    // registrations only — every correspondence kept, unweighted, no MSE criterion); sums_ok = 1 while
    // they are valid for the next pass A, which then reads nn_t only
    float sum_s[3];
    int32_t sums_ok;
    // Lazy source cloud (WorkArgs::lazy_x): a silent tail tested the pair at T_pend * X without storing
    // the moved points or their bounds; pending = 1 until the next tail (or the pair's last update)
    // stores them.  While pending, a point whose stored L (X.w) has its sign bit set was re-written by
    // the search in between and is at the newer state already; every other point's stored (X, L, U) is
    // the consistent triple of the older state.
    float T_pend[16];
    int32_t pending;
};

// NN result of one query: (float bits of d² << 32) | target index.  d² >= 0, so the unsigned order
// of the keys is the lexicographic (d², index) order; the minimum key is PCL's answer (nearest
// target, lowest index among equal distances) whatever order the targets are visited in.
using NNKey = uint64_t;
__host__ __device__ inline float key_d2(NNKey k) {
    union {
        uint32_t u;
        float f;
    } c;
    c.u = (uint32_t)(k >> 32);
    return c.f;
}
__host__ __device__ inline int32_t key_idx(NNKey k) { return (int32_t)(uint32_t)k; }

// Workspace, pair p at [p * stride, ...) of each array.
struct WorkArgs {
    float4* X;          // input_transformed [npairs * x_stride]
    NNKey* nn_key;      // per-query NN key   [npairs * x_stride]; splits > 1 merge by atomicMin.  After
                        // a fused fitness pass (pair_cache_test, fitness) a HIT's index bits hold its NN's
                        // SORTED target position, not the original index: only key_d2 is meaningful
                        // there (finish_kernel reads d² only; nothing may read key_idx after that pass)
    PairState* state;   // [npairs]
    int64_t x_stride;   // >= max source points per pair
    int32_t splits;     // brute force: target splits per pair (1 for batches; >1 for single-pair latency)
    int32_t leaf;       // pruned: targets per block (16 or 32); 0 = brute force
    int32_t kd_index;   // clouds of <= 8192 points get the balanced kd order (index_kernel), else Morton;
                        // bit 0: targets, bit 1: sources
    int32_t src_by_tgt; // 1: a source whose target gets the kd order is ordered by descending the target's
                        // kd tree (src_order_kernel) instead of by its own tree: queries sorted by the
                        // target leaf they fall in, and that leaf seeds their first search
    int32_t stage_first;  // 1 (batched plan): src_order_kernel writes the first pass' query records
    int32_t seed_next;    // 1 (multi-tile plan, PCL numerics): the update's transform and fitness_prep_kernel
                          // write the next NN pass's seed keys (the previous NN at the moved point) from the
                          // correspondence records, so no nn_seed_kernel launch
                          // (qv / qm, sorted order) itself; 0: the first pass' nn_key seeds
    float* tbb;         // [npairs * 8] the target's bounding box (lo xyz, hi xyz), from init_kernel's
                        // validation pass (the Morton index skips its own pass over the cloud); or nullptr
    uint16_t* mo_hist;  // [npairs * mo_groups * 2^14] per-workgroup Morton cell counts (u16) of a large target
                        // (multi-workgroup sort, index_mo_hist_kernel); nullptr: one workgroup per target
    int32_t mo_groups;  // workgroups per target of that sort (>= t_stride / 8192)
    int32_t* mo_rep;    // [npairs * 2^14] per Morton cell: the original index of one of its targets, -1: empty
                        // (written by that sort; nn_seed_kernel's first-pass seed: a target in the query's cell)
    uint32_t* kdn;      // [npairs * kKdnStride] the target kd tree: [0, 6) quantisation lo / scale bits,
                        // [8 + node] internal node (heap order) = 1 << 31 | mid << 13 | axis << 11 | key
    // Pruned-search index, built once per registration by index_kernel (SURVEY.md §8f "sorted map"):
    float4* tsort;      // [npairs * t_stride] targets in index order (kd / Morton), .w = original index bits;
                        // positions [m, t_stride): +inf coordinates (never a match)
    int32_t* tinv;      // [npairs * t_stride] original target index -> sorted position
    float4* tbox;       // [npairs * 2 * b_stride] per block: lo, hi (empty blocks: +inf, -inf)
    float4* sbox;       // [npairs * 2 * sb_stride] per superblock of kSuper blocks: lo, hi
    int32_t* sperm;     // [npairs * x_stride] source indices in index order (kd / Morton)
    int64_t t_stride, b_stride, sb_stride;
    float4* corr;       // PCL numerics: [npairs * x_stride * 2] per source point {s.xyz, w}, {d.xyz, d²}
    // Cached-neighbour test (nn_lds_kernel<true>; nullptr = off):
    // L_i (X_i.w): a lower bound on |X_i - t_k| for every target k other than the NN; U_i (nn_u[i]):
    // an upper bound of the second-nearest distance.  Set by a search, widened by every kernel that
    // moves X_i.
    float* nn_u;        // [npairs * x_stride] U_i
    int32_t tile_own;     // 1 (one-tile plan): nn_tile_kernel seeds, searches and writes the records itself
                          // (plan option tile_own = 0: the three-launch form, for A/B)
    int32_t defer_xform;  // 1: the update leaves X_i := T_inc X_i to the next pass's test kernel
    int32_t sums_tail;    // 1: the fused tail also folds the next pass A's Σs (eligible pairs: PairState)
    int32_t fold_keys;    // 1 (multi-tile single pairs, wide update): no corr_kernel after the search — the
                          // update's pass A forms the correspondence records from X and the merged keys'
                          // targets and writes them for pass B
    int32_t res_update;   // 1 (batched plan, sources <= kResMaxN): fold_update_res_kernel, the pair held on
                          // chip across the update (plan option res_update = 0: fold_update_kernel)
    int32_t held_update;  // 1 (wide update, sources <= kHeldMaxN): fold_update_held_kernel, the records held
                          // in the fillers' registers from pass A to pass B (plan option held_update)
    int32_t fit_xform;    // 1 (one-tile plan, no cache, no seeds): the fitness pass' nn_tile_kernel forms
                          // X := final * input itself (fitness_prep_kernel's work; plan option fit_xform)
    int32_t lazy_x;       // 1 (batched plan, fused test, fold_update_kernel): every second fused tail is
                          // silent — it stores neither X nor U; the next update forms T_pend * X itself and
                          // its tail stores two steps at once (PairState::pending; plan option lazy_x)
    float4* nn_t;       // [npairs * x_stride] the NN target of X_i: xyz, .w = its sorted target position |
                        // the query's sorted position << 14 (nt_pack)
    float4* sq;         // [npairs * x_stride] the pass's miss list in the order the test found them: a
                        // missed query's {X.xyz, U} (the test appends, the search stages by rank) ...
    uint2* sm;          // ... {its source index | its NN's sorted target position << 14, its sorted position}
    float4* qv;         // [npairs * x_stride] a search item's queries in list order {x, y, z, U} ...
    uint2* qm;          // ... {source index | sorted position << 14, seed's sorted target position}
    uint32_t* need;     // [npairs * need_stride] per pair: bit s = the query at Morton position s missed
    int64_t need_stride;
    int32_t* miss_cnt;  // [npairs] misses of the current pass (cleared by the update); | kMissUnranked when
                        // the fused test left them unplaced (sq / sm + bitmap) for the search to place
    // Batched search (nn_lds_kernel): the pass's pair work list, heaviest first, and its queue
    int32_t* plist;     // [npairs * ceil(x_stride / 64)] items (pair << 10 | part)
    int32_t* plist_n;   // [4]: items, (queue), the pass's part size (nn_order_kernel)
    int32_t* queue;     // [1] next work-list index (reset by nn_order_kernel)
    int32_t* owork;     // [npairs] the next pass' work per pair, published by fold_update_kernel when it
                        // builds the work list itself (plist_n[3]: its arrival counter)
    int32_t part_size;  // nn_lds_kernel: misses per work item of a heavy pair (0: one item per pair);
                        // plist holds items (pair << 10 | part)
    int32_t stage_sel;  // nn_lds_kernel: a ranked item of at most this many misses stages only the
                        // superblocks its queries can reach (stage_tile_sel; plan option stage_sel, 0: off)
    unsigned long long* evals;  // [kCountSlots][kCountStride]: per slot distance evaluations, box tests,
                                // cached-neighbour hits (count_add; the host sums the slots)
    uint64_t* ticks;    // debug (plan option phase_ticks = 1): s_memrealtime (100 MHz) at fold_update phase
                        // boundaries of pair 0 — start, pass A, pass B, solve, transform
    uint64_t* pass_ticks;  // debug (plan option phase_ticks = 1): this NN pass' own slots [kPassTickSlots] of the
                           // batched search's event counts / clocks (tools/experiments/nn_events.py), or nullptr
};
constexpr int kPassTickSlots = 16;  // per NN pass: 11 event counters / clocks + 4 per-item walls
constexpr int kMaxTickPasses = 64;  // passes with their own slots (later passes: none)
// first per-pass slot of a batch of npairs (after the pair-0 stamps and the per-pair debug slots)
inline int64_t pass_tick_base(int npairs) { return 32 + 20 * (int64_t)npairs; }

// ---- the ICP path (launch_index, launch_index_cloud: icp4r_index.hip; launch_init, launch_fitness_prep,
// launch_finish, launch_rot_f32: icp4r_frame.hip; the others: icp4r_kernels.hip).
// One registration = SURVEY.md §3.2 / Appendix A.  It runs on the
// device as a fixed sequence of launches with no host synchronisation: per-pair phase flags (PairState)
// let a finished pair's workgroups return at once.  run_pairs (icp4r_capi.cpp) picks one of:
//
//   batched (many pairs, targets <= kLdsMaxTargets; up to kMaxGroups pair groups, a stream each)
//     launch_init, launch_index                       validate, X := guess * src; kd / Morton orders, boxes
//     per iteration:
//       launch_nn_lds      [nn_cache_test_kernel] [nn_order_kernel] nn_lds_kernel — the test and the work
//                          list only where the previous update's fused tail did not make them
//       launch_update      fold_update_kernel (or its res form): correspondences -> fold passes A and B ->
//                          3x3 solve -> hasConverged -> the tail: X := T_inc * X, the next pass' test and list
//     launch_fitness_prep, launch_nn_lds(fitness), launch_finish
//
//   pruned / tile (single pairs, small batches, targets of any size; one stream)
//     launch_init, launch_index
//     per iteration:
//       launch_nn_tile     [nn_seed_kernel] nn_tile_kernel [launch_corr] — one tile: the search alone
//         or launch_nn_pruned   [nn_seed_kernel] nn_pruned_kernel<Q, B> [launch_corr]   (plan option nn_tile = 0)
//       launch_update      fold_update_held_kernel / fold_update_wide_kernel (at most one pair per CU), else
//                          fold_update_kernel; F64 numerics: update_f64_kernel
//     [launch_fitness_prep], the search once more (fitness), launch_finish
//     brute force (small targets, ICP4R_NN_BRUTE): launch_nn in the search's place, launch_update with
//     need_corr (launch_corr first), no launch_index
//     launch_corr        corr_kernel: the correspondence records from the merged keys, where the search did
//                        not write them itself — called by launch_nn_tile, launch_nn_pruned and launch_update
//
//   reciprocal registrations (use_reciprocal_correspondences): launch_recip (icp4r_recip.hip) between the
//     search and the update of every iteration, on the batched plan without the cached-neighbour test or
//     the pruned / tile plan without fold_keys and the held update; never solo
//
//   solo (the tile plan's pairs when every target fits one LDS tile; sources <= kSoloMaxN by default)
//     launch_init, launch_index, launch_solo          solo_kernel: every iteration, the fitness pass and the
//                                                     result row of a pair by one workgroup in one launch
//
// nn_kernel and nn_pruned_kernel hold Q queries per lane in VGPRs and stream targets through the scalar
// cache: the target address is wave-uniform, so each target point lands in SGPRs and is broadcast to 64
// lanes x Q queries with no LDS traffic; the batched, tiled and solo searches stage a target tile in LDS
// and evaluate (query, block) work items instead.  Per (query, target) the VALU executes 3 sub + 3 mul +
// 2 add (FLANN's L2_Simple, unfused) and a compare/select.  Every NN result is a u64 key (d² bits, target
// index) whose minimum is PCL's answer (lowest index among ties), so pruning, visiting order and target
// splits cannot change it.  Determinism: fixed-order
// reductions only (xor-butterfly per wave, waves in index order, the PCL-numerics folds sequential in
// source order); no float atomics.
hipError_t launch_init(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st);
hipError_t launch_nn(int q, bool packed, const PairArgs& a, const WorkArgs& w, int npairs, int max_n,
                     int fitness_pass, hipStream_t st);
hipError_t launch_index(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st);
// one cloud's index alone (as pair p's target; w's index buffers), no source column or order
hipError_t launch_index_cloud(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st);
// chunk_sb: superblocks per target chunk (<= 64); chunks: grid.z (1: one wave searches every superblock)
hipError_t launch_nn_pruned(int q, int chunk_sb, int chunks, const PairArgs& a, const WorkArgs& w, int npairs,
                            int max_n, int fitness_pass, int first, hipStream_t st);
// the pruned plan's LDS-tiled search: nn_seed_kernel, nn_tile_kernel (target tiles x query parts),
// launch_corr (records, when the update reads them)
hipError_t launch_nn_tile(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, int max_m, int fitness_pass,
                          int first, int qrun, hipStream_t st, hipEvent_t tile_start = nullptr, hipEvent_t tile_stop = nullptr);
// corr_kernel, its one launch: every active pair's correspondence records from its merged keys
hipError_t launch_corr(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, hipStream_t st);
// events recorded around the batched NN's stages (any may be null)
struct NNLdsEvents {
    hipEvent_t test_start = nullptr, test_stop = nullptr, search_start = nullptr, search_stop = nullptr;
};
// ordered: the previous fold_update_kernel built the work list (no nn_order_kernel launch)
// pending: the pass follows a silent tail (WorkArgs::lazy_x) — a searched point is stored whole, its L flagged
hipError_t launch_nn_lds(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, int fitness_pass, int first,
                         int ncu, hipStream_t st, const NNLdsEvents& ev, int test_fused = 0, int ordered = 0,
                         int pending = 0);
constexpr int kLdsMaxTargets = 8192;  // nn_lds_kernel: whole target set in LDS
constexpr int kLdsMinPairs = 256;     // ... used for batches of at least this many pairs
constexpr int kLdsMaxSources = 1 << 14;  // ... with at most this many sources (14-bit index / position fields)
constexpr int kResMaxN = 8192;            // fold_update_res_kernel: sources of at most this many points
constexpr int kDefaultResUpdate = 0;      // ... plan option res_update's default
constexpr int kDefaultLazyX = 1;          // fold_update_kernel: plan option lazy_x's default
constexpr int kHeldMaxN = 10 * 896;       // fold_update_held_kernel: sources of at most this many points
constexpr int kHeldSmallN = 3 * 704;      // ... its 3-record form (the 2k scans; 11 filler waves) up to this many
constexpr int kDefaultHeldUpdate = 1;     // ... plan option held_update's default
constexpr int kSoloMaxN = 1024;           // solo_kernel by default for single pairs of at most this many sources
// wide: one 1024-thread workgroup per pair (fold_update_wide_kernel) — plans with at most one pair
// per CU and neither the fused test nor the fused work list
hipError_t launch_update(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, bool need_corr,
                         hipStream_t st, int tail_test = 0,
                         int order_ncu = 0,  // > 0: the launch also builds the next pass's work list
                         bool wide = false,
                         int silent = 0,     // 1 (WorkArgs::lazy_x): the fused tail stores neither X nor U
                         int pending = 0);   // 1 (WorkArgs::lazy_x): the previous launch's tail was silent
// solo_kernel: every iteration and the fitness pass of each pair in one workgroup (PCL numerics,
// targets <= kLdsMaxTargets, sources <= kCacheMaxN; after launch_init and launch_index)
hipError_t launch_solo(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, int iters, hipStream_t st);
hipError_t launch_fitness_prep(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st, int test = 0);
hipError_t launch_finish(const PairArgs& a, const WorkArgs& w, int npairs, hipStream_t st);
hipError_t launch_rot_f32(const float* sigma, float* R, int k, hipStream_t st);

// ---- reciprocal correspondences (icp4r_recip.hip; icp4r_params.use_reciprocal_correspondences)
// The stage's own workspace, pair p at [p * stride, ...) of each array (run_pairs offsets a pair group's view).
constexpr int kRecipLeaf = 64;  // sources per block of the reverse search (one wave's box)
struct RecipArgs {
    NNKey* win;        // [npairs * 2 * w_stride] per target: the smallest (d², source index) key that chose it,
                       // two buffers taken in turn by parity (the vote clears the other one)
    float4* rsrc;      // [npairs * s_stride] the moved source in index order (sperm), .w = original index bits
    float4* rbox;      // [npairs * 2 * b_stride] per block of kRecipLeaf sorted sources: lo, hi
    int64_t w_stride;  // >= max target points per pair
    int64_t s_stride;  // max source points per pair rounded up to whole workgroups (256)
    int64_t b_stride;  // s_stride / kRecipLeaf
};
// One iteration's reciprocal stage for every active pair, after the search and before the update: a
// source whose nearest target has a nearer source (key order) gets d² = +inf in its key and record.
// parity: the iteration's winner buffer (0 / 1 in turn; both all-ones before the first iteration).
hipError_t launch_recip(const PairArgs& a, const WorkArgs& w, const RecipArgs& r, int npairs, int max_n, int parity,
                        hipStream_t st);

// ---- scan-to-map store (icp4r_map.hip)
struct SectorArgs {
    float cx, cy, cz;  // query point (the vehicle position p_now)
    float radius;      // RADAR_RADIUS
    float heading;     // degrees (float, as Sector_Search receives it)
};
struct Mat3x4d {
    double R[9];  // row-major
    double t[3];
};
hipError_t launch_associate(const float4* in, int64_t n, const Mat3x4d& M, float4* out, hipStream_t st);
int64_t sector_blocks(int64_t n);
// The searches and the delete are one stable compaction (count per block, scan, ordered write) with
// the keep test as a parameter; counts / offsets hold sector_blocks(n) entries, out every kept point.
hipError_t launch_sector(const float4* map, int64_t n, const SectorArgs& a, int32_t* counts, int32_t* offsets,
                         int32_t* total, float4* out, hipStream_t st);
struct BoxArgs {
    float lo[3], hi[3];  // min <= p && max > p
};
hipError_t launch_box(const float4* map, int64_t n, const BoxArgs& b, int32_t* counts, int32_t* offsets,
                      int32_t* total, float4* out, hipStream_t st);
hipError_t launch_radius(const float4* map, int64_t n, const float* c, float radius, int32_t* counts,
                         int32_t* offsets, int32_t* total, float4* out, hipStream_t st);
// keeps the points in none of the nb boxes (device, nb x 6)
hipError_t launch_outside_boxes(const float4* map, int64_t n, const float* d_boxes, int32_t nb, int32_t* counts,
                                int32_t* offsets, int32_t* total, float4* out, hipStream_t st);
// Downsampled insert of na arrivals into n0 stored points (n0 + na < 2^31): the new store to out (room
// for n0 + na points), its size to *total, the reference's counter to **counter (in the scratch).
// scratch: ds_layout(n0, na).bytes; counts / offsets: sector_blocks(n0 + na) entries.
struct DsLayout {
    size_t smin, rep, scount, swin, pairs_a, pairs_b, sslot, akeep, rcounts, roffsets, counter, bytes;
};
DsLayout ds_layout(int64_t n0, int64_t na);
hipError_t launch_downsample(const float4* map, int64_t n0, const float4* arr, int64_t na, float ds, void* scratch,
                             int32_t* counts, int32_t* offsets, int32_t* total, float4* out, int32_t** counter,
                             hipStream_t st);

// Stable LSD radix sort of n (key, value) pairs by the key's low `bits` bits (8 per pass), between a
// and b; -> the buffer that holds the result.  counts / offsets: 256 * sector_blocks(n) entries.
int2* launch_radix_sort(int2* a, int2* b, int32_t n, int bits, int32_t* counts, int32_t* offsets, int32_t* total,
                        hipStream_t st);

// The compactions' exclusive scan of nblk block counts by one workgroup; their sum to *total.
hipError_t launch_block_scan(const int32_t* counts, int nblk, int32_t* offsets, int32_t* total, hipStream_t st);
// The bounding box of the points of pts[0, n) whose x, y and z are finite: bbox[0..2] = min, bbox[3..5] =
// max as order-preserving words (float_unord, icp4r_device.hpp), reduced with integer atomics; no such
// point leaves min = +inf, max = -inf.  Shared by the k-NN index and the voxel grid.
hipError_t launch_finite_bbox(const float4* pts, int64_t n, uint32_t* bbox, hipStream_t st);

// ---- voxel-grid downsampling (icp4r_voxel.hip; include/icp4r/icp4r_voxel.h)
struct VoxelArgs {
    float inv[3];        // 1.0f / leaf, correctly rounded
    int32_t all_data;    // 0: the output intensity is 0
    uint32_t min_pts;    // voxels with fewer members give no output
};
// What voxel_grid_kernel leaves on the device (and the host entry reads back).
struct VoxelGridDev {
    int32_t min_b[3];
    int32_t div[3];
    int32_t flag;        // 0: a grid; 1: no participating point; -1: grid overflow
    int32_t pad;
};
struct VoxelLayout {  // byte offsets into the workspace
    size_t bbox, grid, tot, pa, pb, counts, offsets, heads, kept, bytes;
};
VoxelLayout voxel_layout(int64_t n);
// Stage 1: the bounding box and the grid of pts[0, n) (0 < n < 2^31) into the workspace.
hipError_t launch_voxel_grid(const float4* pts, int64_t n, const VoxelArgs& a, void* work, hipStream_t st);
// Stage 2, after stage 1 on the same stream: keys, sort by the key's low `bits` bits (31: any grid; the
// host entry passes the grid's own width), voxels, centroids.  out: room for n points; *count: the
// voxels written, or -1 on grid overflow (nothing written then).
hipError_t launch_voxel_filter(const float4* pts, int64_t n, const VoxelArgs& a, int bits, void* work, float4* out,
                               int32_t* count, hipStream_t st);

// ---- the incremental voxel grid (icp4r_voxel_acc.hip; include/icp4r/icp4r_voxel_acc.h)
constexpr int kAccAxisBits = 21;                   // a cell's biased offset from the origin per axis
constexpr int32_t kAccBias = 1 << (kAccAxisBits - 1);
constexpr int kAccMergeBlock = 2048;               // state elements per workgroup of the merge kernel
constexpr int kAccSmall = 8192;                    // scans of at most this many points: one workgroup sorts them in LDS
// The accumulator's device-resident head: what every add folds and every filter reads.
struct AccMeta {
    uint32_t bbox[6];    // the accumulated box of the participating points (order-preserving words)
    int32_t nvox;        // voxels in the current state buffer
    int32_t origin[3];   // the cell all keys are relative to (valid with have_origin)
    int32_t have_origin;
    int32_t range;       // sticky: a device add left the range and was skipped
    int32_t grid_flag;   // voxel_grid_from_bbox of bbox: 0 a grid, 1 no participating point, -1 overflow
    int32_t pad;
};
// What the prep kernel leaves for the other kernels of one add (and the host entry reads back).
struct AccScanInfo {
    int32_t skip;        // 0: merge; 1: no participating point; 2: outside the range
    int32_t minc[3];     // the scan's minimum cell
    int32_t ext[3];      // cells per axis of the scan's own box
    int32_t pad;
    int64_t cells;       // ext0 ext1 ext2 (saturated): <= INT32_MAX lets one sort do
};
// One sorted state buffer: voxel v is (key[v], sums[v], count[v]), keys ascending.
struct AccState {
    uint64_t* key;       // (oz << 42) | (oy << 21) | ox, biased offsets
    float4* sums;        // the four chains so far
    uint32_t* count;     // members so far
};
struct AccLayout {  // byte offsets into the add workspace of a scan of n points
    size_t bbox, info, tot, pkey, pa, pb, counts, offsets, skey, heads, posf, newrank, newkeys, bytes;
};
AccLayout acc_layout(int64_t n);
hipError_t launch_acc_clear(AccMeta* meta, hipStream_t st);
// Stage 1 of an add: the scan's box, the range rule, the fold into meta (sticky: a scan outside the
// range sets meta->range — the device entry; the host entry reads info back and refuses instead).
hipError_t launch_acc_prep(const float4* pts, int64_t n, const VoxelArgs& a, AccMeta* meta, void* work, int sticky,
                           hipStream_t st);
// Stage 2, after stage 1 on the same stream.  A scan of more than kAccSmall points is sorted by the
// store's radix sort — sort_bits > 0: one sort of the scan-relative key's low sort_bits bits (info.cells
// <= INT32_MAX); 0: two sorts of the 64-bit key's words.  max_vox: the
// host's bound on meta->nvox before the add.  Merges cur into next (room for max_vox + n voxels).
hipError_t launch_acc_merge(const float4* pts, int64_t n, const VoxelArgs& a, int sort_bits, AccMeta* meta,
                            const AccState& cur, const AccState& next, int64_t max_vox, void* work, hipStream_t st);
// The centroids of the state in key order to out (room for max_vox points) and their number to *count
// (-1: grid overflow, -2: the range flag; nothing written then).  scan: acc_filter_scan_bytes(max_vox)
// of block counts, offsets and one total, used when a.min_pts > 1.
size_t acc_filter_scan_bytes(int64_t max_vox);
hipError_t launch_acc_filter(const AccMeta* meta, const AccState& cur, int64_t max_vox, const VoxelArgs& a,
                             int32_t* scan, float4* out, int32_t* count, hipStream_t st);

// ---- the map's k-NN index and search (icp4r_map_knn.hip)
// A snapshot of the first `indexed` stored points: their float4 copy in Morton order (.w = the bits of
// the insertion position; a point with a non-finite coordinate, and the padding up to a whole leaf,
// hold NaN coordinates), boxes of the leaves (16 consecutive positions) and, above them, of every 64
// consecutive nodes of the level below, until a level has at most 64 nodes (or kKnnMaxLevels).
constexpr int kKnnLeaf = 16, kKnnFan = 64, kKnnMaxLevels = 4;
struct KnnIndex {
    const float4* sorted = nullptr;
    const float4* box[kKnnMaxLevels] = {};  // per level: (lo, hi) per node; level 0 = the leaves
    int32_t cnt[kKnnMaxLevels] = {};        // nodes per level
    int32_t levels = 0;                     // 0: no tree (nothing indexed)
    const uint32_t* bbox = nullptr;         // the finite points' bounding box, 6 order-preserving words
};
struct KnnLayout {  // byte offsets into the index buffer
    size_t sorted, box[kKnnMaxLevels], bbox, bytes;
    int32_t cnt[kKnnMaxLevels], levels;
};
KnnLayout knn_layout(int64_t n);
// Scratch of a sort of n pairs: two pair buffers, the radix counts and offsets, one int32.
struct KnnSortLayout {
    size_t pa, pb, counts, offsets, total, bytes;
};
KnnSortLayout knn_sort_layout(int64_t n);
// Builds the index of pts[0, n) (0 < n < 2^31) into `index` (knn_layout(n).bytes) with `scratch`
// (knn_sort_layout(n).bytes).
hipError_t launch_knn_index(const float4* pts, int64_t n, void* index, void* scratch, hipStream_t st);
KnnIndex knn_view(const void* index, int64_t n);
struct KnnSearch {
    const float4* pts;   // the store
    int64_t n;
    KnnIndex ix;         // the tree over [0, tail0) (levels = 0: none)
    int64_t tail0;       // [tail0, n) is swept through LDS tiles
    const float4* q;     // device queries
    int32_t nq, k;
    double md2;          // max_dist * max_dist
    float bound;         // md2 rounded up to float (-inf: nothing can match)
    float4* pout;        // any output may be null
    float* dout;
    int32_t* iout;
    int32_t* fout;
};
// scratch (knn_sort_layout(nq).bytes) sorts the queries by the index's Morton key; unused without a tree
hipError_t launch_knn_search(const KnnSearch& s, void* scratch, hipStream_t st);

// ---- radar ego velocity (icp4r_ego.hip)
struct EgoArgs {
    const float* rec;      // device records, 5 floats each
    const int64_t* off;    // [nscans] first record of scan s
    const int32_t* cnt;    // [nscans]
    int64_t stride;        // workspace points per scan (>= max cnt)
    float4* feat;          // [nscans * stride] distance, arfa, beta, v_r
    double4* pd;           // [nscans * stride] cos(DEG2RAD(beta)) v_r, cos / sin / DEG2RAD of arfa
    int32_t* scores;       // [nscans * max_h] inlier counts
    int32_t max_h;         // hypotheses of the largest scan
    int32_t iterations;    // icp4r_ego_params.iterations (<= 0: (int)(0.2 n) per scan)
    double sigma, dyn;
    uint64_t seed;
    uint8_t* mask;         // optional: static flag per record
    icp4r_ego_result* results;
};
hipError_t launch_ego(const EgoArgs& e, int nscans, int max_n, float4* xyzi, hipStream_t st);
hipError_t launch_ego_features(const EgoArgs& e, int nscans, int max_n, float4* xyzi, hipStream_t st);

// ---- the Doppler gate (icp4r_gate.hip; include/icp4r/icp4r_gate.h)
constexpr int kGateTile = 1024;  // points per (scan, tile) of the compaction: one wave, 16 mask bytes a lane
struct GateArgs {
    const float4* xyzi;    // device points, point i of scan s at off[s] + i
    const int64_t* off;    // [nscans]
    const int32_t* cnt;    // [nscans]; a count < 0 or > max_n packs nothing
    const uint8_t* mask;   // one byte per point, indexed like xyzi (unused when all != 0)
    int32_t nscans, max_n;
    int32_t tiles;         // tiles per scan: ceil(max_n / kGateTile), at least 1
    int32_t all;           // ICP4R_GATE_ALL: keep every point
    int32_t* counts;       // workspace [nscans * tiles]: kept points per tile
    int64_t* base;         // workspace [nscans * tiles]: first packed index per tile
    float4* clouds;        // out: the packed points
    int64_t* pair_off;     // out [nscans + 1]: [s0, s0, s1, ...]
    int32_t* pair_n;       // out [nscans + 1]
    const int32_t* bad;    // optional [nscans] (launch_gate_guard): results[s].status := ICP4R_E_INVALID where set
    icp4r_ego_result* results;
};
hipError_t launch_gate(const GateArgs& g, hipStream_t st);
// cnt_safe[s] = cnt[s] where the ego kernels stay inside a workspace of cap records (off[s] >= 0 and
// off[s] + min(cnt[s], max_n) <= cap), else 0 with bad[s] = 1
hipError_t launch_gate_guard(const int64_t* off, const int32_t* cnt, int nscans, int max_n, int64_t cap, int32_t* cnt_safe,
                             int32_t* bad, hipStream_t st);

// ---- generalized ICP (icp4r_gicp.hip): fast_gicp's LsqRegistration state per pair
struct GicpState {
    double R[9], t[3];  // x0 (row-major rotation, translation)
    double lambda;      // lm_lambda_ (< 0: not yet initialised)
};
// One iteration runs as three kernels over slices of each pair's source points (gicp_slices(n), a
// function of n only, so a pair's sums do not depend on the batch around it): the linearisation (its
// last slice solves the first kGicpSpec Levenberg-Marquardt trials), the trials' errors (its last
// slice decides), and the move of X.
constexpr int kGicpSys = 21 + 6 + 1 + 1;  // H (upper triangle), g, y, |valid|
constexpr int kGicpSpec = 2;             // LM trials evaluated per pass (the rest, rarely needed, one by one)
constexpr int kGicpMaxSlices = 64;
constexpr int kGicpGrid = 2048;
constexpr int kGicpKnnWaves = 16384;     // k-NN covariance walk: lanes per query up to 8 while the
                                         // grid stays within this many waves (0 lanes: this rule)          // workgroups per iteration kernel, about (a pair: at most its slices)
struct GicpTrial {
    double R[9], t[3];    // the trial transform delta * x0
    double dR[9], dt[3];  // delta
    double d[6];          // the LDLT step
    double lambda;
};
struct GicpCand {  // written by the linearisation's last slice, read by the trial kernel
    GicpTrial c[kGicpSpec];
    double lambda0;        // the iteration's first damping (lm_init * max|diag H| on the first iteration)
    double sys[kGicpSys];  // H, g, y0, |valid| at x0
    double R0[9], t0[3];   // x0
};
struct GicpArgs {
    GicpState* gs;        // [npairs]
    GicpCand* cand;       // [npairs]
    double* part_lin;     // [npairs][kGicpMaxSlices][kGicpSys] per-slice linearisation sums
    double* part_err;     // [npairs][kGicpMaxSlices][kGicpSpec] per-slice trial errors
    int32_t* cnt;         // [npairs] slices arrived (zero between launches)
    const double* cov_src;  // [npairs * x_stride * 6] regularised source covariances (upper triangle)
    const double* cov_tgt;  // [npairs * t_stride * 6]
    double* mah;          // [npairs * x_stride * 6] Mahalanobis of the current correspondences
    int64_t t_stride;
    double max_d2;        // corr_dist_threshold_² (float) as double
    double rot_eps, trans_eps, lm_init;
    int32_t lm_max_iterations, max_iterations;
    int32_t spec;         // LM trials evaluated speculatively, 0..kGicpSpec (plan option gicp_spec)
    int32_t grid;         // workgroups per iteration kernel, about (plan option gicp_grid)
};
hipError_t launch_gicp_init(const float* guess, GicpState* gs, int npairs, hipStream_t st);
hipError_t launch_gicp_cov(const float4* cloud, const int64_t* off, const int32_t* cnt, int npairs, int max_n,
                           int64_t stride, int k, int reg, double* cov, int lanes, hipStream_t st);
// k-NN covariances over a Morton index of the cloud itself (w.tsort / tbox / sbox, leaf 16; pairs whose
// w.state is invalid have no index and are skipped)
hipError_t launch_gicp_knn_cov(const float4* cloud, const int64_t* off, const int32_t* cnt, const WorkArgs& w,
                               int npairs, int max_n, int64_t stride, int k, int reg, double* cov, int lanes,
                               hipStream_t st);
// the number of pairs still iterating into *out and, if host_out, into pinned host memory
// host_out (pinned): (seq << 32) | the active count, one 64-bit store — a check's value is told apart from a
// stale one of an earlier call still in flight by its sequence number
hipError_t launch_gicp_active(const PairState* st, int npairs, int32_t* out, int64_t* host_out, uint32_t seq,
                              hipStream_t s);
hipError_t launch_gicp_iter(const PairArgs& a, const WorkArgs& w, const GicpArgs& g, int npairs, int max_n, int it,
                            hipStream_t st);

}  // namespace icp4r
