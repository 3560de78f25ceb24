/*
 * icp4r_map_knn.h — the scan-to-map store's batched exact k-nearest search (KD_TREE::Nearest_Search,
 * ikd_Tree.h:238) and the index behind it.  Included by icp4r/icp4r_map.h, whose header comment
 * states the contract; include that header.
 */
#ifndef ICP4R_MAP_KNN_H
#define ICP4R_MAP_KNN_H

#include "icp4r/icp4r_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/* KD_TREE::Nearest_Search, batched: the k nearest stored points of each of nq queries (the contract
 * in icp4r_map.h's header comment).  Row q of the outputs holds found[q] = min(k, #candidates) answers in
 * ascending (d, i): the point (float4), the squared distance (the reference's Point_Distance) and the
 * insertion position; its unused slots hold a zero point, distance +inf and index -1.  Any output
 * may be NULL.  An empty map gives found = 0 everywhere; nq = 0 writes nothing.  flags: 0 (the
 * index, or no index for maps too small to gain from one), ICP4R_MAP_KNN_BRUTE (every stored point,
 * no index: small maps, and the tests' second opinion) or ICP4R_MAP_KNN_INDEX (the index whatever the
 * size).  ICP4R_E_INVALID: unknown or both flags, k outside [1, ICP4R_MAP_KNN_MAX_K], nq < 0, NULL
 * queries with nq > 0, a stride below 12; ICP4R_E_TOO_LARGE: 2^31 stored points or more.
 * The host variant takes queries of stride_bytes (x, y, z first) and is synchronous; the device
 * variant takes float4 queries and device outputs and is asynchronous on hip_stream (NULL = the
 * context's stream) — except that a search which finds the index stale first rebuilds it on the
 * context's stream and waits for that. */
#define ICP4R_MAP_KNN_MAX_K 32
#define ICP4R_MAP_KNN_BRUTE 1
#define ICP4R_MAP_KNN_INDEX 2
int icp4r_map_nearest_search(icp4r_map* map, const float* queries, int64_t nq, int32_t stride_bytes, int32_t k,
                             double max_dist, int32_t flags, float* points_out, float* dist_out, int32_t* index_out,
                             int32_t* found_out);
int icp4r_map_nearest_search_device(icp4r_map* map, const float* d_queries, int64_t nq, int32_t k, double max_dist,
                                    int32_t flags, float* d_points, float* d_dist, int32_t* d_index, int32_t* d_found,
                                    void* hip_stream);

/* Brings the index up to date now (synchronous; nothing to do when it already covers the store).
 * icp4r_map_index_stats: how many points the index covers (0: none, or dropped by an edit), the tail
 * behind it, the tail size past which the next search rebuilds, and the builds so far. */
int icp4r_map_index_build(icp4r_map* map);
int icp4r_map_index_stats(const icp4r_map* map, int64_t* indexed, int64_t* tail, int64_t* tail_limit, int32_t* builds);

#ifdef __cplusplus
}
#endif

#endif /* ICP4R_MAP_KNN_H */
