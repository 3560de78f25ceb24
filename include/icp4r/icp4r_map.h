/*
 * icp4r_map.h — device-resident scan-to-map store and sector query.
 *
 * Replaces the reference's ikd-Tree map as radar_odometry uses it (a KD_TREE<pcl::PointXYZI>):
 *
 *   radar_odometry.cpp:92       KD_TREE<PointXYZI> ikd_Tree(0.3, 0.6, 0.5)   -> icp4r_map_create
 *   radar_odometry.cpp:347      ikd_Tree.Build(src->points)                  -> icp4r_map_build
 *   radar_odometry.cpp:348      ikd_Tree.set_downsample_param(0.5)           -> (no effect: the node
 *                               only calls Add_Points(.., false), which never downsamples)
 *   radar_odometry.cpp:382-390  pointAssociateToMap per point + Add_Points(scan_map, false)
 *                                                                            -> icp4r_map_add_scan
 *                               (or icp4r_map_add_points for world-frame points)
 *   radar_odometry.cpp:396      ikd_Tree.Sector_Search(p_now, 80, heading, SubMap->points)
 *                                                                            -> icp4r_map_sector_search
 *   third_party/ikd-Tree/ikd_Tree.cpp:415-419 (Sector_Search), 422-497 (Add_Points),
 *   1098-1140 (Search_by_sector), 1427-1448 (calc_dist, calc_heading)
 *
 * Sector_Search visits every node, so the store is a dense float4 (x, y, z, intensity) array in HBM,
 * in insertion order, and the query is a full filter at HBM bandwidth (ikd-Tree returns the same SET
 * in its tree's pre-order).  The keep test is the reference's, C precedence included:
 *
 *   (d2 <= r*r && |h - heading| < 60) || |h - heading| > 300
 *
 * with d2 and h = calc_heading(p, center) (degrees, 0 along +y, +90 along -x) in the reference's
 * float/double mix.  Points with |dh| > 300 are kept whatever their distance (the reference's
 * operator-precedence quirk); a point AT the centre has h = NaN and is never kept.
 *
 * Map maintenance (ikd_Tree.h:238-245; the node itself does not call these): Delete_Point_Boxes,
 * Box_Search, Radius_Search and the downsampling Add_Points(points, true).  Box membership is
 * half-open in float, min[k] <= p[k] && max[k] > p[k]; radius membership is calc_dist(p, c) <=
 * fl(r * r); a NaN coordinate or bound fails every comparison, so such a point is never found and
 * never deleted.  Deleting leaves the survivors dense and in insertion order.  ikd-Tree's rebuild
 * and rebalancing have no counterpart here.  They change no result of Box_Search or Radius_Search,
 * and none of Sector_Search while nothing has been deleted (the node never deletes).  After a
 * deletion or a downsampling add, however, the reference's Sector_Search may also return deleted
 * points with |dh| > 300: its keep test reads `!deleted && d2 <= r*r && dh < 60 || dh > 300`, so the
 * second branch ignores the flag, and a lazily deleted node stays in the tree until a rebuild
 * happens to drop it.  Which of them come back depends on the tree's rebalancing state; the store
 * compacts and never returns a deleted point (tests/test_map_reference.py, cases G1 and G2).
 * KD_TREE::size() differs in the same way: the reference counts lazily deleted nodes, the store
 * counts the points it holds.
 *
 * Nearest_Search (ikd_Tree.h:238, ikd_Tree.cpp:368-398 and :877-1021; its entries are declared in
 * icp4r/icp4r_map_knn.h, which this header includes) is the one query with an index behind it.  For a query q and the stored points p_i (i = the insertion position, as
 * icp4r_map_points_device shows it), d_i = calc_dist(q, p_i) in float, ((dx*dx) + dy*dy) + dz*dz
 * unfused; p_i is a candidate iff its three coordinates are finite and (double)d_i <= max_dist *
 * max_dist (the product in double: a negative max_dist acts as its magnitude, a NaN finds nothing, a
 * d_i that overflowed to +inf passes an infinite max_dist).  The answer is the min(k, #candidates)
 * smallest candidates by (d_i, i), ascending, each with its point, d_i and i.  A query with a
 * non-finite coordinate finds nothing.  The reference's tree gives the same distances (an exact
 * k-NN that never returns a lazily deleted node); among exactly equal d_i it keeps whichever its
 * traversal met first where the store keeps the lowest i, a stored point with a non-finite
 * coordinate is never returned (the reference's Build over NaN has no defined order), and k < 1,
 * undefined in the reference, is refused here as is k > ICP4R_MAP_KNN_MAX_K.
 *
 * The index is a snapshot the map owns: the points in Morton order with a 64-ary tree of boxes over
 * blocks of 16.  Build, Delete_Point_Boxes, the downsampling insert and growth of the store drop it;
 * a plain append (Add_Points(.., false), add_scan) leaves it and the appended points form a tail
 * that the search sweeps by brute force, until the tail would pass tail_limit and the next search
 * rebuilds the index.
 */
#ifndef ICP4R_MAP_H
#define ICP4R_MAP_H

#include "icp4r/icp4r.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct icp4r_map icp4r_map;

/* A map store on the context's device (uses the context's stream; one map per context is
 * typical, several are allowed).  A map may outlive its context: icp4r_destroy frees the device memory
 * of the context's maps and detaches them; every entry on a detached map then returns
 * ICP4R_E_INVALID ("the map's context was destroyed") without touching the device, and
 * icp4r_map_destroy only frees the host struct. */
int icp4r_map_create(icp4r_ctx* ctx, icp4r_map** out);
int icp4r_map_destroy(icp4r_map* map);

/* KD_TREE::Build: replace the contents with n points (x, y, z[, intensity]) of stride_bytes. */
int icp4r_map_build(icp4r_map* map, const float* pts, int64_t n, int32_t stride_bytes);

/* KD_TREE::Add_Points(points, false): append.  downsample_on must be 0 — the node's only call
 * (radar_odometry.cpp:390); this entry carries no box length, so a downsampling insert goes through
 * icp4r_map_add_points_downsample (downsample_on != 0: ICP4R_E_INVALID). */
int icp4r_map_add_points(icp4r_map* map, const float* pts, int64_t n, int32_t stride_bytes, int32_t downsample_on);

/* KD_TREE::Add_Points(points, true) with downsample box box_length (finite, > 0; ikd_Tree.cpp:430-457).
 * Of every downsample cell (floorf(p / box_length) per axis) that an arriving point falls in, only
 * the point nearest to the cell's centre stays, among the cell's stored points and its arrivals: an
 * arrival wins a tie against a stored point, the last tied arrival among arrivals, the lowest index
 * among stored points.  Stored points of other cells, and stored points outside their own cell's
 * float box, stay.  Surviving stored points keep their places; surviving arrivals follow in input
 * order.  *counter = the reference's return value (the arrivals its sequential loop re-inserts). */
int icp4r_map_add_points_downsample(icp4r_map* map, const float* pts, int64_t n, int32_t stride_bytes,
                                    float box_length, int64_t* counter);

/* KD_TREE::Delete_Point_Boxes: removes the points inside any of the nb boxes (nb x 6 floats: min xyz,
 * max xyz); *deleted = how many (a point in several boxes counts once).  The survivors stay dense and
 * in insertion order; the capacity never shrinks.  nb = 0 deletes nothing. */
int icp4r_map_delete_boxes(icp4r_map* map, const float* boxes, int32_t nb, int64_t* deleted);

/* pointAssociateToMap + Add_Points(.., false) for one scan: p_w = R * p + t in double (R row-major
 * 3x3 = Rtrans, t = t_w_curr; per row ((R0*x + R1*y) + R2*z) + t), stored as float, intensity
 * copied.  world_out (optional, host, n x 4 floats) receives the world-frame scan (`scan_map`). */
int icp4r_map_add_scan(icp4r_map* map, const float* scan, int64_t n, int32_t stride_bytes, const double* R,
                       const double* t, float* world_out);

int icp4r_map_size(const icp4r_map* map, int64_t* n);

/* KD_TREE::Sector_Search(center, radius, heading_deg, Storage): the kept points, insertion order,
 * to host memory (float4 each).  Writes at most out_cap points; *out_n = the number kept (if it
 * exceeds out_cap the call returns ICP4R_E_TOO_LARGE and writes nothing).  Synchronous. */
int icp4r_map_sector_search(icp4r_map* map, const float* center, float radius, float heading_deg, float* out,
                            int64_t out_cap, int64_t* out_n);

/* Device-resident variant for scan-to-map registration: writes the kept points (float4) to d_out
 * (device, capacity >= icp4r_map_size) and their count to *d_count (device int32 — usable directly
 * as icp4r_batch.tgt_n).  Asynchronous on hip_stream (NULL = the context's stream). */
int icp4r_map_sector_search_device(icp4r_map* map, const float* center, float radius, float heading_deg,
                                   float* d_out, int32_t* d_count, void* hip_stream);

/* KD_TREE::Box_Search / Radius_Search (radius >= 0): the stored points inside the box (6 floats) /
 * within the radius of center, insertion order; arguments and overflow as icp4r_map_sector_search
 * and icp4r_map_sector_search_device. */
int icp4r_map_box_search(icp4r_map* map, const float* box6, float* out, int64_t out_cap, int64_t* out_n);
int icp4r_map_radius_search(icp4r_map* map, const float* center, float radius, float* out, int64_t out_cap,
                            int64_t* out_n);
int icp4r_map_box_search_device(icp4r_map* map, const float* box6, float* d_out, int32_t* d_count, void* hip_stream);
int icp4r_map_radius_search_device(icp4r_map* map, const float* center, float radius, float* d_out, int32_t* d_count,
                                   void* hip_stream);

/* The stored points (device, float4, insertion order) and their count; an edit (delete, downsampled
 * insert, growth) moves them. */
int icp4r_map_points_device(icp4r_map* map, const float** d_points, int64_t* n);

/* Average device time (HIP events) of the search, delete, downsampled-insert and index-build launches since the
 * last icp4r_map_time_reset, and how many there were. */
int icp4r_map_time_ms(icp4r_map* map, double* avg_ms, int32_t* calls);
int icp4r_map_time_reset(icp4r_map* map);

#ifdef __cplusplus
}
#endif

/* KD_TREE::Nearest_Search and the map's index: icp4r_map_nearest_search[_device],
 * icp4r_map_index_build, icp4r_map_index_stats. */
#include "icp4r/icp4r_map_knn.h"

#endif /* ICP4R_MAP_H */
